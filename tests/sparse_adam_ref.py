"""torch.optim.SparseAdam restated in plain numpy on the CPU, and the case the SparseAdam tests
run on (not a test module).  No GPU, no project imports.

Restated from torch's definition (torch/optim/_functional.py, sparse_adam), for the rows a
coalesced gradient names and no others:

    m += (1 - b1) (g - m);   v += (1 - b2) (g^2 - v)
    p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)

``dtype`` float64 is the reference (tests/test_bag_sparse_cpu.py holds it to torch.optim.SparseAdam
itself); float32 is the yardstick a bound is measured with: the scalars a kernel is handed
(the step size, 1 - b1, b2, 1 - b2, eps, computed in double and rounded once) and every operation
rounded once (numpy: no fma contraction).  The bound of a quantity is ``MARGIN`` x the float32
restatement's worst distance from float64 on the case's own inputs, p absolute, m and v relative
to the float64 value: the rule and the margin of tests/test_gpu_adam.py (the margin is that file's
allowance for explicit fmas and the hardware square root and reciprocal, ~1 ulp each).  Nothing is
fitted to a kernel's output.

The case: |p| in [0.2, 0.5] with a random sign; gradients carry p's sign, so no m passes through
zero (where a relative distance measures the cancellation, not the arithmetic); 5 steps with a
changing lr; each step names its own random third of the rows, so rows skip steps, come back, and
a quarter of the rows is never named."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = 4.0
ROWS = 1000
BETAS, EPS = (0.9, 0.999), 1e-8
LRS = (1e-3, 1e-3, 3e-4, 2e-3, 7e-4)


def step_size(lr, betas, t):
    return lr * math.sqrt(1.0 - betas[1] ** t) / (1.0 - betas[0] ** t)


def sparse_adam_step(p, m, v, ids, g, lr, t, betas=BETAS, eps=EPS, dtype=F64):
    """Step t (1-based) of the rows ``ids`` (unique) with gradient rows ``g``, in place."""
    b1, b2 = betas
    if dtype == F64:
        ss, w1, c2, e = step_size(lr, betas, t), 1.0 - b1, 1.0 - b2, eps
    else:
        ss, w1, c2, e = (dtype(x) for x in (step_size(lr, betas, t), 1.0 - b1, 1.0 - b2, eps))
    gg = np.asarray(g, dtype=dtype)
    mm, vv = m[ids], v[ids]
    mm = mm + w1 * (gg - mm)
    vv = vv + c2 * (gg * gg - vv)
    m[ids], v[ids] = mm, vv
    p[ids] = p[ids] - ss * mm / (np.sqrt(vv) + e)


def run(case, dtype=F64, first=1, state=None, steps=None, step_shift=0):
    """(p, m, v) after the case's steps in ``dtype``; ``step_shift``: a mutant's step count."""
    if state is None:
        p = case["p"].astype(dtype)
        m, v = np.zeros_like(p), np.zeros_like(p)
    else:
        p, m, v = (x.astype(dtype).copy() for x in state)
    for i, (ids, g, lr) in enumerate(case["steps"] if steps is None else steps):
        sparse_adam_step(p, m, v, ids, g, lr, first + i + step_shift, dtype=dtype)
    return p, m, v


def make_case(dim, seed=0):
    g = np.random.default_rng(7000 + 10 * dim + seed)
    sign = np.where(g.random((ROWS, dim)) < 0.5, -1.0, 1.0)
    p = (sign * g.uniform(0.2, 0.5, (ROWS, dim))).astype(F32)
    pool = np.nonzero(np.arange(ROWS) % 4 != 3)[0]          # rows 3, 7, 11, ...: never named
    steps = []
    for lr in LRS:
        ids = np.sort(g.permutation(pool)[:ROWS // 3]).astype(np.int64)
        vals = (sign[ids] * (1e-4 + np.abs(g.normal(0.0, 1e-2, (ids.size, dim))))).astype(F32)
        steps.append((ids, vals, lr))
    touched = np.zeros(ROWS, bool)
    touched[np.concatenate([s[0] for s in steps])] = True
    assert (~touched).sum() >= ROWS // 4
    counts = np.bincount(np.concatenate([s[0] for s in steps]), minlength=ROWS)
    assert counts.max() >= 3 and (counts == 1).any()         # rows that come and go
    return dict(dim=dim, p=p, steps=steps, touched=touched)


def distance(got, ref, touched):
    """{p, m, v}: worst |got - ref| over the touched rows, absolute for p, relative for m, v."""
    out = {}
    for q, a, b in zip("pmv", got, ref):
        d = np.abs(np.asarray(a, dtype=F64)[touched] - b[touched])
        if q != "p":
            d = d / np.abs(b[touched])
        out[q] = float(np.where(np.isfinite(d), d, np.inf).max())
    return out


def bounds(case, ref=None):
    """MARGIN x the float32 restatement's distance from the float64 one, per quantity."""
    ref = ref or run(case, F64)
    fp = distance(run(case, F32), ref, case["touched"])
    return {q: MARGIN * x for q, x in fp.items()}, fp
