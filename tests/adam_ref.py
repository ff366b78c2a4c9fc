"""The fp32 table / flat Adam restated in plain numpy on the CPU — TEST INFRASTRUCTURE ONLY.

Restated from torch.optim.Adam's definition as csrc/adam.hip:4-7 states it (coupled L2, the lerp
form of exp_avg, both bias corrections), not derived from the kernels' output.  No GPU, no
project imports.  ``dtype``: float64 is the reference, float32 the yardstick a bound is measured
with (tests/test_adam_cpu.py); numpy rounds every fp32 operation once (no fma contraction).

* ``make_scalars``: csrc/adam_math.h's make_scalars, the per-step scalars computed in double and
  rounded to fp32 (the `lr == 0` constants of the zero-gradient form included).
* ``adam_step``: one step of every element with gradient ``g`` (0 where a row got none).
* ``zero_step_folded``: adam0, the zero-gradient step with the folded constants k1, k2, ra, rb.
* ``replay``: the zero-gradient steps stamp+1 .. target a row owes, each with its own step's lr.
* ``dense_schedule``: every row of the table every step, gradient or not.
* ``step_table``: ncf_adam_step_scalars' four floats per step; ``splitmix_seed``: clock_advance.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
LOCK = 0x40000000       # NCF_STAMP_LOCK
HP = (0.9, 0.999, 1e-8, 1e-5)   # beta1, beta2, eps, weight decay: the project's


def make_scalars(lr, hp, t):
    """AdamScalars of step t (1-based) as fp32 values."""
    b1, b2, eps, wd = hp
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    ns = -(lr / bc1)
    s = dict(neg_step=ns, w1=1.0 - b1, b2=b2, c2=1.0 - b2, inv_bc=1.0 / math.sqrt(bc2), eps=eps,
             wd=wd, b1=b1, k1=(1.0 - b1) * wd, k2=(1.0 - b2) * wd * wd,
             ra=(1.0 / math.sqrt(bc2)) / ns if ns != 0.0 else -3.0e38,
             rb=eps / ns if ns != 0.0 else -3.0e38)
    return {k: F32(v) for k, v in s.items()}


def adam_step(p, m, v, g, lr, t, hp, dtype=F64, s=None):
    """(p, m, v) after step t with gradient g; the scalars rounded as make_scalars rounds them,
    the arithmetic in ``dtype``."""
    s = s or make_scalars(lr, hp, t)
    c = {k: dtype(x) for k, x in s.items()}
    p, m, v, g = (np.asarray(x, dtype=dtype) for x in (p, m, v, g))
    g = g + c["wd"] * p
    m = m + c["w1"] * (g - m)
    v = v * c["b2"] + c["c2"] * g * g
    p = p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"])
    return p, m, v


def zero_step_folded(p, m, v, s, dtype=F32):
    """adam0: the step of an element whose gradient is zero, constants folded."""
    c = {k: dtype(x) for k, x in s.items()}
    p, m, v = (np.asarray(x, dtype=dtype) for x in (p, m, v))
    m = c["b1"] * m + c["k1"] * p
    v = c["k2"] * p * p + v * c["b2"]
    with np.errstate(under="ignore"):
        p = p + m / (np.sqrt(v) * c["ra"] + c["rb"])
    return p, m, v


def _zero(p, m, v, s, dtype):
    if dtype == F32:
        return zero_step_folded(p, m, v, s, F32)
    return adam_step(p, m, v, 0.0, None, None, None, dtype, s=s)


def replay(p, m, v, stamps, target, lr_of_step, hp, dtype=F64, skip=(), scalars=None, zero=None):
    """Rows [rows, D] of one table: every row r not in ``skip`` takes the zero-gradient steps
    stamps[r]+1 .. target (``target`` a step or one per row).  In float32 the step is
    zero_step_folded.  ``scalars(t)``, ``zero(p, m, v, s, dtype)``: replacements (mutants)."""
    scalars = scalars or (lambda t: make_scalars(lr_of_step(t), hp, t))
    zero = zero or _zero
    p, m, v = (np.array(x, dtype=dtype) for x in (p, m, v))
    stamps = np.asarray(stamps, dtype=np.int64)
    to = np.broadcast_to(np.asarray(target, dtype=np.int64), stamps.shape)
    live = np.ones(stamps.shape, bool)
    live[list(skip)] = False
    live &= stamps < to
    if not live.any():
        return p, m, v
    for q in range(int(stamps[live].min()) + 1, int(to[live].max()) + 1):
        r = np.nonzero(live & (stamps < q) & (q <= to))[0]
        if r.size:
            p[r], m[r], v[r] = zero(p[r], m[r], v[r], scalars(q), dtype)
    return p, m, v


def dense_schedule(p, m, v, touched, lr_of_step, hp, steps, dtype=F64, first=1):
    """Every row every step first .. first+steps-1; touched[i] = (row ids, G [n, D]) of step
    first+i.  In float32 the rows without a gradient take zero_step_folded."""
    p, m, v = (np.array(x, dtype=dtype) for x in (p, m, v))
    for i in range(steps):
        t = first + i
        ids, G = touched[i]
        s = make_scalars(lr_of_step(t), hp, t)
        has = np.zeros(p.shape[0], bool)
        has[ids] = True
        g = np.zeros(p.shape, dtype)
        g[ids] = np.asarray(G, dtype=dtype)
        if dtype == F32:
            a = adam_step(p, m, v, g, None, None, None, F32, s=s)
            b = zero_step_folded(p, m, v, s, F32)
            p, m, v = (np.where(has[:, None], x, y) for x, y in zip(a, b))
        else:
            p, m, v = adam_step(p, m, v, g, None, None, None, dtype, s=s)
    return p, m, v


def step_table(lr_of_step, hp, upto):
    """[4 (upto + 1)] fp32: [4s .. 4s+3] = neg_step, inv_bc2_sqrt, ra, rb of step s (s >= 1)."""
    out = np.zeros(4 * (upto + 1), F32)
    for t in range(1, upto + 1):
        s = make_scalars(lr_of_step(t), hp, t)
        out[4 * t:4 * t + 4] = (s["neg_step"], s["inv_bc"], s["ra"], s["rb"])
    return out


def splitmix_seed(base, t):
    """clock->seed after the advance to clock->t = t."""
    M = (1 << 64) - 1
    z = (base + 0x9E3779B97F4A7C15 * (t + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return (z ^ (z >> 31)) & 0x3FFFFFFFFFFFFFFF
