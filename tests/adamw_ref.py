"""Adam with decoupled weight decay (torch.optim.AdamW) restated in plain numpy on the CPU — TEST
INFRASTRUCTURE ONLY.

Restated from torch's definition (``param.mul_(1 - lr * wd)``, then the Adam step on the plain
gradient: exp_avg.lerp_, exp_avg_sq.mul_.addcmul_, addcdiv_ with both bias corrections), not
derived from the kernels' output.  No GPU, no project imports.  ``dtype``: float64 is the
reference, float32 the yardstick a bound is measured with (tests/test_adamw_cpu.py); numpy rounds
every fp32 operation once (no fma contraction).

* ``make_scalars``: the per-step scalars computed in double and rounded to fp32 (``rounded=False``:
  left in double, for the comparison with torch itself), with the step's ``decay = 1 - lr * wd``.
* ``adamw_step``: one step of every element with gradient ``g`` (0 where a row got none).
* ``zero_step_folded``: the zero-gradient step with the folded constants ra, rb.
* ``replay``: the zero-gradient steps stamp+1 .. target a row owes, each with its own step's lr
  and weight decay.
* ``dense_schedule``: every row of the table every step, gradient or not.
* ``step_table``: the decoupled step table, STRIDE floats per step (include/ncf_hip.h).
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
LOCK = 0x40000000       # NCF_STAMP_LOCK
STRIDE = 8              # NCF_ADAMW_TABLE_STRIDE
HP = (0.9, 0.999, 1e-8, 1e-2)   # beta1, beta2, eps, weight decay (torch.optim.AdamW's default)


def make_scalars(lr, hp, t, rounded=True):
    """The scalars of step t (1-based): fp32 values, or doubles with ``rounded=False``."""
    b1, b2, eps, wd = hp
    bc1 = 1.0 - math.pow(b1, float(t))
    bc2 = 1.0 - math.pow(b2, float(t))
    ns = -(lr / bc1)
    s = dict(neg_step=ns, w1=1.0 - b1, b2=b2, c2=1.0 - b2, inv_bc=1.0 / math.sqrt(bc2), eps=eps,
             b1=b1, decay=1.0 - lr * wd,
             ra=(1.0 / math.sqrt(bc2)) / ns if ns != 0.0 else -3.0e38,
             rb=eps / ns if ns != 0.0 else -3.0e38)
    return {k: F32(v) for k, v in s.items()} if rounded else s


def adamw_step(p, m, v, g, lr, t, hp, dtype=F64, s=None):
    """(p, m, v) after step t with gradient g: the decay multiplies p first, then the Adam term of
    the plain gradient is added; the arithmetic in ``dtype``."""
    s = s or make_scalars(lr, hp, t)
    c = {k: dtype(x) for k, x in s.items()}
    p, m, v, g = (np.asarray(x, dtype=dtype) for x in (p, m, v, g))
    p = p * c["decay"]
    m = m + c["w1"] * (g - m)
    v = v * c["b2"] + c["c2"] * g * g
    p = p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"])
    return p, m, v


def zero_step_folded(p, m, v, s, dtype=F32):
    """The step of an element whose gradient is zero, neg_step folded into the denominator."""
    c = {k: dtype(x) for k, x in s.items()}
    p, m, v = (np.asarray(x, dtype=dtype) for x in (p, m, v))
    m = c["b1"] * m
    v = v * c["b2"]
    with np.errstate(under="ignore"):
        p = p * c["decay"] + m / (np.sqrt(v) * c["ra"] + c["rb"])
    return p, m, v


def _zero(p, m, v, s, dtype):
    if dtype == F32:
        return zero_step_folded(p, m, v, s, F32)
    return adamw_step(p, m, v, 0.0, None, None, None, dtype, s=s)


def replay(p, m, v, stamps, target, lr_of_step, hp_of_step, dtype=F64, skip=(), scalars=None,
           zero=None):
    """Rows [rows, D] of one table: every row r not in ``skip`` takes the zero-gradient steps
    stamps[r]+1 .. target (``target`` a step or one per row), step t with lr_of_step(t) and
    hp_of_step(t) (a tuple is the same at every step).  In float32 the step is
    zero_step_folded.  ``scalars(t)``, ``zero(p, m, v, s, dtype)``: replacements (mutants)."""
    hp = hp_of_step if callable(hp_of_step) else (lambda t: hp_of_step)
    scalars = scalars or (lambda t: make_scalars(lr_of_step(t), hp(t), t))
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


def dense_schedule(p, m, v, touched, lr_of_step, hp_of_step, steps, dtype=F64, first=1):
    """Every row every step first .. first+steps-1; touched[i] = (row ids, G [n, D]) of step
    first+i.  In float32 the rows without a gradient take zero_step_folded."""
    hp = hp_of_step if callable(hp_of_step) else (lambda t: hp_of_step)
    p, m, v = (np.array(x, dtype=dtype) for x in (p, m, v))
    for i in range(steps):
        t = first + i
        ids, G = touched[i]
        s = make_scalars(lr_of_step(t), hp(t), t)
        has = np.zeros(p.shape[0], bool)
        has[ids] = True
        g = np.zeros(p.shape, dtype)
        g[ids] = np.asarray(G, dtype=dtype)
        if dtype == F32:
            a = adamw_step(p, m, v, g, None, None, None, F32, s=s)
            b = zero_step_folded(p, m, v, s, F32)
            p, m, v = (np.where(has[:, None], x, y) for x, y in zip(a, b))
        else:
            p, m, v = adamw_step(p, m, v, g, None, None, None, dtype, s=s)
    return p, m, v


def step_table(lr_of_step, hp_of_step, upto):
    """[STRIDE (upto + 1)] fp32: [8s .. 8s+4] = neg_step, inv_bc2_sqrt, ra, rb, decay of step s
    (s >= 1), the rest zero."""
    hp = hp_of_step if callable(hp_of_step) else (lambda t: hp_of_step)
    out = np.zeros(STRIDE * (upto + 1), F32)
    for t in range(1, upto + 1):
        s = make_scalars(lr_of_step(t), hp(t), t)
        out[STRIDE * t:STRIDE * t + 5] = (s["neg_step"], s["inv_bc"], s["ra"], s["rb"], s["decay"])
    return out
