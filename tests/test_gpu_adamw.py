"""The decoupled-weight-decay (torch.optim.AdamW) forms of csrc/adam.hip, one entry point at a time,
against float64 (tests/adamw_ref.py), on the MI355X: every pair entry point that replays, with
NCF_ADAM_DECOUPLED set, at every width with the gaps that straddle replay_uniform's 8-step chunks;
every gradient-step entry point over three steps (ncf_embedding_bwd_reduce_apply_clock with the
flag among them, behind its own LayerNorm backward); 40 steps of the deferred schedule's own call
sequence against the dense schedule; the refusals.  The geometry (widths, rows, list sizes, gaps)
and the device plumbing are tests/test_gpu_adam.py's.

Each check takes the implementation under test as an argument: here it is the kernel;
tests/test_adamw_cpu.py runs the same check, on the same inputs, with the fp32 restatement (which
must pass with a quarter of every bound used) and with mutants (which must fail).

Bounds, none fitted to the GPU's output: for each quantity of each case 4 x the worst distance of
the fp32 restatement (numpy: every operation rounded once) from float64 on that case's own inputs;
p absolute, m and v relative to the float64 value over the elements whose moments are not zero.
The figures stand in REPLAY_FP32 / GRAD_FP32 / SCHED_FP32; tests/test_adamw_cpu.py re-measures them.

Inputs of the replay cases: |p| in [0.35, 0.5], random sign, and two moment populations: "touched
history" (the odd rows at most 9 steps behind: |m| = 2e-2 + |N(0, 1e-2)| with p's sign,
v ~ U(1e-5, 1e-3)) and "never touched" (m = v = 0 exactly).  A never-touched row must come back
with m == v == 0 bitwise and p equal, bitwise, to p multiplied by each owed step's decay, every
product rounded to fp32 (which is what the fp32 restatement computes for such a row).
Weight decay 0.5 (0.25 after a wd change): one owed step then moves a never-touched element by
lr wd |p| >= 3e-4 * 0.25 * 0.35 = 2.6e-5, above 20 x the p bound (the sensitivity condition,
tests/test_adamw_cpu.py); torch's default 1e-2 would move it by 1e-6, less than one bound.  With
wd = 0 a never-touched row does not move at all: there it is held bitwise and the condition is
held on m of the touched-history rows, which every owed step shrinks by a tenth.
The entry points are called with weight_decay = WD_ARG, a value no case uses: with the flag the
decay comes from the step table alone.
"""
import functools

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import adamw_ref as W
from tests import embed_ref as R
from tests import test_gpu_adam as G
from tests import test_gpu_embed as E

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = G.DEV

F32, F64, LOCK = W.F32, W.F64, W.LOCK
WIDTHS, ROWS, MAX_N, COUNT, GAPS, PAD, NAMES = (G.WIDTHS, G.ROWS, G.MAX_N, G.COUNT, G.GAPS, G.PAD,
                                                G.NAMES)
B1, B2, EPS = W.HP[:3]
WD, WD_LATE, WD_ARG = 0.5, 0.25, 7.0
REPLAY_CASES = ((17, "base"), (330, "base"), (330, "wd0"), (330, "lr_change"), (330, "lr0"),
                (330, "wd_change"))
lr_of = G.lr_of


def hp_of(target, variant):
    """(beta1, beta2, eps, wd) of step t.  wd_change: 0.5 up to step target - 30, 0.25 after."""
    if variant == "wd0":
        return lambda t: (B1, B2, EPS, 0.0)
    if variant == "wd_change":
        return lambda t: (B1, B2, EPS, WD if t <= target - 30 else WD_LATE)
    return lambda t: (B1, B2, EPS, WD)


def segments(lr, hp, upto):
    """[(first, last, lr, wd)]: the calls of deferred.adamw_step_scalars that fill steps 1 .. upto,
    one per run of equal (lr, wd), as deferred._ensure refills from the step a change takes effect."""
    key = lambda t: (lr(t), hp(t)[3])   # noqa: E731
    seg, first = [], 1
    for t in range(2, upto + 2):
        if t == upto + 1 or key(t) != key(first):
            seg.append((first, t - 1) + key(first))
            first = t
    return seg


# ----------------------------------------------------------------------------- inputs
def _tables(g, rows, D, touched_rows):
    out = {}
    for tb in (0, 1):
        sign = np.where(g.random((rows, D)) < 0.5, -1.0, 1.0)
        p = sign * g.uniform(0.35, 0.5, (rows, D))
        mt = sign * (2e-2 + np.abs(g.normal(0.0, 1e-2, (rows, D))))
        vt = g.uniform(1e-5, 1e-3, (rows, D))
        t = touched_rows[:, None]
        out[f"p{tb}"] = p.astype(F32)
        out[f"m{tb}"] = np.where(t, mt, 0.0).astype(F32)
        out[f"v{tb}"] = np.where(t, vt, 0.0).astype(F32)
    return out


@functools.lru_cache(maxsize=8)
def replay_case(D, target, variant):
    """tests/test_gpu_adam.py's replay_case with the two populations above: two kinds of table
    pairs behind ``target`` by GAPS, 97 / 3 rows listed in id buffers of 128, some listed rows
    locked, some ahead, raw id lists for the claim form; the float64 and the fp32 replay of every
    row that is behind and not locked."""
    g = np.random.default_rng(2000 * D + target + 11 * len(variant))
    kinds = []
    for k, rows in enumerate(ROWS):
        perm = g.permutation(rows)
        ids = np.concatenate([perm[:COUNT[k]], np.resize(perm[COUNT[k]:], MAX_N - COUNT[k])])
        gap = np.array([GAPS[(5 * r + 3) % 16] for r in range(rows)])
        gap[ids[:COUNT[k]]] = [GAPS[c % 16] for c in range(COUNT[k])]
        gap = np.minimum(gap, target)
        stamp = (target - gap).astype(np.int32)
        touched = (gap <= 9) & (np.arange(rows) % 2 == 1)
        t = _tables(g, rows, D, touched)
        listed = ids[:COUNT[k]]
        locked = [listed[c] for c in (5, 37, 70) if c < COUNT[k]] + [perm[-1]]
        ahead = [listed[c] for c in (11, 50) if c < COUNT[k]]
        if k == 1:
            locked, ahead = [perm[-1]], [listed[2]]
        stamp[locked] |= LOCK
        stamp[ahead] = target + 1
        raw = np.concatenate([np.repeat(listed, 1 + np.arange(COUNT[k]) % 3), listed[::2],
                              listed[::3], listed[::-5], [-1, rows, -7, rows + 100, 2 ** 40]])
        kinds.append(dict(t, stamp=stamp, ids=ids.astype(np.int64), count=COUNT[k], rows=rows,
                          raw=raw.astype(np.int64), never=~touched))
    n = max(len(kd["raw"]) for kd in kinds)
    for kd in kinds:
        kd["raw"] = np.concatenate([kd["raw"], np.full(n - len(kd["raw"]), -1, np.int64)])
    c = dict(D=D, target=target, variant=variant, hp=hp_of(target, variant),
             lr=lr_of(target, variant), kinds=kinds, t_now=target - 1, rel=1)
    c["ref"] = replay_all(c, target, F64)
    c["f32"] = replay_all(c, target, F32)
    return c


def replay_all(c, target, dtype, **kw):
    """Every row behind ``target`` and not locked, replayed to it, in ``dtype``."""
    out = []
    for kd in c["kinds"]:
        r = {}
        for tb in (0, 1):
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = W.replay(
                kd[f"p{tb}"], kd[f"m{tb}"], kd[f"v{tb}"], kd["stamp"], target, c["lr"], c["hp"],
                dtype, **kw)
        out.append(r)
    return out


def _err(got, ref, q):
    """Worst |got - ref|: absolute for p; for m and v relative to the float64 value, over the
    elements where that is not zero (where it is, the value must be an exact zero)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    if q != "p":
        z = ref == 0
        if z.any() and bool((got[z] != 0).any()):
            return float("inf")
        d = d[~z] / np.abs(ref[~z])
        if d.size == 0:
            return 0.0
    d = np.where(np.isfinite(d), d, np.inf)
    return float(d.max())


def measure_replay(c):
    out = {}
    for k, kd in enumerate(c["kinds"]):
        b = G.behind(kd, c["target"])
        for n in NAMES:
            out[n[0]] = max(out.get(n[0], 0.0), _err(c["f32"][k][n][b], c["ref"][k][n][b], n[0]))
    return out


def replay_sensitivity(c):
    """{p, m}: the smallest change the last owed step makes, from the float64 reference: p over
    every replayed element (wd = 0: over the touched-history rows, the others stand still), m
    relative over the touched-history rows."""
    prev = replay_all(c, c["target"] - 1, F64)
    out = {"p": np.inf, "m": np.inf}
    for k, kd in enumerate(c["kinds"]):
        b = G.behind(kd, c["target"])
        bt = b & ~kd["never"]
        for n in ("p0", "p1"):
            rows = bt if c["variant"] == "wd0" else b
            d = np.abs(c["ref"][k][n][rows] - prev[k][n][rows])
            out["p"] = min(out["p"], float(d.min()) if d.size else np.inf)
        for n in ("m0", "m1"):
            d = np.abs(c["ref"][k][n][bt] - prev[k][n][bt]) / np.abs(c["ref"][k][n][bt])
            out["m"] = min(out["m"], float(d.min()) if d.size else np.inf)
    return out


# ----------------------------------------------------------------------------- replay: who, where
REPLAY_ENTRIES = (
    [("pairs_catchup_clock", None), ("pairs_catchup_lock_clock", 0), ("pairs_catchup_lock_clock", 1),
     ("pairs_catchup_claim_clock", None), ("reduce_batch_catchup", None)] +
    [(n, e) for n in ("pairs_sweep_rolling", "pairs_sweep_rolling_part") for e in (8, 3, 64)])


def check_replay(D, entry, impl, cases=REPLAY_CASES):
    """``impl(entry, case)`` -> per kind dict(p0 .. v1, stamp) after the call.  p, m, v of the
    replayed rows against float64; the never-touched rows among them bitwise (m == v == 0, p the
    fp32 product of the owed decays); stamps exactly; every row the entry point must skip
    bit-unchanged.  Returns the worst fraction of its bound per quantity."""
    worst = {}
    for target, variant in cases:
        c = replay_case(D, target, variant)
        got = impl(entry, c)
        fp = REPLAY_FP32[(D, target, variant)]
        for k, (kd, (rep, after, tabs)) in enumerate(zip(c["kinds"], G.plan(entry, c))):
            tag = (entry, D, target, variant, k)
            assert np.array_equal(got[k]["stamp"], after), (tag, "stamp")
            nv = rep & kd["never"]
            for n in NAMES:
                x = got[k][n]
                assert np.array_equal(x[~rep].view(np.int32), kd[n][~rep].view(np.int32)), \
                    (tag, n, "a skipped row changed")
                want = c["f32"][k][n][nv] if n[0] == "p" else np.zeros_like(x[nv])
                assert np.array_equal(x[nv].view(np.int32), want.view(np.int32)), \
                    (tag, n, "a never-touched row is not the product of its owed decays")
                f = G._frac(_err(x[rep], c["ref"][k][n][rep], n[0]), fp[n[0]])
                worst[n[0]] = max(worst.get(n[0], 0.0), f)
                assert f < 1.0, (tag, n, f)
    return worst


# ----------------------------------------------------------------------------- gradient steps
FIRST = G.FIRST
GRAD_ENTRIES = ("table", "table_dense_grad", "flat", "flat_clock", "flat_clock_close",
                "pairs_apply_clock")


def grad_cases(entry):
    if entry == "table":
        return [("table", 16, "null"), ("table", 64, "slot"), ("table", 256, "big")]
    if entry == "table_dense_grad":
        return [("dense", 64, "zeros")]
    if entry.startswith("flat"):
        return [("flat", n, "") for n in (5, 1027, G.FLAT_BIG[entry])]
    return [("apply", D, "") for D in WIDTHS]


@functools.lru_cache(maxsize=4)
def grad_case(family, a, b):
    """tests/test_gpu_adam.py's inputs of the case (tables with non-zero moments of both
    populations, three steps of gradients) under AdamW's rule at wd = 0.5."""
    c = dict(G.grad_case(family, a, b), hp=(B1, B2, EPS, WD))
    c["ref"] = grad_steps(c, F64)
    return c


def grad_steps(c, dtype, tables=(0, 1), scal=None, step=None):
    """The three steps of every active row in ``dtype``.  float32: a zero gradient row of a table
    sweep (a zero element of a dense gradient) takes zero_step_folded."""
    out = []
    for kd in c["kinds"]:
        r = {}
        for tb in (0, 1):
            if kd[f"p{tb}"] is None:
                continue
            p, m, v = (kd[f"{q}{tb}"].astype(dtype) for q in "pmv")
            a = kd["active"]
            for s in range(c["steps"] if tb in tables else 0):
                t = c["first"] + s
                sc = (scal or W.make_scalars)(c["lr"](t), c["hp"], t)
                g = kd["g"][s][tb][a].astype(dtype)
                x = (step or W.adamw_step)(p[a], m[a], v[a], g, None, None, None, dtype, s=sc)
                if dtype == F32 and c["family"] in ("table", "dense"):
                    y = W.zero_step_folded(p[a], m[a], v[a], sc, F32)
                    z = g == 0 if c["family"] == "dense" else np.broadcast_to(
                        ~np.isin(np.arange(kd["rows"]), kd["touched"])[:, None], g.shape)
                    x = tuple(np.where(z, yy, xx) for xx, yy in zip(x, y))
                p[a], m[a], v[a] = x
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = p, m, v
        out.append(r)
    return out


def measure_grad(c):
    f32 = grad_steps(c, F32)
    out = {}
    for k, kd in enumerate(c["kinds"]):
        for n, x in f32[k].items():
            a = kd["active"]
            out[n[0]] = max(out.get(n[0], 0.0), _err(x[a], c["ref"][k][n][a], n[0]))
    return out


def check_gradient_step(entry, impl, cases=None):
    """``impl(entry, case)`` -> per kind dict(p0, m0, v0[, p1, m1, v1], stamp[, clock]) after the
    three steps: every stepped row against float64, the others bit-unchanged, stamps and the
    closing form's clock exactly."""
    worst = {}
    for key in cases or grad_cases(entry):
        c = grad_case(*key)
        got = impl(entry, c)
        fp = GRAD_FP32[key]
        for k, kd in enumerate(c["kinds"]):
            tag, a = (entry, key, k), kd["active"]
            if kd["stamp"] is not None:
                after = kd["stamp"].copy()
                after[a] = c["first"] + c["steps"] - 1
                assert np.array_equal(got[k]["stamp"], after), (tag, "stamp")
            for n, ref in c["ref"][k].items():
                assert np.array_equal(got[k][n][~a].view(np.int32), kd[n][~a].view(np.int32)), \
                    (tag, n, "a row without a gradient changed")
                f = G._frac(_err(got[k][n][a], ref[a], n[0]), fp[n[0]])
                worst[n[0]] = max(worst.get(n[0], 0.0), f)
                assert f < 1.0, (tag, n, f)
        if entry == "flat_clock_close":
            t, reserved, seed = got[0]["clock"]
            assert (t, reserved) == (c["t_now"] + c["steps"], 0), (key, t, reserved)
            assert seed == G.A.splitmix_seed(G.SEED, t), (key, seed)
    return worst


# ----------------------------------------------------------------------------- the apply in the embedding backward
# ncf_embedding_bwd_reduce_apply_clock with the flag: tests/test_gpu_embed.py's "struct" id lists
# (singletons, a pair split by a piece cut, whole pieces, 10- and 18-piece segments), 1000 users and
# 700 items, three steps FIRST .. FIRST + 2 with the same ids and output gradients; every step's
# table gradients are the LayerNorm backward at that step's rows (tests/embed_ref.py: float64 the
# reference, float32 in the kernels' order the yardstick), stepped by AdamW at wd = 0.5.  m and v
# are compared relative to the float64 value or to a floor, whichever is larger (M_FLOOR = 1e-2,
# V_FLOOR = 3e-7: about a thirtieth of their typical size here, (1 - b1) |g| and (1 - b2) g^2 at
# |g| ~ 1): a gradient element that cancels to nearly zero carries its absolute rounding into m
# and v, and has no relative distance worth a bound.
BWD_DIMS = (16, 64, 256)
BWD_ROWS = (1000, 700)
M_FLOOR, V_FLOOR = 1e-2, 3e-7
KIND_TABLES = (("mfu", "mlpu"), ("mfi", "mlpi"))


@functools.lru_cache(maxsize=3)
def bwd_apply_case(D):
    e = E.bwd_case(D, "struct", *BWD_ROWS)
    g = np.random.default_rng(7000 + D)
    c = dict(e=e, D=D, hp=(B1, B2, EPS, WD), lr=lambda t: 1e-3, first=FIRST, steps=3,
             t_now=FIRST - 1, p={}, m={}, v={})
    for k in R.TABLES:
        p = e["rows"][k].numpy().astype(F32)
        c["p"][k] = p
        c["m"][k] = (1e-1 * g.normal(0.0, 1.0, p.shape)).astype(F32)
        c["v"][k] = g.uniform(1e-3, 1e-2, p.shape).astype(F32)
    c["ref"] = bwd_apply_steps(c, F64)
    return c


def bwd_apply_steps(c, dtype, step=None, scal=None):
    """{table: (p, m, v)} of the unique rows after the three steps in ``dtype``."""
    e = c["e"]
    st = {k: tuple(np.asarray(c[q][k], dtype=dtype) for q in "pmv") for k in R.TABLES}
    for s in range(c["steps"]):
        t = c["first"] + s
        rows = {k: st[k][0] for k in R.TABLES}
        bwd = R.embedding_bwd if dtype == F64 else R.embedding_bwd_f32
        grads = bwd(e["uid"], e["iid"], e["dys"], rows, e["gammas"], E.EPS, compact=True)["grads"]
        sc = (scal or W.make_scalars)(c["lr"](t), c["hp"], t)
        for k in R.TABLES:
            p, m, v = st[k]
            st[k] = (step or W.adamw_step)(p, m, v, grads[k].numpy(), None, None, None, dtype, s=sc)
    return st


def _err_floor(got, ref, q):
    d = np.abs(np.asarray(got, F64) - np.asarray(ref, F64))
    if q != "p":
        d = d / np.maximum(np.abs(ref), M_FLOOR if q == "m" else V_FLOOR)
    d = np.where(np.isfinite(d), d, np.inf)
    return float(d.max())


def measure_bwd_apply(c):
    f32 = bwd_apply_steps(c, F32)
    out = {}
    for k in R.TABLES:
        for q, x, r in zip("pmv", f32[k], c["ref"][k]):
            out[q] = max(out.get(q, 0.0), _err_floor(x, r, q))
    return out


def check_bwd_apply(D, impl):
    """``impl(case)`` -> dict(tables {table: (p, m, v) of the unique rows}, untouched: whether
    every other row kept its bits, stamps: per kind (of the unique rows, of the others)).  The
    stepped rows against float64; stamps = the last step on exactly the unique rows."""
    c = bwd_apply_case(D)
    got, fp, worst = impl(c), BWD_FP32[D], {}
    assert got["untouched"], (D, "a row outside the batch changed")
    last = c["first"] + c["steps"] - 1
    for k, (hit, rest) in enumerate(got["stamps"]):
        assert bool((hit == last).all()) and bool((rest == c["t_now"]).all()), (D, k, "stamp")
    for k in R.TABLES:
        for q, x, r in zip("pmv", got["tables"][k], c["ref"][k]):
            f = G._frac(_err_floor(x, r, q), fp[q])
            worst[q] = max(worst.get(q, 0.0), f)
            assert f < 1.0, (D, k, q, f)
    return worst


# ----------------------------------------------------------------------------- the schedule
SCHED_WIDTHS = G.SCHED_WIDTHS
SCHED_WD_AT = 18


def sched_hp(t):
    return (B1, B2, EPS, WD if t < SCHED_WD_AT else WD_LATE)


@functools.lru_cache(maxsize=2)
def sched_case(D):
    """tests/test_gpu_adam.py's schedule inputs (fresh tables, 40 steps of touched rows, a third of
    the rows never, the lr change at step 25) with a wd change at step 18."""
    c = dict(G.sched_case(D), hp=sched_hp)
    c["ref"] = sched_dense(c, F64)
    return c


def sched_dense(c, dtype):
    out = []
    for kd in c["kinds"]:
        r = {}
        for tb in (0, 1):
            tt = [(ids, Gr[tb]) for ids, Gr in kd["touched"]]
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = W.dense_schedule(
                kd[f"p{tb}"], kd[f"m{tb}"], kd[f"v{tb}"], tt, c["lr"], c["hp"], c["steps"], dtype)
        out.append(r)
    return out


def measure_sched(c):
    f32 = sched_dense(c, F32)
    out = {}
    for k in range(len(c["kinds"])):
        for n in NAMES:
            out[n[0]] = max(out.get(n[0], 0.0), _err(f32[k][n], c["ref"][k][n], n[0]))
    return out


def check_schedule(D, impl):
    """``impl(case)`` -> (per kind dict(p0 .. v1, stamp) after the closing sweep, per step and kind
    the oldest stamp after that step's rolling sweep).  Every row against the dense schedule in
    float64; after step s >= 8 no stamp is older than 8 steps."""
    c = sched_case(D)
    got, oldest = impl(c)
    fp, worst = SCHED_FP32[D], {}
    assert len(oldest) == c["steps"]
    for s, per_kind in enumerate(oldest, start=1):
        for k, o in enumerate(per_kind):
            assert o >= s - c["every"], (D, s, k, o)
    for k in range(len(c["kinds"])):
        assert bool((got[k]["stamp"] == c["steps"]).all()), (D, k)
        for n in NAMES:
            f = G._frac(_err(got[k][n], c["ref"][k][n], n[0]), fp[n[0]])
            worst[n[0]] = max(worst.get(n[0], 0.0), f)
            assert f < 1.0, (D, k, n, f)
    return worst


# ----------------------------------------------------------------------------- the fp32 figures
# The fp32 restatement's worst distance from float64 per case (p absolute, m and v relative), one
# host thread; the bound of a quantity is 4 x its figure.  tests/test_adamw_cpu.py re-measures
# each and holds it within [0.25 x, 1.001 x] of what it measures.
REPLAY_FP32 = {
    (16, 17, "base"): {"p": 2.3352e-07, "m": 4.5140e-07, "v": 4.4813e-07},
    (16, 330, "base"): {"p": 4.5773e-07, "m": 4.5467e-07, "v": 3.5762e-07},
    (16, 330, "wd0"): {"p": 9.1467e-08, "m": 4.5274e-07, "v": 3.4608e-07},
    (16, 330, "lr_change"): {"p": 4.3570e-07, "m": 4.2418e-07, "v": 3.1084e-07},
    (16, 330, "lr0"): {"p": 4.1032e-07, "m": 4.5274e-07, "v": 3.4608e-07},
    (16, 330, "wd_change"): {"p": 5.2346e-07, "m": 4.2418e-07, "v": 3.1084e-07},
    (32, 17, "base"): {"p": 2.3057e-07, "m": 4.0684e-07, "v": 3.6040e-07},
    (32, 330, "base"): {"p": 4.6755e-07, "m": 4.3072e-07, "v": 4.5475e-07},
    (32, 330, "wd0"): {"p": 9.2390e-08, "m": 4.3733e-07, "v": 3.5457e-07},
    (32, 330, "lr_change"): {"p": 4.7056e-07, "m": 4.1221e-07, "v": 3.3899e-07},
    (32, 330, "lr0"): {"p": 4.8417e-07, "m": 4.3733e-07, "v": 3.5457e-07},
    (32, 330, "wd_change"): {"p": 5.4519e-07, "m": 4.1221e-07, "v": 3.3899e-07},
    (64, 17, "base"): {"p": 2.3930e-07, "m": 4.4542e-07, "v": 3.9023e-07},
    (64, 330, "base"): {"p": 4.6193e-07, "m": 4.5903e-07, "v": 4.0359e-07},
    (64, 330, "wd0"): {"p": 8.3389e-08, "m": 4.6599e-07, "v": 3.9434e-07},
    (64, 330, "lr_change"): {"p": 4.7286e-07, "m": 4.6404e-07, "v": 4.4744e-07},
    (64, 330, "lr0"): {"p": 4.5865e-07, "m": 4.6599e-07, "v": 3.9434e-07},
    (64, 330, "wd_change"): {"p": 6.1077e-07, "m": 4.6404e-07, "v": 4.4744e-07},
    (128, 17, "base"): {"p": 2.4233e-07, "m": 4.5382e-07, "v": 4.3734e-07},
    (128, 330, "base"): {"p": 4.7848e-07, "m": 4.6851e-07, "v": 4.0096e-07},
    (128, 330, "wd0"): {"p": 8.5097e-08, "m": 4.8439e-07, "v": 4.3975e-07},
    (128, 330, "lr_change"): {"p": 4.5157e-07, "m": 4.8219e-07, "v": 4.0069e-07},
    (128, 330, "lr0"): {"p": 4.8992e-07, "m": 4.8439e-07, "v": 4.3975e-07},
    (128, 330, "wd_change"): {"p": 6.1515e-07, "m": 4.8219e-07, "v": 4.0069e-07},
    (256, 17, "base"): {"p": 2.4128e-07, "m": 5.2545e-07, "v": 4.6785e-07},
    (256, 330, "base"): {"p": 4.8466e-07, "m": 5.0202e-07, "v": 4.3005e-07},
    (256, 330, "wd0"): {"p": 9.0987e-08, "m": 5.1829e-07, "v": 4.3777e-07},
    (256, 330, "lr_change"): {"p": 4.8626e-07, "m": 5.0014e-07, "v": 4.7082e-07},
    (256, 330, "lr0"): {"p": 4.8258e-07, "m": 5.1829e-07, "v": 4.3777e-07},
    (256, 330, "wd_change"): {"p": 6.1329e-07, "m": 5.0014e-07, "v": 4.7082e-07},
}
GRAD_FP32 = {
    ('table', 16, 'null'): {"p": 7.0826e-08, "m": 2.1055e-07, "v": 1.5403e-07},
    ('table', 64, 'slot'): {"p": 7.2606e-08, "m": 2.0399e-07, "v": 2.6333e-07},
    ('table', 256, 'big'): {"p": 8.4541e-08, "m": 2.2122e-07, "v": 3.0605e-07},
    ('dense', 64, 'zeros'): {"p": 7.4689e-08, "m": 2.1760e-07, "v": 2.1741e-07},
    ('flat', 5, ''): {"p": 2.9281e-08, "m": 2.7259e-08, "v": 5.8400e-08},
    ('flat', 1027, ''): {"p": 6.2614e-08, "m": 1.4143e-07, "v": 2.0289e-07},
    ('flat', 1048835, ''): {"p": 8.3710e-08, "m": 2.0882e-07, "v": 2.9501e-07},
    ('flat', 4194311, ''): {"p": 8.3655e-08, "m": 2.0303e-07, "v": 3.2503e-07},
    ('apply', 16, ''): {"p": 7.0086e-08, "m": 1.3015e-07, "v": 2.2812e-07},
    ('apply', 32, ''): {"p": 7.0095e-08, "m": 1.4368e-07, "v": 2.3724e-07},
    ('apply', 64, ''): {"p": 7.1318e-08, "m": 1.4770e-07, "v": 2.5557e-07},
    ('apply', 128, ''): {"p": 7.8178e-08, "m": 1.5789e-07, "v": 2.5371e-07},
    ('apply', 256, ''): {"p": 7.7265e-08, "m": 1.6248e-07, "v": 2.7712e-07},
}
BWD_FP32 = {      # (m and v against max(|float64 value|, floor))
    16: {"p": 3.4079e-07, "m": 5.9877e-06, "v": 5.5847e-06},
    64: {"p": 4.6359e-07, "m": 1.3985e-05, "v": 8.7055e-06},
    256: {"p": 5.1245e-07, "m": 6.7622e-05, "v": 5.1396e-06},
}
SCHED_FP32 = {
    16: {"p": 2.8015e-07, "m": 9.1279e-07, "v": 6.6725e-07},
    64: {"p": 3.1854e-07, "m": 1.2486e-06, "v": 9.1118e-07},
    256: {"p": 3.2048e-07, "m": 1.0329e-06, "v": 7.3707e-07},
}


# ----------------------------------------------------------------------------- the kernels
def _flag(d, dtype=None):
    """NCF_ADAM_DECOUPLED on every pair of a tests/test_gpu_adam.py _Dev."""
    from ncf_amd import _lib
    for pr in d.pairs:
        pr.param_dtype = (_lib.DTYPE_F32 if dtype is None else dtype) | _lib.ADAM_DECOUPLED
    return d


def gpu_step_table(lr, hp, upto):
    """The decoupled step table as deferred._ensure fills it: one deferred.adamw_step_scalars call
    per run of equal (lr, wd), padded PAD steps past the highest step used."""
    from ncf_amd import _lib
    from ncf_amd.deferred import adamw_step_scalars
    S = _lib.ADAMW_TABLE_STRIDE
    host = np.zeros(S * (upto + PAD + 1), F32)
    for first, last, x, wd in segments(lr, hp, upto + PAD):
        adamw_step_scalars(x, B1, B2, EPS, wd, first, last - first + 1, host[S * first:])
    return torch.from_numpy(host).to(DEV)


def _one_reduction(keep):
    """A one-descriptor reduce list (5 rows of 64 ones -> 64 fives) and its scratch: the catch-up
    of ncf_reduce_batch_catchup then runs inside the fused launch."""
    from ncf_amd import _lib
    part, out = torch.ones(5, 64, device=DEV), torch.zeros(64, device=DEV)
    lst = _lib.ReduceList()
    d = lst.d[0]
    d.part, d.out, d.stride, d.ldo = part.data_ptr(), out.data_ptr(), 64, 64
    d.L, d.cols, d.P, d.accumulate, d.scale, d.reserved = 64, 64, 5, 0, 1.0, 0
    lst.count = 1
    scr = torch.zeros(max(_lib.query("ncf_reduce_batch_scratch", lst.address), 1), device=DEV)
    keep += [part, out, scr, lst]
    return lst, scr, out


def gpu_replay(entry, c):
    from ncf_amd import _lib
    name, arg = entry
    D, target = c["D"], c["target"]
    hp = (B1, B2, EPS, WD_ARG)
    d = _flag(G._Dev(c))
    tabt = gpu_step_table(c["lr"], c["hp"], target)
    tab = tabt.data_ptr()
    clk, cnt, st, rel = d.clock.data_ptr(), d.count.data_ptr(), d.st, c["rel"]
    if name == "pairs_catchup_clock":
        _lib.call("ncf_adam_pairs_catchup_clock", d.pa, 2, D, cnt, MAX_N, rel, clk, tab, *hp, st)
    elif name == "pairs_catchup_lock_clock":
        _lib.call("ncf_adam_pairs_catchup_lock_clock", d.pa, 2, D, cnt, MAX_N, rel, arg, clk, tab,
                  *hp, st)
    elif name == "reduce_batch_catchup":
        lst, scr, out = _one_reduction(d.keep)
        _lib.call("ncf_reduce_batch_catchup", lst.address, scr.data_ptr(), scr.numel(), d.pa, 2, D,
                  cnt, MAX_N, rel, clk, tab, *hp, st)
        torch.cuda.synchronize()
        assert float(out.sum()) == 5.0 * 64
    elif name == "pairs_catchup_claim_clock":
        raw = [torch.from_numpy(kd["raw"]).to(DEV) for kd in c["kinds"]]
        _lib.call("ncf_adam_pairs_catchup_claim_clock", d.pa, 2, D, raw[0].data_ptr(),
                  raw[1].data_ptr(), raw[0].numel(), rel, clk, tab, *hp, st)
    elif name == "pairs_sweep_rolling":
        _lib.call("ncf_adam_pairs_sweep_rolling", d.pa, 2, D, arg, rel, clk, tab, *hp, st)
    elif name == "pairs_sweep_rolling_part":
        for part in range(G.NPARTS):
            _lib.call("ncf_adam_pairs_sweep_rolling_part", d.pa, 2, D, arg, rel, part, G.NPARTS,
                      clk, tab, *hp, st)
    else:
        raise KeyError(name)
    out = d.result()
    assert d.clock_words() == (c["t_now"], 0, G.SEED)        # (the clock is read only)
    return out


def gpu_gradient(entry, c):
    from ncf_amd import _lib
    first, fam = c["first"], c["family"]
    wd = c["hp"][3]
    hp, hp_clock = (B1, B2, EPS, wd), (B1, B2, EPS, WD_ARG)
    d = _flag(G._Dev(c))
    tabt = gpu_step_table(c["lr"], lambda t: c["hp"], first + c["steps"])
    tab = tabt.data_ptr()
    clk, cnt, st = d.clock.data_ptr(), d.count.data_ptr(), d.st
    kd = c["kinds"][0]
    for s in range(c["steps"]):
        step = first + s
        if fam in ("table", "dense", "flat"):
            x = d.kinds[0]
            p, m, v = (x[n].data_ptr() for n in NAMES[:3])
            rows, D = kd["p0"].shape
            Gd = kd["g"][s][0]
            if entry == "table":
                slot = np.full(rows, -1, np.int32)
                slot[kd["touched"]] = np.arange(len(kd["touched"]), dtype=np.int32)
                sl, Gc = torch.from_numpy(slot).to(DEV), torch.from_numpy(Gd[kd["touched"]]).to(DEV)
                null = c["b"] == "null"
                _lib.call("ncf_adam_table", p, m, v, rows, D, None if null else sl.data_ptr(),
                          None if null else Gc.data_ptr(), 1e-3, *hp, -float(step), st)
                torch.cuda.synchronize()
                continue
            g = torch.from_numpy(Gd).to(DEV)
            d.keep.append(g)
            if entry == "table_dense_grad":
                _lib.call("ncf_adam_table_dense_grad", p, g.data_ptr(), m, v, rows * D, 1e-3, *hp,
                          -float(step), st)
            elif entry == "flat":
                _lib.call("ncf_adam_flat", p, g.data_ptr(), m, v, rows * D, 1e-3, *hp, -float(step), st)
            elif entry == "flat_clock":       # the clock stands at first - 1: step_rel = 1 + s
                _lib.call("ncf_adam_flat_clock", p, g.data_ptr(), m, v, rows * D, tab,
                          (1 + s) | _lib.ADAM_DECOUPLED, clk, *hp_clock, st)
            else:                               # the closing form advances the clock itself
                _lib.call("ncf_adam_flat_clock_close", p, g.data_ptr(), m, v, rows * D, tab,
                          1 | _lib.ADAM_DECOUPLED, clk, *hp_clock, G.SEED, st)
            continue
        for k, kk in enumerate(c["kinds"]):
            d.gradients(k, *kk["G"][s])
        assert entry == "pairs_apply_clock"
        _lib.call("ncf_adam_pairs_apply_clock", d.pa, 2, c["a"], cnt, MAX_N, 1 + s, clk, tab,
                  *hp_clock, st)
    out = d.result()
    if entry == "flat_clock_close":
        out[0]["clock"] = d.clock_words()
    else:
        assert d.clock_words() == (c["t_now"], 0, G.SEED)
    return out


def gpu_schedule(c, dense=False):
    """The calls of one deferred step as deferred.py issues them with the flag set: the catch-up of
    the step's rows to the clock's step, their apply (step clock->t + 1), the rolling sweep of that
    step's slice, the clock advance; the rolling sweep of period 1 to the last step at the end (as
    DeferredTableAdam.sync).  ``dense``: ncf_adam_table (negative step) over every table every step instead."""
    from ncf_amd import _lib
    D = c["D"]
    hp = (B1, B2, EPS, WD_ARG)
    kinds = [dict(kd, ids=np.zeros(MAX_N, np.int64), count=0) for kd in c["kinds"]]
    d = _flag(G._Dev(dict(t_now=0), kinds=kinds))
    tabt = gpu_step_table(c["lr"], c["hp"], c["steps"])
    tab = tabt.data_ptr()
    clk, cnt, st = d.clock.data_ptr(), d.count.data_ptr(), d.st
    oldest = []
    for s in range(c["steps"]):
        n = []
        for k, kd in enumerate(c["kinds"]):
            ids, Gr = kd["touched"][s]
            if dense:
                slot = np.full(kd["rows"], -1, np.int32)
                slot[ids] = np.arange(len(ids), dtype=np.int32)
                sl = torch.from_numpy(slot).to(DEV)
                for tb in (0, 1):
                    Gc = torch.from_numpy(np.ascontiguousarray(Gr[tb])).to(DEV) if len(ids) else None
                    x = d.kinds[k]
                    _lib.call("ncf_adam_table", x[f"p{tb}"].data_ptr(), x[f"m{tb}"].data_ptr(),
                              x[f"v{tb}"].data_ptr(), kd["rows"], D,
                              sl.data_ptr() if len(ids) else None,
                              Gc.data_ptr() if len(ids) else None, c["lr"](s + 1),
                              *c["hp"](s + 1), -float(s + 1), st)
                    torch.cuda.synchronize()
                continue
            buf = np.resize(np.arange(kd["rows"]), MAX_N).astype(np.int64)     # valid past the count
            buf[:len(ids)] = ids
            d.kinds[k]["ids"].copy_(torch.from_numpy(buf))
            Gc = [np.zeros((MAX_N, D), F32) for _ in (0, 1)]
            for tb in (0, 1):
                Gc[tb][:len(ids)] = Gr[tb]
            d.gradients(k, *Gc)
            n.append(len(ids))
        if dense:
            continue
        d.count.copy_(torch.tensor(n + [0], dtype=torch.int32))
        _lib.call("ncf_adam_pairs_catchup_clock", d.pa, 2, D, cnt, MAX_N, 0, clk, tab, *hp, st)
        _lib.call("ncf_adam_pairs_apply_clock", d.pa, 2, D, cnt, MAX_N, 1, clk, tab, *hp, st)
        _lib.call("ncf_adam_pairs_sweep_rolling", d.pa, 2, D, c["every"], 1, clk, tab, *hp, st)
        _lib.call("ncf_step_clock_advance", clk, G.SEED, st)
        torch.cuda.synchronize()
        oldest.append([int(x["stamp"].min()) for x in d.kinds])
    if dense:
        return d.result(), None
    _lib.call("ncf_adam_pairs_sweep_rolling", d.pa, 2, D, 1, 0, clk, tab, *hp, st)
    assert d.clock_words()[0] == c["steps"]
    return d.result(), oldest


def gpu_bwd_apply(c, fused=True):
    """Per step: ncf_dedup_ids, then ncf_embedding_bwd_reduce_apply_clock with the flagged pairs
    (``fused``), or ncf_embedding_bwd_reduce and ncf_adam_pairs_apply_clock over its unique rows
    and compact gradients (the two calls the header says it equals)."""
    from ncf_amd import _lib
    e, D = c["e"], c["D"]
    n, (NU, NI) = e["n"], BWD_ROWS
    st = _lib.stream_ptr(DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    uid, iid = E._dev(e["uid"]), E._dev(e["iid"])
    dys = [E._dev(e["dys"][k]) for k in R.TABLES]
    gm, gl = E._dev(e["gammas"][0]), E._dev(e["gammas"][1])
    tab, before = {}, {}
    for k in R.TABLES:
        rows, uq = (NU if k[-1] == "u" else NI), E._dev(e["uniq_" + k[-1]])
        full = []
        for q, fill in (("p", float("nan")), ("m", 0.25), ("v", 0.5)):
            t = torch.full((rows, D), fill, device=DEV)
            t[uq] = torch.from_numpy(c[q][k]).to(DEV)
            full.append(t)
        tab[k] = full
        before[k] = [t.clone() for t in full]
    stamps = [torch.full((r,), c["t_now"], dtype=torch.int32, device=DEV) for r in BWD_ROWS]
    pairs = (_lib.TablePair * 2)()
    for k, (a, b) in enumerate(KIND_TABLES):
        pr = pairs[k]
        pr.p0, pr.m0, pr.v0 = (P(t) for t in tab[a])
        pr.p1, pr.m1, pr.v1 = (P(t) for t in tab[b])
        pr.stamp, pr.rows = P(stamps[k]), BWD_ROWS[k]
        pr.param_dtype = _lib.DTYPE_F32 | _lib.ADAM_DECOUPLED
    pa = __import__("ctypes").addressof(pairs)
    tabt = gpu_step_table(c["lr"], lambda t: c["hp"], c["first"] + c["steps"])
    clock = torch.tensor([c["t_now"], G.SEED], dtype=torch.int64, device=DEV)
    ws = torch.zeros(_lib.query("ncf_embedding_bwd_workspace", n, D), dtype=torch.uint8, device=DEV)
    uq = [torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
    nu = torch.zeros(2, dtype=torch.int32, device=DEV)
    Gc = [E._nan(n, D) for _ in range(4)]
    pg = [E._nan(D) for _ in range(4)]
    hp = (B1, B2, EPS, WD_ARG)
    for s in range(c["steps"]):
        _lib.call("ncf_dedup_ids", P(uid), P(iid), n, D, NU, NI, P(uq[0]), P(uq[1]), None, None,
                  P(nu), P(ws), ws.numel(), st)
        if fused:
            _lib.call("ncf_embedding_bwd_reduce_apply_clock", n, D, NU, NI, *[P(x) for x in dys],
                      P(gm), P(gl), E.EPS, *[P(x) for x in Gc], P(uq[0]), P(uq[1]),
                      *[P(x) for x in pg], P(ws), ws.numel(), None, pa, 1 + s, P(clock), P(tabt),
                      *hp, st)
        else:
            _lib.call("ncf_embedding_bwd_reduce", n, D, NU, NI, *[P(x) for x in dys],
                      *[P(tab[k][0]) for k in R.TABLES], P(gm), P(gl), E.EPS, *[P(x) for x in Gc],
                      P(uq[0]), P(uq[1]), *[P(x) for x in pg], P(ws), ws.numel(), None, st)
            for k in range(2):
                pairs[k].row_ids = P(uq[k])
                pairs[k].g0, pairs[k].g1 = P(Gc[2 * k]), P(Gc[2 * k + 1])
            _lib.call("ncf_adam_pairs_apply_clock", pa, 2, D, P(nu), n, 1 + s, P(clock), P(tabt),
                      *hp, st)
        torch.cuda.synchronize()
    assert int(clock[0]) == c["t_now"]
    out = dict(tables={}, untouched=True, stamps=[], full={k: [t.cpu() for t in tab[k]] for k in tab})
    for k in R.TABLES:
        ids = e["uniq_" + k[-1]]
        out["tables"][k] = tuple(t[ids].numpy() for t in out["full"][k])
        rest = torch.ones(out["full"][k][0].shape[0], dtype=torch.bool)
        rest[ids] = False
        for t, b in zip(out["full"][k], before[k]):
            same = t[rest].view(torch.int32) == b.cpu()[rest].view(torch.int32)
            out["untouched"] = out["untouched"] and bool(same.all())
    for k, kind in enumerate("ui"):
        ids, sp = e["uniq_" + kind], stamps[k].cpu()
        rest = torch.ones(sp.numel(), dtype=torch.bool)
        rest[ids] = False
        out["stamps"].append((sp[ids].numpy(), sp[rest].numpy()))
    assert all(bool(torch.isfinite(x[:int(nu[j // 2])]).all()) for j, x in enumerate(Gc))
    return out


def _line(what, worst):
    print(f"{what}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()) + " of the bound")


@pytest.mark.parametrize("name", sorted({e[0] for e in REPLAY_ENTRIES}))
@pytest.mark.parametrize("D", WIDTHS)
def test_replay_vs_float64(D, name):
    for entry in REPLAY_ENTRIES:
        if entry[0] == name:
            _line(f"adamw replay {entry} D {D}", check_replay(D, entry, gpu_replay))


@pytest.mark.parametrize("entry", GRAD_ENTRIES)
def test_gradient_step_vs_float64(entry):
    _line(f"adamw gradient step {entry}", check_gradient_step(entry, gpu_gradient))


@pytest.mark.parametrize("D", BWD_DIMS)
def test_embedding_bwd_reduce_apply_clock_vs_float64(D):
    _line(f"adamw embedding backward + apply D {D}", check_bwd_apply(D, gpu_bwd_apply))
    a = gpu_bwd_apply(bwd_apply_case(D))["full"]
    b = gpu_bwd_apply(bwd_apply_case(D), fused=False)["full"]
    for k in R.TABLES:              # the reduce followed by the flagged apply: the same bits
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (D, k)


def test_fixed_step_forms_take_the_clock_forms_bits():
    """The decoupled forms (a negative step; NCF_ADAM_DECOUPLED in step_rel): ncf_adam_flat ==
    ncf_adam_flat_clock == ncf_adam_flat_clock_close, and ncf_adam_table_dense_grad ==
    ncf_adam_table on a gradient without exact zeros, bit for bit."""
    c = grad_case("flat", 1027, "")
    a, b, e = (gpu_gradient(x, c)[0] for x in ("flat", "flat_clock", "flat_clock_close"))
    for n in NAMES[:3]:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n
        assert np.array_equal(a[n].view(np.int32), e[n].view(np.int32)), n
    c = grad_case("table", 64, "slot")
    a, b = gpu_gradient("table", c)[0], gpu_gradient("table_dense_grad", dict(c, family="dense"))[0]
    for n in NAMES[:3]:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n


@pytest.mark.parametrize("D", SCHED_WIDTHS)
def test_schedule_vs_dense_float64(D):
    _line(f"adamw schedule D {D}", check_schedule(D, gpu_schedule))
    got, _ = gpu_schedule(sched_case(D))
    dense, _ = gpu_schedule(sched_case(D), dense=True)
    for k in range(len(got)):       # the deferred schedule is the dense one, bit for bit
        for n in NAMES:
            assert np.array_equal(got[k][n].view(np.int32), dense[k][n].view(np.int32)), (D, k, n)


def test_refusals():
    """NCF_ERR_ARG: the flag on bf16 rows, on the owner-side gsum apply, and on one pair only."""
    from ncf_amd import _lib
    c = replay_case(16, 17, "base")
    hp = (B1, B2, EPS, WD_ARG)
    tabt = gpu_step_table(c["lr"], c["hp"], 17)
    tab = tabt.data_ptr()

    def calls(d):
        clk, cnt, st = d.clock.data_ptr(), d.count.data_ptr(), d.st
        raw = torch.zeros(4, dtype=torch.int64, device=DEV)
        lst, scr, _ = _one_reduction(d.keep)
        d.keep.append(raw)
        return [
            ("ncf_adam_pairs_catchup_clock", (d.pa, 2, 16, cnt, MAX_N, 1, clk, tab, *hp, st)),
            ("ncf_adam_pairs_catchup_lock_clock", (d.pa, 2, 16, cnt, MAX_N, 1, 0, clk, tab, *hp, st)),
            ("ncf_adam_pairs_catchup_claim_clock", (d.pa, 2, 16, raw.data_ptr(), raw.data_ptr(), 4,
                                                    1, clk, tab, *hp, st)),
            ("ncf_adam_pairs_apply_clock", (d.pa, 2, 16, cnt, MAX_N, 1, clk, tab, *hp, st)),
            ("ncf_adam_pairs_sweep_rolling", (d.pa, 2, 16, 8, 1, clk, tab, *hp, st)),
            ("ncf_adam_pairs_sweep_rolling_part", (d.pa, 2, 16, 8, 1, 0, 2, clk, tab, *hp, st)),
            ("ncf_reduce_batch_catchup", (lst.address, scr.data_ptr(), scr.numel(), d.pa, 2, 16, cnt,
                                          MAX_N, 1, clk, tab, *hp, st)),
            # (refused on the pairs alone, before any other argument is read)
            ("ncf_embedding_bwd_reduce_apply_clock", (4, 16, ROWS[0], ROWS[1]) + (None,) * 6 +
             (1e-5,) + (None,) * 10 + (None, 0, None, d.pa, 1, clk, tab, *hp, st)),
        ]

    def refused(name, args):
        with pytest.raises(_lib.NCFArgumentError):       # (NCF_ERR_ARG)
            _lib.call(name, *args)

    for dtype in (_lib.DTYPE_BF16, _lib.DTYPE_BF16_SR):
        d = _flag(G._Dev(c), dtype)
        for name, args in calls(d):
            refused(name, args)
    d = _flag(G._Dev(c))
    d.pairs[1].param_dtype = _lib.DTYPE_F32            # the pairs disagree on the flag
    for name, args in calls(d):
        refused(name, args)
    d = _flag(G._Dev(c))
    got = torch.zeros(4, 32, device=DEV)
    pos = torch.full((MAX_N, 1), -1, dtype=torch.int32, device=DEV)
    refused("ncf_adam_pairs_apply_gsum_clock",
            (d.pa, 2, 16, d.count.data_ptr(), MAX_N, 1, got.data_ptr(), pos.data_ptr(),
             pos.data_ptr(), 1, d.clock.data_ptr(), tab, *hp, d.st))
    torch.cuda.synchronize()
    for k, kd in enumerate(c["kinds"]):                # nothing was launched
        for n in NAMES:
            assert np.array_equal(d.result()[k][n].view(np.int32), kd[n].view(np.int32))
