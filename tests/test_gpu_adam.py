"""The fp32 table and flat Adam entry points of csrc/adam.hip (and the catch-up inside
ncf_reduce_batch_catchup), one at a time, against float64 (tests/adam_ref.py), on the MI355X:
every replaying entry point at every width NCF_DISPATCH_DIM accepts with the gaps that straddle
replay_uniform's 8-step chunks, every gradient-step entry point over three steps, and 40 steps of
the deferred schedule's own call sequence against the dense schedule.

Each check takes the implementation under test as an argument: here it is the kernel;
tests/test_adam_cpu.py runs the same check, on the same inputs, with the fp32 restatement (which
must pass with a quarter of every bound used) and with mutants (which must fail).

Bounds, none fitted to the GPU's output: for each quantity of each case 4 x the worst distance of
the fp32 restatement (one host thread, numpy: every operation rounded once) from float64 on
that case's own inputs; p absolute, m and v relative to the float64 value.  The measured figures
stand in REPLAY_FP32 / GRAD_FP32 / SCHED_FP32 below; tests/test_adam_cpu.py re-measures them.

Inputs: |p| in [0.2, 0.5], random sign; two moment populations in every case, "untouched
history" (m = wd p u, u in [0.5, 1.5]; v = (wd p)^2 u', u' in [1.6, 3]: each step changes v by
more than 3e-4 of it) and "touched history" (v ~ U(1e-5, 1e-3), |m| ~ |N(0, 1e-2)|).  m and the
gradients carry p's sign, as the weight decay's term does: an m that passes through zero has no
relative distance worth a bound.  In the replay cases the touched-history rows are the odd rows
at most 9 steps behind, with |m| = 2e-2 + |N(0, 1e-2)|, for the sensitivity condition
(replay_sensitivity): one missing or extra owed step must move every replayed element by at least
20 x the p bound, which a touched-history row 130 steps behind (m decayed to wd p under a v that
has hardly decayed) cannot give.  With wd = 0 no input can give it (m decays by 0.9 per step:
the 130th owed step moves p by less than an ulp); there the condition is held on m, which every
owed step changes by a tenth of it.

On the MI355X the kernels used at most 0.28 of a bound in the replays (p 0.271, m 0.279, v 0.25),
0.30 in the table and row steps, 0.83 in the flat steps (v; p and m 0.25), 0.26 in the schedule.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import adam_ref as A

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")

F32, F64, LOCK = A.F32, A.F64, A.LOCK
WIDTHS = (16, 32, 64, 128, 256)
ROWS = (203, 5)             # two kinds; 203: no multiple of the 4, 8 or 16 rows of a block
MAX_N, COUNT = 128, (97, 3)
# neighbours in the list (one wave at D < 64) always differ
GAPS = (0, 130, 1, 65, 2, 64, 7, 63, 8, 25, 9, 24, 15, 23, 16, 17)
PAD = 4096                  # steps the step table holds past the target (deferred.SCALAR_PAD)
REPLAY_CASES = ((17, "base"), (17, "wd0"), (330, "base"), (330, "wd0"), (330, "lr_change"),
                (330, "lr0"))
NAMES = ("p0", "m0", "v0", "p1", "m1", "v1")


def hp_of(variant):
    return A.HP[:3] + (0.0,) if variant == "wd0" else A.HP


def lr_of(target, variant):
    """lr of step t.  lr_change: 1e-3 up to step target - 40, 3e-4 after; lr0: 20 steps of
    lr = 0, target - 60 .. target - 41."""
    if variant == "lr_change":
        return lambda t: 1e-3 if t <= target - 40 else 3e-4
    if variant == "lr0":
        return lambda t: 0.0 if target - 60 <= t <= target - 41 else 1e-3
    return lambda t: 1e-3


def lr_segments(lr, upto):
    """[(first, last, lr)]: the calls of ncf_adam_step_scalars that fill steps 1 .. upto, one per
    run of equal lr (deferred._ensure refills from the step an lr change takes effect)."""
    seg, first = [], 1
    for t in range(2, upto + 2):
        if t == upto + 1 or lr(t) != lr(first):
            seg.append((first, t - 1, lr(first)))
            first = t
    return seg


# ----------------------------------------------------------------------------- inputs
def _tables(g, rows, D, touched_rows):
    """Both tables of a kind: |p| in [0.2, 0.5], random sign; rows in ``touched_rows`` (bool) hold
    the touched-history moments, the others the untouched-history ones."""
    out = {}
    for tb in (0, 1):
        sign = np.where(g.random((rows, D)) < 0.5, -1.0, 1.0)
        p = sign * g.uniform(0.2, 0.5, (rows, D))
        wdp = 1e-5 * p
        m = wdp * g.uniform(0.5, 1.5, (rows, D))
        v = wdp * wdp * g.uniform(1.6, 3.0, (rows, D))
        mt = sign * (2e-2 + np.abs(g.normal(0.0, 1e-2, (rows, D))))
        vt = g.uniform(1e-5, 1e-3, (rows, D))
        t = touched_rows[:, None]
        out[f"p{tb}"] = p.astype(F32)
        out[f"m{tb}"] = np.where(t, mt, m).astype(F32)
        out[f"v{tb}"] = np.where(t, vt, v).astype(F32)
    return out


@functools.lru_cache(maxsize=8)
def replay_case(D, target, variant):
    """Two kinds (203 and 5 rows) of table pairs behind ``target`` by the gaps of GAPS, 97 / 3 of
    their rows listed in id buffers of 128 (the entries past the count name valid rows, behind
    too), some listed rows locked, some ahead; raw id lists for the claim form; the float64
    replay of every row that is behind and not locked."""
    g = np.random.default_rng(1000 * D + target + 7 * len(variant))
    hp, lr = hp_of(variant), lr_of(target, variant)
    kinds = []
    for k, rows in enumerate(ROWS):
        perm = g.permutation(rows)
        ids = np.concatenate([perm[:COUNT[k]], np.resize(perm[COUNT[k]:], MAX_N - COUNT[k])])
        gap = np.array([GAPS[(5 * r + 3) % 16] for r in range(rows)])
        gap[ids[:COUNT[k]]] = [GAPS[c % 16] for c in range(COUNT[k])]
        gap = np.minimum(gap, target)
        stamp = (target - gap).astype(np.int32)
        t = _tables(g, rows, D, (gap <= 9) & (np.arange(rows) % 2 == 1))
        listed = ids[:COUNT[k]]
        locked = [listed[c] for c in (5, 37, 70) if c < COUNT[k]] + [perm[-1]]
        ahead = [listed[c] for c in (11, 50) if c < COUNT[k]]
        if k == 1:
            locked, ahead = [perm[-1]], [listed[2]]
        stamp[locked] |= LOCK
        stamp[ahead] = target + 1
        # raw ids: every listed row 1-6 times, duplicates adjacent and far apart, ids out of range
        raw = np.concatenate([np.repeat(listed, 1 + np.arange(COUNT[k]) % 3), listed[::2],
                              listed[::3], listed[::-5], [-1, rows, -7, rows + 100, 2 ** 40]])
        kinds.append(dict(t, stamp=stamp, ids=ids.astype(np.int64), count=COUNT[k], rows=rows,
                          raw=raw.astype(np.int64)))
    n = max(len(kd["raw"]) for kd in kinds)
    for kd in kinds:            # one occurrence count for both kinds: padded out of range
        kd["raw"] = np.concatenate([kd["raw"], np.full(n - len(kd["raw"]), -1, np.int64)])
    c = dict(D=D, target=target, variant=variant, hp=hp, lr=lr, kinds=kinds, t_now=target - 1, rel=1)
    c["ref"] = _replay_all(c, target, F64)
    return c


def _replay_all(c, target, dtype, **kw):
    """Every row behind ``target`` and not locked, replayed to it, in ``dtype``."""
    out = []
    for kd in c["kinds"]:
        r = {}
        for tb in (0, 1):
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = A.replay(
                kd[f"p{tb}"], kd[f"m{tb}"], kd[f"v{tb}"], kd["stamp"], target, c["lr"], c["hp"], dtype,
                **kw)
        out.append(r)
    return out


def behind(kd, target):
    return kd["stamp"].astype(np.int64) < target       # (locked stamps compare above any target)


def _err(got, ref, q):
    """Worst |got - ref|: absolute for p, relative to the float64 value for m and v."""
    if got.size == 0:
        return 0.0
    d = np.abs(got.astype(F64) - ref)
    if q != "p":
        d = d / np.abs(ref)
    d = np.where(np.isfinite(d), d, np.inf)
    return float(d.max())


def _frac(err, figure):
    """``err`` as a fraction of its bound, 4 x the fp32 restatement's figure."""
    return err / (4 * figure) if figure > 0 else (0.0 if err == 0 else float("inf"))


def measure_replay(c):
    """{p, m, v}: the fp32 restatement's worst distance from float64 over the case."""
    f32 = _replay_all(c, c["target"], F32)
    out = {}
    for k, kd in enumerate(c["kinds"]):
        b = behind(kd, c["target"])
        for n in NAMES:
            out[n[0]] = max(out.get(n[0], 0.0), _err(f32[k][n][b], c["ref"][k][n][b], n[0]))
    return out


def replay_sensitivity(c):
    """{p, m, v}: the smallest change the last owed step makes to any replayed element, from the
    float64 reference: min |x(target) - x(target - 1)|, relative for m and v."""
    prev = _replay_all(c, c["target"] - 1, F64)
    out = {}
    for k, kd in enumerate(c["kinds"]):
        b = behind(kd, c["target"])
        for n in NAMES:
            d = np.abs(c["ref"][k][n][b] - prev[k][n][b])
            if n[0] != "p":
                d = d / np.abs(c["ref"][k][n][b])
            out[n[0]] = min(out.get(n[0], np.inf), float(d.min()))
    return out


# ----------------------------------------------------------------------------- replay: who, where
REPLAY_ENTRIES = (
    [("rows_catchup", True), ("rows_catchup", False), ("rows_catchup_clock", True),
     ("rows_catchup_clock", False), ("pairs_catchup_clock", None), ("pairs_catchup_lock_clock", 0),
     ("pairs_catchup_lock_clock", 1), ("pairs_catchup_claim_clock", None), ("sweep", None),
     ("reduce_batch_catchup", None)] +
    # every = 3: 203 rows in slices of 68, the last one short; 64: the 5-row table's slice of
    # the target lies past its end
    [(n, e) for n in ("sweep_rolling", "pairs_sweep_rolling", "pairs_sweep_rolling_part")
     for e in (8, 3, 64)])
SWEEP_RANGE = ((7, 150), (1, 3))        # ncf_adam_sweep: row0 > 0, ending before the table's end
NPARTS = 3


def slice_rows(total, every, target, part=0, nparts=1):
    """k_pairs_sweep's rows of the slice of step ``target``: (row0, rows)."""
    sl = (total + every - 1) // every
    s0 = (target % every) * sl
    srows = max(0, min(sl, total - s0))
    row0 = s0 + srows * part // nparts
    return row0, s0 + srows * (part + 1) // nparts - row0


def plan(entry, c, all_ids=False, locked_too=False, drop_last=False):
    """Per kind: (rows the entry point replays [bool], the stamps after it, the tables it steps).
    The keyword arguments are mutants (tests/test_adam_cpu.py)."""
    name, arg = entry
    target, out = c["target"], []
    for k, kd in enumerate(c["kinds"]):
        rows, stamp = kd["rows"], kd["stamp"]
        sel = np.zeros(rows, bool)
        if name.startswith(("rows_catchup", "pairs_catchup_clock", "pairs_catchup_lock",
                            "reduce_batch")):
            sel[kd["ids"][:MAX_N if all_ids else kd["count"]]] = True
        elif name == "pairs_catchup_claim_clock":
            raw = kd["raw"]
            sel[raw[(raw >= 0) & (raw < rows)]] = True
        elif name == "sweep":
            r0, n = SWEEP_RANGE[k]
            sel[r0:r0 + n - drop_last] = True
        else:
            r0, n = slice_rows(rows, arg, target)
            sel[r0:r0 + max(0, n - drop_last)] = True
        eff = stamp & ~LOCK if locked_too else stamp
        rep = sel & (eff.astype(np.int64) < target)
        after = stamp.copy()
        lock1 = name == "pairs_catchup_lock_clock" and arg == 1
        after[rep] = target | LOCK if lock1 else target
        if lock1:
            after[sel & (stamp == target)] = target | LOCK
        tabs = (0,) if name.startswith("rows_catchup") and not arg else (0, 1)
        out.append((rep, after, tabs))
    return out


def check_replay(D, entry, impl, cases=REPLAY_CASES):
    """``impl(entry, case)`` -> per kind dict(p0, m0, v0, p1, m1, v1, stamp) after the call.
    p, m, v of the replayed rows against float64; stamps exactly; every row the entry point must
    skip (unlisted, past the count, locked, ahead, outside the range or slice) bit-unchanged.
    Returns the worst fraction of its bound per quantity."""
    worst = {}
    for target, variant in cases:
        c = replay_case(D, target, variant)
        got = impl(entry, c)
        fp = REPLAY_FP32[(D, target, variant)]
        for k, (kd, (rep, after, tabs)) in enumerate(zip(c["kinds"], plan(entry, c))):
            tag = (entry, D, target, variant, k)
            assert np.array_equal(got[k]["stamp"], after), (tag, "stamp")
            for n in NAMES:
                r = rep if int(n[1]) in tabs else np.zeros_like(rep)
                assert np.array_equal(got[k][n][~r].view(np.int32), kd[n][~r].view(np.int32)), \
                    (tag, n, "a skipped row changed")
                f = _frac(_err(got[k][n][r], c["ref"][k][n][r], n[0]), fp[n[0]])
                worst[n[0]] = max(worst.get(n[0], 0.0), f)
                assert f < 1.0, (tag, n, f)
    return worst


# ----------------------------------------------------------------------------- gradient steps
FIRST = 15                  # steps 15, 16, 17: steep bias corrections
FLAT_N = (1, 3, 4, 5, 1023, 1027)
FLAT_BIG = {"flat": (1 << 20) + 259, "flat_clock": (1 << 20) + 259,
            "flat_clock_close": 4 * (1 << 20) + 7}       # past the grid cap of each kernel
SEED = 0x1234567
GRAD_ENTRIES = ("table", "table_dense_grad", "flat", "flat_clock", "flat_clock_close",
                "rows_apply", "rows_apply_clock", "pairs_apply_clock", "pairs_apply_p1_null",
                "pairs_apply_gsum_clock")


def grad_cases(entry):
    """The case keys of an entry point (grad_case's arguments after the family)."""
    if entry == "table":
        return [("table", D, m) for D in WIDTHS for m in ("slot", "null")] + [("table", 256, "big")]
    if entry == "table_dense_grad":
        return [("dense", 64, "zeros")]
    if entry.startswith("flat"):
        return [("flat", n, "") for n in FLAT_N + (FLAT_BIG[entry],)]
    if entry == "pairs_apply_gsum_clock":
        return [("gsum", D, W) for D in WIDTHS for W in (1, 3)]
    return [("apply", D, "") for D in WIDTHS]


def _moments(g, shape, p):
    """Non-zero moments, the two populations interleaved by row.  m and the gradients (_grad)
    carry p's sign, as the weight decay's term does: no m passes through zero, where its relative
    distance from float64 would measure the cancellation and not the arithmetic."""
    rows = shape[0]
    t = (np.arange(rows) % 2 == 1)[:, None]
    wdp = 1e-5 * p
    m = np.where(t, np.sign(p) * np.abs(g.normal(0.0, 1e-2, shape)), wdp * g.uniform(0.5, 1.5, shape))
    v = np.where(t, g.uniform(1e-5, 1e-3, shape), wdp * wdp * g.uniform(1.6, 3.0, shape))
    return m.astype(F32), v.astype(F32)


def _params(g, shape, by_column=False):
    """|p| in [0.2, 0.5], the sign random per element (``by_column``: per column)."""
    sign = np.where(g.random(shape[-1] if by_column else shape) < 0.5, -1.0, 1.0)
    return (sign * g.uniform(0.2, 0.5, shape)).astype(F32)


def _grad(g, p, scale=1e-2):
    return (np.sign(p) * np.abs(g.normal(0.0, scale, p.shape))).astype(F32)


@functools.lru_cache(maxsize=4)
def grad_case(family, a, b):
    """kinds: per kind the tables (p1 None: one table), ``active`` (the rows that step) and per
    step the dense gradient of every table (zero rows where no gradient reaches); the float64
    result of the three steps FIRST .. FIRST + 2."""
    g = np.random.default_rng(len(family) * 7919 + a * 31 + (b if isinstance(b, int) else len(b)))
    c = dict(family=family, a=a, b=b, hp=A.HP, lr=lambda t: 1e-3, first=FIRST, steps=3, t_now=FIRST - 1)
    kinds = []
    if family in ("table", "dense", "flat"):
        rows, D = {"table": (16400 if b == "big" else 203, a), "dense": (203, a), "flat": (a, 1)}[family]
        p = _params(g, (rows, D))
        m, v = _moments(g, (rows, D), p)
        touched = g.random(rows) < 0.4 if family != "flat" and b != "null" else \
            np.full(rows, family == "flat")
        ids = np.nonzero(touched)[0]
        gs = []
        for _ in range(3):
            G = np.zeros((rows, D), F32)
            G[ids] = _grad(g, p[ids])
            if family == "dense" and len(ids):     # single exact zeros in touched rows
                G[ids[0], 3], G[ids[-1], 0], G[ids[1], D - 1] = 0.0, -0.0, 0.0
            gs.append([G])
        kinds.append(dict(p0=p, m0=m, v0=v, p1=None, rows=rows, active=np.ones(rows, bool),
                          touched=ids, g=gs, stamp=None))
    else:
        D = a
        for k, rows in enumerate(ROWS):
            t = {}
            for tb in (0, 1):
                t[f"p{tb}"] = _params(g, (rows, D), by_column=family == "gsum")
                t[f"m{tb}"], t[f"v{tb}"] = _moments(g, (rows, D), t[f"p{tb}"])
            perm = g.permutation(rows)
            count = (COUNT[0], 0)[k]            # the second kind: count = 0
            ids = np.resize(perm, MAX_N).astype(np.int64)
            active = np.zeros(rows, bool)
            active[ids[:count]] = True
            kd = dict(t, rows=rows, ids=ids, count=count, active=active,
                      stamp=np.full(rows, FIRST - 1, np.int32), g=[], G=[], got=[], pos=[])
            for s in range(3):
                if family == "gsum":
                    W, J = b, 150
                    # [mf | mlp] halves of 2 D floats, magnitudes 1e-6 .. 1
                    sign = np.sign(np.concatenate([t["p0"][0], t["p1"][0]]))
                    got = (sign * np.abs(g.normal(0.0, 1.0, (J, 2 * D))) *
                           10.0 ** g.uniform(-6, 0, (J, 1))).astype(F32)
                    pos = g.integers(0, J, (MAX_N, W)).astype(np.int32)
                    pos[g.random((MAX_N, W)) < 0.3] = -1
                    pos[1] = -1                 # a listed row no rank touched
                    G64 = np.zeros((MAX_N, 2 * D), F64)
                    G32 = np.zeros((MAX_N, 2 * D), F32)
                    for r in range(W):          # the rank-order sum (0 + x == x exactly)
                        x = np.where(pos[:, r:r + 1] >= 0, got[np.maximum(pos[:, r], 0)], F32(0))
                        G64 += x
                        G32 = G32 + x
                    kd["got"].append(got)
                    kd["pos"].append(pos)
                    Gc64, Gc = (G64[:, :D], G64[:, D:]), (G32[:, :D].copy(), G32[:, D:].copy())
                else:
                    Gc = tuple(_grad(g, t[f"p{tb}"][ids]) for tb in (0, 1))
                    Gc64 = Gc
                dense = []
                for tb in (0, 1):
                    x = np.zeros((rows, D), F64)
                    x[ids[:count]] = Gc64[tb][:count]
                    dense.append(x)
                kd["g"].append(dense)
                kd["G"].append(Gc)              # compact fp32 gradients [MAX_N, D] per table
            kinds.append(kd)
    c["kinds"] = kinds
    c["ref"] = grad_steps(c, F64)
    return c


def grad_steps(c, dtype, tables=(0, 1), zero_form=True, scal=None):
    """The three steps of every active row in ``dtype``.  float32: a zero gradient row of a table
    sweep takes zero_step_folded, as k_adam_table / k_adam_table_dense_grad step it."""
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
                sc = (scal or A.make_scalars)(c["lr"](t), c["hp"], t)
                g = kd["g"][s][tb][a].astype(dtype)
                if dtype == F32 and c["family"] == "gsum":      # the sum taken in fp32, rank order
                    g = np.zeros(kd[f"p{tb}"].shape, F32)
                    g[kd["ids"][:kd["count"]]] = kd["G"][s][tb][:kd["count"]]
                    g = g[a]
                x = A.adam_step(p[a], m[a], v[a], g, None, None, None, dtype, s=sc)
                if dtype == F32 and zero_form and c["family"] in ("table", "dense"):
                    y = A.zero_step_folded(p[a], m[a], v[a], sc, F32)
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
    three steps.  p, m and v of every stepped row against float64, the rows no gradient reaches
    bit-unchanged, stamps exactly (the apply forms: the step), the clock of the closing form."""
    worst = {}
    for key in cases or grad_cases(entry):
        c = grad_case(*key)
        got = impl(entry, c)
        fp = GRAD_FP32[key]
        tabs = (0,) if entry == "pairs_apply_p1_null" else (0, 1)
        for k, kd in enumerate(c["kinds"]):
            tag, a = (entry, key, k), kd["active"]
            if kd["stamp"] is not None:
                after = kd["stamp"].copy()
                after[a] = c["first"] + c["steps"] - 1
                assert np.array_equal(got[k]["stamp"], after), (tag, "stamp")
            for n, ref in c["ref"][k].items():
                r = a if int(n[1]) in tabs else np.zeros_like(a)
                assert np.array_equal(got[k][n][~r].view(np.int32), kd[n][~r].view(np.int32)), \
                    (tag, n, "a row without a gradient changed")
                f = _frac(_err(got[k][n][r], ref[r], n[0]), fp[n[0]])
                worst[n[0]] = max(worst.get(n[0], 0.0), f)
                assert f < 1.0, (tag, n, f)
        if entry == "flat_clock_close":     # t rose by one per launch, reserved 0, the seed
            t, reserved, seed = got[0]["clock"]
            assert (t, reserved) == (c["t_now"] + c["steps"], 0), (key, t, reserved)
            assert seed == A.splitmix_seed(SEED, t), (key, seed)
        if entry == "pairs_apply_gsum_clock":
            # the same bits as ncf_adam_pairs_apply_clock fed the fp32 sum taken in rank order
            same = impl("pairs_apply_clock", c)
            for k in range(len(c["kinds"])):
                for n in NAMES + ("stamp",):
                    assert np.array_equal(got[k][n].view(np.int32), same[k][n].view(np.int32)), (key, k, n)
    return worst


# ----------------------------------------------------------------------------- the schedule
SCHED_STEPS, SCHED_EVERY, SCHED_LR_AT = 40, 8, 25
SCHED_WIDTHS = (16, 64, 256)


def sched_lr(t):
    return 1e-3 if t < SCHED_LR_AT else 3e-4


@functools.lru_cache(maxsize=2)
def sched_case(D):
    """Fresh tables (moments 0, stamps 0) and 40 steps of touched rows: 0-60 of the 203 rows (0-2
    of the 5), half of them the step before's, a third of the rows never, step 13 nobody."""
    g = np.random.default_rng(4000 + D)
    c = dict(D=D, hp=A.HP, lr=sched_lr, steps=SCHED_STEPS, every=SCHED_EVERY, kinds=[])
    for k, rows in enumerate(ROWS):
        t = {}
        for tb in (0, 1):
            t[f"p{tb}"] = _params(g, (rows, D))
            t[f"m{tb}"] = np.zeros((rows, D), F32)
            t[f"v{tb}"] = np.zeros((rows, D), F32)
        pool = np.nonzero(np.arange(rows) % 3 != 2)[0]
        touched, prev = [], np.zeros(0, np.int64)
        for s in range(1, SCHED_STEPS + 1):
            n = 0 if s == 13 else int(g.integers(0, min(61, len(pool) - 1)))
            keep = prev[:n // 2]
            new = g.permutation(np.setdiff1d(pool, keep))[:n - len(keep)]
            ids = np.concatenate([keep, new]).astype(np.int64)
            prev = g.permutation(ids)
            touched.append((ids, tuple(_grad(g, t[f"p{tb}"][ids]) for tb in (0, 1))))
        never = np.setdiff1d(np.arange(rows), np.concatenate([x[0] for x in touched]))
        assert len(never) >= rows // 3
        c["kinds"].append(dict(t, rows=rows, touched=touched, stamp=np.zeros(rows, np.int32)))
    c["ref"] = sched_dense(c, F64)
    return c


def sched_dense(c, dtype):
    out = []
    for kd in c["kinds"]:
        r = {}
        for tb in (0, 1):
            tt = [(ids, G[tb]) for ids, G in kd["touched"]]
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = A.dense_schedule(
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
    """``impl(case)`` -> (per kind dict(p0 .. v1, stamp) after the closing sweep, per step and
    kind the oldest stamp after that step's rolling sweep).  Every row against the dense schedule
    in float64; after step s >= 8 no stamp is older than 8 steps."""
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
            f = _frac(_err(got[k][n], c["ref"][k][n], n[0]), fp[n[0]])
            worst[n[0]] = max(worst.get(n[0], 0.0), f)
            assert f < 1.0, (D, k, n, f)
    return worst


# ----------------------------------------------------------------------------- the fp32 figures
# The fp32 restatement's worst distance from float64 per case (p absolute, m and v relative),
# one host thread; the bound of a quantity is 4 x its figure.  tests/test_adam_cpu.py re-measures
# each and holds it within [0.25 x, 1.001 x] of what it measures.
REPLAY_FP32 = {
    (16, 17, "base"): {"p": 1.2734e-07, "m": 5.3561e-07, "v": 1.1895e-06},
    (16, 17, "wd0"): {"p": 1.1994e-07, "m": 7.7926e-07, "v": 6.2772e-07},
    (16, 330, "base"): {"p": 3.1038e-07, "m": 1.2210e-06, "v": 1.7295e-06},
    (16, 330, "wd0"): {"p": 2.8959e-07, "m": 4.0253e-06, "v": 9.1024e-07},
    (16, 330, "lr_change"): {"p": 3.3960e-07, "m": 1.1553e-06, "v": 1.7382e-06},
    (16, 330, "lr0"): {"p": 3.3789e-07, "m": 8.3100e-07, "v": 2.5247e-06},
    (32, 17, "base"): {"p": 1.5391e-07, "m": 6.0938e-07, "v": 1.0811e-06},
    (32, 17, "wd0"): {"p": 1.2926e-07, "m": 7.6483e-07, "v": 7.0902e-07},
    (32, 330, "base"): {"p": 2.8720e-07, "m": 1.3564e-06, "v": 1.9057e-06},
    (32, 330, "wd0"): {"p": 3.1398e-07, "m": 3.9468e-06, "v": 1.0445e-06},
    (32, 330, "lr_change"): {"p": 3.6538e-07, "m": 9.9311e-07, "v": 1.6428e-06},
    (32, 330, "lr0"): {"p": 2.7031e-07, "m": 1.0685e-06, "v": 2.8216e-06},
    (64, 17, "base"): {"p": 1.3086e-07, "m": 6.4280e-07, "v": 9.5100e-07},
    (64, 17, "wd0"): {"p": 1.3647e-07, "m": 7.8307e-07, "v": 7.3174e-07},
    (64, 330, "base"): {"p": 3.0917e-07, "m": 1.1336e-06, "v": 1.8682e-06},
    (64, 330, "wd0"): {"p": 3.4825e-07, "m": 4.0475e-06, "v": 9.7538e-07},
    (64, 330, "lr_change"): {"p": 4.8945e-07, "m": 1.6490e-06, "v": 1.9121e-06},
    (64, 330, "lr0"): {"p": 2.5442e-07, "m": 1.1699e-06, "v": 2.5247e-06},
    (128, 17, "base"): {"p": 1.3408e-07, "m": 6.7449e-07, "v": 1.2529e-06},
    (128, 17, "wd0"): {"p": 1.3555e-07, "m": 8.4569e-07, "v": 7.1106e-07},
    (128, 330, "base"): {"p": 3.5921e-07, "m": 1.2446e-06, "v": 3.0407e-06},
    (128, 330, "wd0"): {"p": 3.4890e-07, "m": 4.1445e-06, "v": 1.1402e-06},
    (128, 330, "lr_change"): {"p": 4.2662e-07, "m": 1.3494e-06, "v": 2.1105e-06},
    (128, 330, "lr0"): {"p": 3.5122e-07, "m": 1.1298e-06, "v": 3.3406e-06},
    (256, 17, "base"): {"p": 1.6160e-07, "m": 6.7360e-07, "v": 1.2210e-06},
    (256, 17, "wd0"): {"p": 1.3905e-07, "m": 8.5906e-07, "v": 7.2435e-07},
    (256, 330, "base"): {"p": 3.6865e-07, "m": 1.3606e-06, "v": 2.5190e-06},
    (256, 330, "wd0"): {"p": 4.1586e-07, "m": 4.1085e-06, "v": 1.0871e-06},
    (256, 330, "lr_change"): {"p": 3.5833e-07, "m": 1.2574e-06, "v": 3.9231e-06},
    (256, 330, "lr0"): {"p": 3.9453e-07, "m": 1.1693e-06, "v": 3.0823e-06},
}
GRAD_FP32 = {
    ("table", 16, "slot"): {"p": 4.0562e-08, "m": 3.1350e-07, "v": 2.1751e-07},
    ("table", 16, "null"): {"p": 4.0562e-08, "m": 3.1350e-07, "v": 2.5277e-07},
    ("table", 32, "slot"): {"p": 4.2579e-08, "m": 2.7100e-07, "v": 2.7860e-07},
    ("table", 32, "null"): {"p": 4.2408e-08, "m": 2.9749e-07, "v": 2.5567e-07},
    ("table", 64, "slot"): {"p": 4.3255e-08, "m": 2.9887e-07, "v": 2.6749e-07},
    ("table", 64, "null"): {"p": 4.2030e-08, "m": 2.9887e-07, "v": 2.6749e-07},
    ("table", 128, "slot"): {"p": 4.3847e-08, "m": 2.9841e-07, "v": 2.9833e-07},
    ("table", 128, "null"): {"p": 4.3847e-08, "m": 3.1272e-07, "v": 2.6034e-07},
    ("table", 256, "slot"): {"p": 4.3675e-08, "m": 3.0948e-07, "v": 2.8561e-07},
    ("table", 256, "null"): {"p": 4.3679e-08, "m": 3.1357e-07, "v": 2.7196e-07},
    ("table", 256, "big"): {"p": 4.4298e-08, "m": 3.4697e-07, "v": 3.5666e-07},
    ("dense", 64, "zeros"): {"p": 4.2859e-08, "m": 3.1861e-07, "v": 2.5135e-07},
    ("flat", 1, ""): {"p": 7.8502e-09, "m": 3.8615e-08, "v": 2.6174e-08},
    ("flat", 3, ""): {"p": 1.7373e-08, "m": 6.4002e-08, "v": 1.3540e-07},
    ("flat", 4, ""): {"p": 2.5918e-08, "m": 6.2523e-08, "v": 1.4183e-07},
    ("flat", 5, ""): {"p": 1.9601e-08, "m": 6.6904e-08, "v": 6.7905e-08},
    ("flat", 1023, ""): {"p": 4.0775e-08, "m": 1.5319e-07, "v": 2.5078e-07},
    ("flat", 1027, ""): {"p": 4.1023e-08, "m": 1.3467e-07, "v": 2.0969e-07},
    ("flat", 1048835, ""): {"p": 4.4400e-08, "m": 2.1719e-07, "v": 3.2986e-07},
    ("flat", 4194311, ""): {"p": 4.4502e-08, "m": 2.3706e-07, "v": 3.5429e-07},
    ("apply", 16, ""): {"p": 4.0651e-08, "m": 1.5052e-07, "v": 2.2915e-07},
    ("apply", 32, ""): {"p": 4.2496e-08, "m": 1.5565e-07, "v": 3.2318e-07},
    ("apply", 64, ""): {"p": 4.1645e-08, "m": 1.5814e-07, "v": 2.7427e-07},
    ("apply", 128, ""): {"p": 4.2668e-08, "m": 1.8737e-07, "v": 3.1834e-07},
    ("apply", 256, ""): {"p": 4.4538e-08, "m": 1.7830e-07, "v": 2.7541e-07},
    ("gsum", 16, 1): {"p": 4.1898e-08, "m": 1.7504e-07, "v": 2.9548e-07},
    ("gsum", 16, 3): {"p": 4.3166e-08, "m": 2.3471e-07, "v": 3.4209e-07},
    ("gsum", 32, 1): {"p": 4.1553e-08, "m": 1.7604e-07, "v": 2.7092e-07},
    ("gsum", 32, 3): {"p": 4.1283e-08, "m": 2.0433e-07, "v": 3.9375e-07},
    ("gsum", 64, 1): {"p": 4.2369e-08, "m": 1.9077e-07, "v": 2.5501e-07},
    ("gsum", 64, 3): {"p": 4.2405e-08, "m": 2.3107e-07, "v": 3.8857e-07},
    ("gsum", 128, 1): {"p": 4.3287e-08, "m": 2.1472e-07, "v": 2.7277e-07},
    ("gsum", 128, 3): {"p": 4.1943e-08, "m": 2.2540e-07, "v": 3.7724e-07},
    ("gsum", 256, 1): {"p": 4.3895e-08, "m": 2.3685e-07, "v": 3.6317e-07},
    ("gsum", 256, 3): {"p": 4.3783e-08, "m": 2.4338e-07, "v": 4.2049e-07},
}
SCHED_FP32 = {
    16: {"p": 1.8518e-07, "m": 1.0539e-06, "v": 1.5272e-06},
    64: {"p": 2.2306e-07, "m": 1.2166e-06, "v": 1.9087e-06},
    256: {"p": 2.3399e-07, "m": 1.0695e-06, "v": 2.1126e-06},
}


# ----------------------------------------------------------------------------- the kernels
class _Dev:
    """The kinds of a case on the device, their ncf_table_pair array, a clock at t_now."""

    def __init__(self, c, kinds=None, two=True):
        from ncf_amd import _lib
        self.kinds, self.keep = [], []
        src = kinds if kinds is not None else c["kinds"]
        self.pairs = (_lib.TablePair * len(src))()
        for pr, kd in zip(self.pairs, src):
            d = {n: torch.from_numpy(kd[n]).to(DEV) for n in NAMES if kd.get(n) is not None}
            for n in ("stamp", "ids"):
                if kd.get(n) is not None:
                    d[n] = torch.from_numpy(kd[n]).to(DEV)
            self.kinds.append(d)
            pr.p0, pr.m0, pr.v0 = (d[n].data_ptr() for n in NAMES[:3])
            if two and "p1" in d:
                pr.p1, pr.m1, pr.v1 = (d[n].data_ptr() for n in NAMES[3:])
            pr.row_ids = d["ids"].data_ptr() if "ids" in d else None
            pr.stamp = d["stamp"].data_ptr() if "stamp" in d else None
            pr.rows, pr.param_dtype = kd["rows"], _lib.DTYPE_F32
        self.count = torch.tensor([kd.get("count", 0) for kd in src] + [0], dtype=torch.int32, device=DEV)
        self.clock = torch.tensor([c.get("t_now", 0), SEED], dtype=torch.int64, device=DEV)
        self.st = _lib.stream_ptr(DEV)

    @property
    def pa(self):
        return ctypes.addressof(self.pairs)

    def ptrs(self, k, two=True):
        d = self.kinds[k]
        return [d[n].data_ptr() for n in NAMES[:3]] + \
            [d[n].data_ptr() if two else None for n in NAMES[3:]]

    def gradients(self, k, G0, G1):
        g0, g1 = torch.from_numpy(G0).to(DEV), torch.from_numpy(G1).to(DEV)
        self.keep += [g0, g1]
        self.pairs[k].g0, self.pairs[k].g1 = g0.data_ptr(), g1.data_ptr()
        return g0, g1

    def result(self):
        torch.cuda.synchronize()
        return [{n: x.cpu().numpy() for n, x in d.items() if n != "ids"} for d in self.kinds]

    def clock_words(self):
        t = self.clock.cpu()
        w = int(t[0])
        return w & 0xFFFFFFFF, (w >> 32) & 0xFFFFFFFF, int(t[1]) & ((1 << 64) - 1)


@functools.lru_cache(maxsize=4)
def gpu_step_table(lr, upto):
    """The step table as deferred._ensure fills it: one ncf_adam_step_scalars call per run of
    equal lr, padded PAD steps past the highest step used."""
    from ncf_amd import _lib
    host = np.zeros(4 * (upto + PAD + 1), F32)
    for first, last, x in lr_segments(lr, upto + PAD):
        _lib.call("ncf_adam_step_scalars", x, A.HP[0], A.HP[1], A.HP[2], first, last - first + 1,
                  host[4 * first:].ctypes.data)
    return torch.from_numpy(host).to(DEV)


def gpu_replay(entry, c):
    from ncf_amd import _lib
    name, arg = entry
    D, target, hp = c["D"], c["target"], c["hp"]
    d = _Dev(c)
    tab = gpu_step_table(c["lr"], target).data_ptr()
    clk, cnt, st, rel = d.clock.data_ptr(), d.count.data_ptr(), d.st, c["rel"]
    K = range(len(c["kinds"]))
    if name == "rows_catchup":
        for k in K:
            _lib.call("ncf_adam_rows_catchup", *d.ptrs(k, arg), D, d.kinds[k]["ids"].data_ptr(), cnt,
                      k, MAX_N, d.kinds[k]["stamp"].data_ptr(), target, tab, *hp, st)
    elif name == "rows_catchup_clock":
        for k in K:
            _lib.call("ncf_adam_rows_catchup_clock", *d.ptrs(k, arg), D,
                      d.kinds[k]["ids"].data_ptr(), cnt, k, MAX_N, d.kinds[k]["stamp"].data_ptr(),
                      rel, clk, tab, *hp, st)
    elif name == "pairs_catchup_clock":
        _lib.call("ncf_adam_pairs_catchup_clock", d.pa, 2, D, cnt, MAX_N, rel, clk, tab, *hp, st)
    elif name == "pairs_catchup_lock_clock":
        _lib.call("ncf_adam_pairs_catchup_lock_clock", d.pa, 2, D, cnt, MAX_N, rel, arg, clk, tab,
                  *hp, st)
    elif name == "reduce_batch_catchup":
        lst = _lib.ReduceList()
        lst.count = 0
        scratch = torch.zeros(4, device=DEV)
        _lib.call("ncf_reduce_batch_catchup", lst.address, scratch.data_ptr(), scratch.numel(),
                  d.pa, 2, D, cnt, MAX_N, rel, clk, tab, *hp, st)
    elif name == "pairs_catchup_claim_clock":
        raw = [torch.from_numpy(kd["raw"]).to(DEV) for kd in c["kinds"]]
        _lib.call("ncf_adam_pairs_catchup_claim_clock", d.pa, 2, D, raw[0].data_ptr(),
                  raw[1].data_ptr(), raw[0].numel(), rel, clk, tab, *hp, st)
    elif name == "sweep":
        for k in K:
            _lib.call("ncf_adam_sweep", *d.ptrs(k), SWEEP_RANGE[k][0], SWEEP_RANGE[k][1], D,
                      d.kinds[k]["stamp"].data_ptr(), target, tab, *hp, st)
    elif name == "sweep_rolling":
        for k in K:
            rows = c["kinds"][k]["rows"]
            _lib.call("ncf_adam_sweep_rolling", *d.ptrs(k), rows, (rows + arg - 1) // arg, arg, D,
                      d.kinds[k]["stamp"].data_ptr(), rel, clk, tab, *hp, st)
    elif name == "pairs_sweep_rolling":
        _lib.call("ncf_adam_pairs_sweep_rolling", d.pa, 2, D, arg, rel, clk, tab, *hp, st)
    elif name == "pairs_sweep_rolling_part":
        for part in range(NPARTS):
            _lib.call("ncf_adam_pairs_sweep_rolling_part", d.pa, 2, D, arg, rel, part, NPARTS, clk,
                      tab, *hp, st)
    else:
        raise KeyError(name)
    out = d.result()
    assert d.clock_words() == (c["t_now"], 0, SEED)        # (the clock is read only)
    return out


def gpu_gradient(entry, c):
    from ncf_amd import _lib
    hp, first, fam = c["hp"], c["first"], c["family"]
    d = _Dev(c, two=entry != "pairs_apply_p1_null")
    tab = gpu_step_table(c["lr"], first + c["steps"]).data_ptr()
    clk, cnt, st = d.clock.data_ptr(), d.count.data_ptr(), d.st
    kd = c["kinds"][0]
    for s in range(c["steps"]):
        step = first + s
        if fam in ("table", "dense", "flat"):
            x = d.kinds[0]
            p, m, v = (x[n].data_ptr() for n in NAMES[:3])
            rows, D = kd["p0"].shape
            G = kd["g"][s][0]
            if entry == "table":
                slot = np.full(rows, -1, np.int32)
                slot[kd["touched"]] = np.arange(len(kd["touched"]), dtype=np.int32)
                sl, Gc = torch.from_numpy(slot).to(DEV), torch.from_numpy(G[kd["touched"]]).to(DEV)
                null = c["b"] == "null"
                _lib.call("ncf_adam_table", p, m, v, rows, D, None if null else sl.data_ptr(),
                          None if null else Gc.data_ptr(), 1e-3, *hp, float(step), st)
                continue
            g = torch.from_numpy(G).to(DEV)
            d.keep.append(g)
            if entry == "table_dense_grad":
                _lib.call("ncf_adam_table_dense_grad", p, g.data_ptr(), m, v, rows * D, 1e-3, *hp,
                          float(step), st)
            elif entry == "flat":
                _lib.call("ncf_adam_flat", p, g.data_ptr(), m, v, rows * D, 1e-3, *hp, float(step), st)
            elif entry == "flat_clock":       # the clock stands at first - 1: step_rel = 1 + s
                _lib.call("ncf_adam_flat_clock", p, g.data_ptr(), m, v, rows * D, tab, 1 + s, clk,
                          *hp, st)
            else:                               # the closing form advances the clock itself
                _lib.call("ncf_adam_flat_clock_close", p, g.data_ptr(), m, v, rows * D, tab, 1, clk,
                          *hp, SEED, st)
            continue
        D = c["a"]
        for k, kk in enumerate(c["kinds"]):
            d.gradients(k, *kk["G"][s])
        if entry in ("rows_apply", "rows_apply_clock"):
            for k, kk in enumerate(c["kinds"]):
                p0, m0, v0, p1, m1, v1 = d.ptrs(k)
                g0, g1 = d.pairs[k].g0, d.pairs[k].g1
                ids, stamp = d.kinds[k]["ids"].data_ptr(), d.kinds[k]["stamp"].data_ptr()
                if entry == "rows_apply":
                    _lib.call("ncf_adam_rows_apply", p0, m0, v0, g0, p1, m1, v1, g1, D, ids, cnt, k,
                              MAX_N, stamp, step, tab, *hp, st)
                else:
                    _lib.call("ncf_adam_rows_apply_clock", p0, m0, v0, g0, p1, m1, v1, g1, D, ids, cnt,
                              k, MAX_N, stamp, 1 + s, clk, tab, *hp, st)
        elif entry in ("pairs_apply_clock", "pairs_apply_p1_null"):
            _lib.call("ncf_adam_pairs_apply_clock", d.pa, 2, D, cnt, MAX_N, 1 + s, clk, tab, *hp, st)
        elif entry == "pairs_apply_gsum_clock":
            # one `got` for both kinds: kind 1's rows follow kind 0's
            got = torch.from_numpy(np.concatenate([kk["got"][s] for kk in c["kinds"]])).to(DEV)
            off = c["kinds"][0]["got"][s].shape[0]
            pos = [torch.from_numpy(np.where(kk["pos"][s] >= 0, kk["pos"][s] + o, -1).astype(np.int32)).to(DEV)
                   for kk, o in zip(c["kinds"], (0, off))]
            _lib.call("ncf_adam_pairs_apply_gsum_clock", d.pa, 2, D, cnt, MAX_N, 1 + s, got.data_ptr(),
                      pos[0].data_ptr(), pos[1].data_ptr(), c["b"], clk, tab, *hp, st)
            torch.cuda.synchronize()
        else:
            raise KeyError(entry)
    out = d.result()
    if entry == "flat_clock_close":
        out[0]["clock"] = d.clock_words()
    else:
        assert d.clock_words() == (c["t_now"], 0, SEED)
    return out


def gpu_schedule(c):
    """The calls of one deferred step as deferred.py issues them: the catch-up of the step's rows
    to the clock's step, their apply (step clock->t + 1), the rolling sweep of that step's slice,
    the clock advance; ncf_adam_sweep to the last step at the end."""
    from ncf_amd import _lib
    D, hp = c["D"], c["hp"]
    kinds = [dict(kd, ids=np.zeros(MAX_N, np.int64), count=0) for kd in c["kinds"]]
    d = _Dev(dict(t_now=0), kinds=kinds)
    tab = gpu_step_table(c["lr"], c["steps"]).data_ptr()
    clk, cnt, st = d.clock.data_ptr(), d.count.data_ptr(), d.st
    oldest = []
    for s in range(c["steps"]):
        n = []
        for k, kd in enumerate(c["kinds"]):
            ids, G = kd["touched"][s]
            buf = np.resize(np.arange(kd["rows"]), MAX_N).astype(np.int64)     # valid past the count
            buf[:len(ids)] = ids
            d.kinds[k]["ids"].copy_(torch.from_numpy(buf))
            Gc = [np.zeros((MAX_N, D), F32) for _ in (0, 1)]
            for tb in (0, 1):
                Gc[tb][:len(ids)] = G[tb]
            d.gradients(k, *Gc)
            n.append(len(ids))
        d.count.copy_(torch.tensor(n + [0], dtype=torch.int32))
        _lib.call("ncf_adam_pairs_catchup_clock", d.pa, 2, D, cnt, MAX_N, 0, clk, tab, *hp, st)
        _lib.call("ncf_adam_pairs_apply_clock", d.pa, 2, D, cnt, MAX_N, 1, clk, tab, *hp, st)
        _lib.call("ncf_adam_pairs_sweep_rolling", d.pa, 2, D, c["every"], 1, clk, tab, *hp, st)
        _lib.call("ncf_step_clock_advance", clk, SEED, st)
        torch.cuda.synchronize()
        oldest.append([int(x["stamp"].min()) for x in d.kinds])
    for k, kd in enumerate(c["kinds"]):
        _lib.call("ncf_adam_sweep", *d.ptrs(k), 0, kd["rows"], D, d.kinds[k]["stamp"].data_ptr(),
                  c["steps"], tab, *hp, st)
    assert d.clock_words()[0] == c["steps"]
    return d.result(), oldest


def _line(what, worst):
    print(f"{what}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()) + " of the bound")


@pytest.mark.parametrize("name", sorted({e[0] for e in REPLAY_ENTRIES}))
@pytest.mark.parametrize("D", WIDTHS)
def test_replay_vs_float64(D, name):
    for entry in REPLAY_ENTRIES:
        if entry[0] == name:
            _line(f"replay {entry} D {D}", check_replay(D, entry, gpu_replay))


@pytest.mark.parametrize("entry", GRAD_ENTRIES)
def test_gradient_step_vs_float64(entry):
    _line(f"gradient step {entry}", check_gradient_step(entry, gpu_gradient))


@pytest.mark.parametrize("D", SCHED_WIDTHS)
def test_schedule_vs_dense_float64(D):
    _line(f"schedule D {D}", check_schedule(D, gpu_schedule))
