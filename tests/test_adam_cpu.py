"""The premises of tests/test_gpu_adam.py, without a GPU: on every case of every check there the
fp32 restatement (tests/adam_ref.py evaluated in float32) passes with at most a quarter of each
bound used and reproduces the figures recorded beside the cases; one missing or extra owed step
moves every replayed element by at least 20 x the bound; the mutants a subtly wrong kernel would
be fail the same check on the same inputs.  Also: ncf_adam_step_scalars (a host function) to the
last bit of fp32, and the rolling sweep's slice arithmetic."""
import numpy as np
import pytest

from tests import adam_ref as A
from tests import test_gpu_adam as G

F32, F64, LOCK = A.F32, A.F64, A.LOCK


# ----------------------------------------------------------------------------- the fp32 restatement
def _full32(c, key, **kw):
    """The fp32 replay of every row of the case (cached on the case per mutant)."""
    cache = c.setdefault("_f32", {})
    if key not in cache:
        cache[key] = _replay_all32(c, **kw)
    return cache[key]


def _replay_all32(c, stamps=None, target=None, scalars=None, zero=None, lr=None):
    out = []
    for kd in c["kinds"]:
        st = kd["stamp"] if stamps is None else stamps(kd["stamp"])
        to = c["target"] if target is None else target(st)
        r = {}
        for tb in (0, 1):
            r[f"p{tb}"], r[f"m{tb}"], r[f"v{tb}"] = A.replay(
                kd[f"p{tb}"], kd[f"m{tb}"], kd[f"v{tb}"], st, to, lr or c["lr"], c["hp"], F32,
                scalars=None if scalars is None else scalars(c), zero=zero)
        out.append(r)
    return out


def cpu_replay(key="", arith=None, select=None, keep_stamp=False, one_table=False):
    """The fp32 restatement as an implementation for G.check_replay.  The arguments make the
    mutants: ``arith`` other arithmetic (arguments of _replay_all32), ``select`` other rows
    (arguments of G.plan), the stamp of a replayed row not written, the second table skipped."""
    def impl(entry, c):
        full = _full32(c, key, **(arith or {}))
        out = []
        for k, (kd, (rep, after, tabs)) in enumerate(zip(c["kinds"], G.plan(entry, c, **(select or {})))):
            r = {"stamp": kd["stamp"].copy() if keep_stamp else after}
            for n in G.NAMES:
                r[n] = kd[n].copy()
                if int(n[1]) in (tabs if not one_table else (0,)):
                    r[n][rep] = full[k][n][rep]
            out.append(r)
        return out
    return impl


def cpu_gradient(scal=None, rank0=False, tail=False):
    """The fp32 restatement for G.check_gradient_step; mutants: other scalars, the gradient sum's
    rank 0 only, the n % 4 tail of a flat buffer left unchanged."""
    def impl(entry, c):
        if rank0 and c["family"] == "gsum":
            c = dict(c, kinds=[_rank0(kd) for kd in c["kinds"]])
        tabs = (0,) if entry == "pairs_apply_p1_null" else (0, 1)
        res = G.grad_steps(c, F32, tables=tabs, scal=scal)
        out = []
        for kd, r in zip(c["kinds"], res):
            r = {n: x.astype(F32) for n, x in r.items()}
            if tail and c["family"] == "flat":
                n4 = kd["rows"] // 4 * 4
                for n in r:
                    r[n][n4:] = kd[n][n4:]
            if kd["stamp"] is not None:
                r["stamp"] = kd["stamp"].copy()
                r["stamp"][kd["active"]] = c["first"] + c["steps"] - 1
            out.append(r)
        if entry == "flat_clock_close":
            t = c["t_now"] + c["steps"]
            out[0]["clock"] = (t, 0, A.splitmix_seed(G.SEED, t))
        return out
    return impl


def _rank0(kd):
    G0 = []
    for got, pos in zip(kd["got"], kd["pos"]):
        x = np.where(pos[:, :1] >= 0, got[np.maximum(pos[:, 0], 0)], F32(0))
        D = x.shape[1] // 2
        G0.append((x[:, :D].copy(), x[:, D:].copy()))
    return dict(kd, G=G0)


def cpu_schedule(c):
    """The dense schedule in fp32 (the deferred one takes the same steps of every element in the
    same order), and the stamps the call sequence leaves."""
    res = [{n: x.astype(F32) for n, x in r.items()} for r in G.sched_dense(c, F32)]
    oldest = [[] for _ in range(c["steps"])]
    for k, kd in enumerate(c["kinds"]):
        stamp = np.zeros(kd["rows"], np.int32)
        for s in range(1, c["steps"] + 1):
            stamp[kd["touched"][s - 1][0]] = s
            r0, n = G.slice_rows(kd["rows"], c["every"], s)
            stamp[r0:r0 + n] = s
            oldest[s - 1].append(int(stamp.min()))
        res[k]["stamp"] = np.full(kd["rows"], c["steps"], np.int32)
    return res, oldest


def _reproduced(recorded, measured, tag):
    """The recorded figure is what is measured here: no bound wider than 4.004 x it."""
    for q, v in measured.items():
        assert v <= recorded[q] <= 1.001 * v and 0.25 * v <= recorded[q], (tag, q, recorded[q], v)


# ----------------------------------------------------------------------------- headroom
@pytest.mark.parametrize("D", G.WIDTHS)
def test_replay_fp32_restatement_passes_with_headroom(D):
    for target, variant in G.REPLAY_CASES:
        c = G.replay_case(D, target, variant)
        _reproduced(G.REPLAY_FP32[(D, target, variant)], G.measure_replay(c), (D, target, variant))
        for kd in c["kinds"]:       # neighbours in the list, one wave at D < 64, differ in gap
            gap = target - (kd["stamp"][kd["ids"][:kd["count"]]] & ~LOCK).astype(np.int64)
            assert bool((np.diff(gap) != 0).all())
    total = {}
    for entry in G.REPLAY_ENTRIES:
        for q, v in G.check_replay(D, entry, cpu_replay()).items():
            total[q] = max(total.get(q, 0.0), v)
    print(f"replay fp32 D {D}: " + " ".join(f"{q} {v:.3g}" for q, v in total.items()))
    assert max(total.values()) <= 0.25, total


@pytest.mark.parametrize("entry", G.GRAD_ENTRIES)
def test_gradient_step_fp32_restatement_passes_with_headroom(entry):
    for key in G.grad_cases(entry):
        _reproduced(G.GRAD_FP32[key], G.measure_grad(G.grad_case(*key)), key)
    worst = G.check_gradient_step(entry, cpu_gradient())
    print(f"gradient step fp32 {entry}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst


def test_gradient_cases_reach_the_second_grid_stride_trip():
    """grid_for caps a grid at 4096 blocks of 256 threads; k_adam_flat_close at 64 blocks."""
    cap = 4096 * 256
    assert 16400 * 256 // 4 > cap and G.FLAT_BIG["flat"] > cap and G.FLAT_BIG["flat_clock"] > cap
    assert G.FLAT_BIG["flat_clock_close"] // 4 > cap and G.FLAT_BIG["flat_clock_close"] % 4 == 3


@pytest.mark.parametrize("D", G.SCHED_WIDTHS)
def test_schedule_fp32_restatement_passes_with_headroom(D):
    c = G.sched_case(D)
    _reproduced(G.SCHED_FP32[D], G.measure_sched(c), D)
    worst = G.check_schedule(D, cpu_schedule)
    print(f"schedule fp32 D {D}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst
    for kd in c["kinds"]:           # the short last slice; slices past the 5-row table
        sl = [G.slice_rows(kd["rows"], c["every"], s) for s in range(8)]
        assert sum(n for _, n in sl) == kd["rows"]
        assert sl[7] == ((182, 21) if kd["rows"] == 203 else (7, 0))


# ----------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("D", G.WIDTHS)
def test_one_owed_step_is_twenty_bounds(D):
    """One missing or extra owed step moves every replayed element by at least 20 x the p bound
    (wd = 0: the m bound, see tests/test_gpu_adam.py); across lr = 0 steps p stands still and the
    same holds for v."""
    for target, variant in G.REPLAY_CASES:
        c = G.replay_case(D, target, variant)
        fp, sens = G.REPLAY_FP32[(D, target, variant)], G.replay_sensitivity(c)
        q = "m" if variant == "wd0" else "p"
        assert c["lr"](target) > 0
        assert 20 * 4 * fp[q] <= sens[q], (D, target, variant, q, fp[q], sens[q])
        if variant == "lr0":
            assert 20 * 4 * fp["v"] <= sens["v"], (D, target, variant, fp["v"], sens["v"])
            # the float64 reference itself: a row resting at the start of the span keeps its p
            # across it (m and v decay)
            kd = c["kinds"][0]
            a, b = target - 61, target - 41
            st = np.full(kd["rows"], a)
            p, m, v = A.replay(kd["p0"], kd["m0"], kd["v0"], st, b, c["lr"], c["hp"], F64)
            assert np.array_equal(p, kd["p0"].astype(F64)) and bool((np.abs(m) < np.abs(kd["m0"])).any())
            assert bool((v != kd["v0"]).all())


# ----------------------------------------------------------------------------- mutants
def _scal(f):
    """scalars(c) -> (t -> AdamScalars) from f(c, t, make)."""
    return lambda c: (lambda t: f(c, t, lambda lr, tt: A.make_scalars(lr, c["hp"], tt)))


def _adamw_zero(p, m, v, s, dtype):
    """Decoupled weight decay: p shrinks by lr wd p, the moments see no gradient."""
    c = {k: dtype(x) for k, x in s.items()}
    lr = -c["neg_step"] * (dtype(1) - dtype(0.9) ** dtype(s["t"]))
    p = p * (dtype(1) - lr * c["wd"])
    m, v = c["b1"] * m, c["b2"] * v
    return p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"]), m, v


CATCHUP, SWEEP = ("pairs_catchup_clock", None), ("sweep", None)
BASE, LRC, LR0 = ((330, "base"),), ((330, "lr_change"),), ((330, "lr0"),)
REPLAY_MUTANTS = {
    "one_step_short": (CATCHUP, BASE, dict(key="short", arith=dict(target=lambda st: 329))),
    "one_step_short_fresh": (SWEEP, ((17, "base"),), dict(key="short", arith=dict(target=lambda st: 16))),
    "one_step_long": (CATCHUP, BASE, dict(key="long", arith=dict(stamps=lambda st: st - 1))),
    "whole_chunks_only": (CATCHUP, BASE, dict(key="chunks", arith=dict(
        target=lambda st: np.where(st < 330, st + (330 - st.astype(np.int64)) // 8 * 8, 330)))),
    "target_steps_scalars": (CATCHUP, LRC, dict(key="tsc", arith=dict(
        scalars=_scal(lambda c, t, make: make(c["lr"](330), 330))))),
    "target_steps_scalars_fresh": (SWEEP, ((17, "base"),), dict(key="tsc", arith=dict(
        scalars=_scal(lambda c, t, make: make(c["lr"](17), 17))))),
    "new_lr_before_the_change": (CATCHUP, LRC, dict(key="newlr", arith=dict(lr=lambda t: 3e-4))),
    "k2_dropped": (CATCHUP, BASE, dict(key="k2", arith=dict(
        scalars=_scal(lambda c, t, make: dict(make(c["lr"](t), t), k2=F32(0)))))),
    "decoupled_weight_decay": (CATCHUP, BASE, dict(key="adamw", arith=dict(
        scalars=_scal(lambda c, t, make: dict(make(c["lr"](t), t), t=t)), zero=_adamw_zero))),
    "locked_row_replayed": (CATCHUP, BASE, dict(key="locked", arith=dict(stamps=lambda st: st & ~LOCK),
                                                select=dict(locked_too=True))),
    "locked_row_swept": (SWEEP, BASE, dict(key="locked", arith=dict(stamps=lambda st: st & ~LOCK),
                                           select=dict(locked_too=True))),
    "stamp_not_written": (CATCHUP, BASE, dict(keep_stamp=True)),
    "rows_past_count": (CATCHUP, BASE, dict(select=dict(all_ids=True))),
    "rows_past_count_rows_form": (("rows_catchup", True), BASE, dict(select=dict(all_ids=True))),
    "second_table_skipped": (CATCHUP, BASE, dict(one_table=True)),
    "rolling_slice_last_row": (("pairs_sweep_rolling", 8), BASE, dict(select=dict(drop_last=True))),
    "rolling_short_slice_last_row": (("sweep_rolling", 3), ((17, "base"),), dict(select=dict(drop_last=True))),
    "lr0_span_moves_p": (CATCHUP, LR0, dict(key="lr0moves", arith=dict(
        scalars=_scal(lambda c, t, make: make(c["lr"](t) or 1e-6, t))))),
}


@pytest.mark.parametrize("D", [16, 64, 256])
@pytest.mark.parametrize("name", list(REPLAY_MUTANTS))
def test_replay_mutant_fails(name, D):
    entry, cases, kw = REPLAY_MUTANTS[name]
    G.check_replay(D, entry, cpu_replay(), cases=cases)
    with pytest.raises(AssertionError):
        G.check_replay(D, entry, cpu_replay(**kw), cases=cases)


GRAD_MUTANTS = {
    "bias_correction2_missing": ("pairs_apply_clock", ("apply", 16, ""), dict(
        scal=lambda lr, hp, t: dict(A.make_scalars(lr, hp, t), inv_bc=F32(1)))),
    "bias_correction2_missing_flat": ("flat", ("flat", 5, ""), dict(
        scal=lambda lr, hp, t: dict(A.make_scalars(lr, hp, t), inv_bc=F32(1)))),
    "gsum_rank0_only": ("pairs_apply_gsum_clock", ("gsum", 16, 3), dict(rank0=True)),
    "flat_tail_dropped": ("flat_clock_close", ("flat", 1027, ""), dict(tail=True)),
    "flat_tail_dropped_5": ("flat_clock_close", ("flat", 5, ""), dict(tail=True)),
}


@pytest.mark.parametrize("name", list(GRAD_MUTANTS))
def test_gradient_step_mutant_fails(name):
    entry, key, kw = GRAD_MUTANTS[name]
    G.check_gradient_step(entry, cpu_gradient(), cases=[key])
    with pytest.raises(AssertionError):
        G.check_gradient_step(entry, cpu_gradient(**kw), cases=[key])


# ----------------------------------------------------------------------------- host arithmetic
def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _want(lr, t):
    s = A.make_scalars(lr, A.HP, t)
    return [s["neg_step"], s["inv_bc"], s["ra"], s["rb"]]


def test_step_scalars_to_the_last_bit():
    """ncf_adam_step_scalars against adam_ref: steps 1-64, 1000 and 100000 (first > 1), and at
    lr = 0 the finite constants of the zero-gradient form."""
    import _ncf_pkg
    _ncf_pkg.load()
    from ncf_amd import _lib
    b1, b2, eps, _ = A.HP
    for lr in (1e-3, 3e-4, 0.0):
        host = np.full(4 * 64, np.nan, F32)
        _lib.call("ncf_adam_step_scalars", lr, b1, b2, eps, 1, 64, host.ctypes.data)
        assert np.array_equal(_bits(host), _bits(A.step_table(lambda t: lr, A.HP, 64)[4:]))
        for first, count in ((5, 60), (1000, 1), (100000, 2)):
            host = np.full(4 * count, np.nan, F32)
            _lib.call("ncf_adam_step_scalars", lr, b1, b2, eps, first, count, host.ctypes.data)
            want = sum((_want(lr, first + i) for i in range(count)), [])
            assert np.array_equal(_bits(host), _bits(want)), (lr, first)
        if lr == 0.0:
            assert host[2] == host[3] == F32(-3.0e38) and host[0] == 0.0 and bool(np.isfinite(host).all())
    # the table of an lr change, filled as deferred._ensure fills it
    lr = G.lr_of(330, "lr_change")
    seg = G.lr_segments(lr, 400)
    assert seg == [(1, 290, 1e-3), (291, 400, 3e-4)]
    assert G.lr_segments(G.lr_of(330, "lr0"), 400) == [(1, 269, 1e-3), (270, 289, 0.0), (290, 400, 1e-3)]
    host = np.zeros(4 * 401, F32)
    for first, last, x in seg:
        _lib.call("ncf_adam_step_scalars", x, b1, b2, eps, first, last - first + 1,
                  host[4 * first:].ctypes.data)
    assert np.array_equal(_bits(host), _bits(A.step_table(lr, A.HP, 400)))


def test_splitmix_seed_known_values():
    """clock_advance's seed: splitmix64 of base + (t + 1) golden ratios, 62 bits."""
    assert A.splitmix_seed(0, 0) == 0xE220A8397B1DCDAF & 0x3FFFFFFFFFFFFFFF   # splitmix64's first output
    assert A.splitmix_seed(7, 3) != A.splitmix_seed(7, 4) and A.splitmix_seed(7, 3) < 1 << 62


@pytest.mark.parametrize("total", [1, 5, 8, 203, 1000])
@pytest.mark.parametrize("every", [1, 4, 8, 64])
@pytest.mark.parametrize("nparts", [1, 3])
def test_rolling_slices_cover_every_row_once(total, every, nparts):
    """Over ``every`` consecutive targets the slices and parts of k_pairs_sweep (restated:
    G.slice_rows) cover every row of the table exactly once, in range."""
    for t0 in (0, 329):
        seen = np.zeros(total, np.int64)
        for t in range(t0, t0 + every):
            whole = G.slice_rows(total, every, t)
            at = whole[0]
            for part in range(nparts):
                r0, n = G.slice_rows(total, every, t, part, nparts)
                assert n >= 0 and r0 == at and (n == 0 or r0 + n <= total)
                seen[r0:r0 + n] += 1
                at += n
            assert at == whole[0] + whole[1]
        assert bool((seen == 1).all()), (total, every, nparts, t0)
