"""The premises of tests/test_gpu_adamw.py and tests/test_gpu_adamw_step.py, without a GPU: the
float64 restatement (tests/adamw_ref.py) equals torch.optim.AdamW; the decoupled step table
(deferred.adamw_step_scalars) to the last bit; on every case of every GPU check the fp32
restatement passes with at most a quarter of each bound used and reproduces the figures recorded
beside the cases; one missing or extra owed step moves every replayed element by at least 20 x the bound; the mutants a
subtly wrong kernel would be fail the same check on the same inputs; the host-side refusals; the
share of sign-flip-zone elements of the model-level cases."""
import types

import numpy as np
import pytest
import torch

from tests import adamw_ref as W
from tests import parity
from tests import test_gpu_adamw as T
from tests import test_gpu_adamw_step as S

F32, F64, LOCK = W.F32, W.F64, W.LOCK
G = T.G


# ----------------------------------------------------------------------------- against torch
def test_float64_restatement_equals_torch_adamw():
    """40 steps, float64, 12 rows of which 5 never get a gradient and the others some steps only;
    lr changes at step 15, wd at step 25.  The rows without a gradient take the folded
    zero-gradient form, with the scalars left in double.  1e-14 relative: rounding-order slack in
    double (measured 5.6e-17 absolute), not a fitted bound."""
    g = np.random.default_rng(5)
    rows, D, steps = 12, 7, 40
    p0 = g.uniform(-0.5, 0.5, (rows, D))
    lr = lambda t: 1e-3 if t < 15 else 3e-4          # noqa: E731
    hp = lambda t: (0.9, 0.999, 1e-8, 1e-2 if t < 25 else 0.2)   # noqa: E731
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.AdamW([tp], lr=lr(1), weight_decay=hp(1)[3], foreach=False)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, steps + 1):
        ids = np.nonzero((g.random(rows) < 0.4) & (np.arange(rows) >= 5))[0]
        grad = np.zeros_like(p0)
        grad[ids] = g.normal(0, 1e-2, (len(ids), D))
        for grp in opt.param_groups:
            grp["lr"], grp["weight_decay"] = lr(t), hp(t)[3]
        tp.grad = torch.tensor(grad)
        opt.step()
        s = W.make_scalars(lr(t), hp(t), t, rounded=False)
        a = W.adamw_step(p, m, v, grad, None, None, None, F64, s=s)
        b = W.zero_step_folded(p, m, v, s, F64)
        has = np.isin(np.arange(rows), ids)[:, None]
        p, m, v = (np.where(has, x, y) for x, y in zip(a, b))
    st = opt.state[tp]
    worst = float(np.abs(p - tp.detach().numpy()).max())
    print(f"restatement vs torch.optim.AdamW: max |dp| {worst:.3g}")
    assert np.allclose(p, tp.detach().numpy(), rtol=1e-14, atol=0)
    assert np.allclose(m, st["exp_avg"].numpy(), rtol=1e-14, atol=0)
    assert np.allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-14, atol=0)
    assert bool((m[:5] == 0).all() and (v[:5] == 0).all())     # never touched: no moments at all
    assert type(torch.optim.Adam([tp], decoupled_weight_decay=True)) is torch.optim.Adam


# ----------------------------------------------------------------------------- the step table
def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def test_adamw_step_scalars_to_the_last_bit():
    """deferred.adamw_step_scalars (the decoupled table: ncf_adam_step_scalars' four floats, the
    decay, zeros) against the restatement, bit for bit.  The four floats come from the library
    and are checked against an independent restatement; the decay column is one Python expression
    on both sides (no C function computes it), so for that column this holds the layout, the
    dtype and the lr == 0 / wd == 0 cases, not the arithmetic."""
    import _ncf_pkg
    _ncf_pkg.load()
    from ncf_amd import _lib
    from ncf_amd.deferred import adamw_step_scalars
    S8 = _lib.ADAMW_TABLE_STRIDE
    assert S8 == W.STRIDE == 8 and _lib.ADAM_DECOUPLED == 0x100
    b1, b2, eps = W.HP[:3]
    for lr, wd in ((1e-3, 1e-2), (3e-4, 0.5), (0.0, 0.5), (1e-3, 0.0)):
        hp = (b1, b2, eps, wd)
        for first, count in ((1, 64), (5, 60), (1000, 1), (100000, 2)):
            host = np.full(S8 * count, np.nan, F32)
            adamw_step_scalars(lr, b1, b2, eps, wd, first, count, host)
            want = W.step_table(lambda t: lr, hp, first + count - 1)[S8 * first:]
            assert np.array_equal(_bits(host), _bits(want)), (lr, wd, first)
            four = np.full(4 * count, np.nan, F32)
            _lib.call("ncf_adam_step_scalars", lr, b1, b2, eps, first, count, four.ctypes.data)
            assert np.array_equal(_bits(host.reshape(count, S8)[:, :4]), _bits(four.reshape(count, 4)))
            dk = host.reshape(count, S8)[:, 4]
            assert bool((dk == F32(1.0 - lr * wd)).all())
            if lr == 0.0 or wd == 0.0:
                assert bool((dk == F32(1.0)).all())
    # the table of an lr and a wd change, filled as deferred._ensure fills it
    lr, hp = T.lr_of(330, "lr_change"), T.hp_of(330, "wd_change")
    seg = T.segments(lr, hp, 400)
    assert seg == [(1, 290, 1e-3, 0.5), (291, 300, 3e-4, 0.5), (301, 400, 3e-4, 0.25)]
    host = np.zeros(S8 * 401, F32)
    for first, last, x, wd in seg:
        adamw_step_scalars(x, b1, b2, eps, wd, first, last - first + 1, host[S8 * first:])
    assert np.array_equal(_bits(host), _bits(W.step_table(lr, hp, 400)))


# ----------------------------------------------------------------------------- the fp32 restatement
def cpu_replay(arith=None, select=None):
    """The fp32 restatement as an implementation for T.check_replay.  ``arith``: other arithmetic
    (arguments of T.replay_all: mutants); ``select``: other rows (arguments of G.plan)."""
    def impl(entry, c):
        full = T.replay_all(c, **arith) if arith else c["f32"]
        out = []
        for k, (kd, (rep, after, _)) in enumerate(zip(c["kinds"], G.plan(entry, c, **(select or {})))):
            r = {"stamp": after}
            for n in T.NAMES:
                r[n] = kd[n].copy()
                r[n][rep] = full[k][n][rep]
            out.append(r)
        return out
    return impl


def cpu_gradient(**kw):
    def impl(entry, c):
        out = []
        for kd, r in zip(c["kinds"], T.grad_steps(c, F32, **kw)):
            r = {n: x.astype(F32) for n, x in r.items()}
            if kd["stamp"] is not None:
                r["stamp"] = kd["stamp"].copy()
                r["stamp"][kd["active"]] = c["first"] + c["steps"] - 1
            out.append(r)
        if entry == "flat_clock_close":
            t = c["t_now"] + c["steps"]
            out[0]["clock"] = (t, 0, G.A.splitmix_seed(G.SEED, t))
        return out
    return impl


def cpu_schedule(c):
    res = [{n: x.astype(F32) for n, x in r.items()} for r in T.sched_dense(c, F32)]
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


@pytest.mark.parametrize("D", T.WIDTHS)
def test_replay_fp32_restatement_passes_with_headroom(D):
    for target, variant in T.REPLAY_CASES:
        c = T.replay_case(D, target, variant)
        _reproduced(T.REPLAY_FP32[(D, target, variant)], T.measure_replay(c), (D, target, variant))
        for kd in c["kinds"]:       # both populations are replayed, and skipped
            b = G.behind(kd, target)
            assert bool((b & kd["never"]).any()) and (kd["rows"] < 10 or bool((b & ~kd["never"]).any()))
    total = {}
    for entry in T.REPLAY_ENTRIES:
        for q, v in T.check_replay(D, entry, cpu_replay()).items():
            total[q] = max(total.get(q, 0.0), v)
    print(f"adamw replay fp32 D {D}: " + " ".join(f"{q} {v:.3g}" for q, v in total.items()))
    assert max(total.values()) <= 0.25, total


@pytest.mark.parametrize("entry", T.GRAD_ENTRIES)
def test_gradient_step_fp32_restatement_passes_with_headroom(entry):
    for key in T.grad_cases(entry):
        _reproduced(T.GRAD_FP32[key], T.measure_grad(T.grad_case(*key)), key)
    worst = T.check_gradient_step(entry, cpu_gradient())
    print(f"adamw gradient step fp32 {entry}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst
    cap = 4096 * 256                # the sizes reach the second grid-stride trip
    assert 16400 * 256 // 4 > cap and min(G.FLAT_BIG["flat"], G.FLAT_BIG["flat_clock"]) > cap
    assert G.FLAT_BIG["flat_clock_close"] // 4 > cap


@pytest.mark.parametrize("D", T.SCHED_WIDTHS)
def test_schedule_fp32_restatement_passes_with_headroom(D):
    c = T.sched_case(D)
    _reproduced(T.SCHED_FP32[D], T.measure_sched(c), D)
    worst = T.check_schedule(D, cpu_schedule)
    print(f"adamw schedule fp32 D {D}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst
    for k, kd in enumerate(c["kinds"]):   # rows that never get a gradient keep no moments at all
        never = np.setdiff1d(np.arange(kd["rows"]), np.concatenate([x[0] for x in kd["touched"]]))
        assert len(never) >= kd["rows"] // 3
        assert bool((c["ref"][k]["m0"][never] == 0).all())


def cpu_bwd_apply(**kw):
    """The fp32 restatement (tests/embed_ref.py's backward in the kernels' order, then AdamW) as an
    implementation for T.check_bwd_apply; the keyword arguments make the mutants."""
    def impl(c):
        st = T.bwd_apply_steps(c, F32, **kw)
        last = c["first"] + c["steps"] - 1
        stamps = [(np.full(c["e"]["uniq_" + k].numel(), last), np.full(3, c["t_now"])) for k in "ui"]
        return dict(tables={k: tuple(np.asarray(x, F32) for x in v) for k, v in st.items()},
                    untouched=True, stamps=stamps)
    return impl


@pytest.mark.parametrize("D", T.BWD_DIMS)
def test_embedding_bwd_apply_fp32_restatement_passes_with_headroom(D):
    c = T.bwd_apply_case(D)
    _reproduced(T.BWD_FP32[D], T.measure_bwd_apply(c), D)
    worst = T.check_bwd_apply(D, cpu_bwd_apply())
    print(f"adamw embedding backward + apply fp32 D {D}: " + " ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 0.25, worst
    cov = T.E.coverage(c["e"]["sorted_u"])       # single-piece and multi-piece segments both step
    assert cov["singletons"] and cov["ten_pieces"] and cov["eighteen_pieces"] and cov["split_pair"]
    for k in T.R.TABLES:                         # the floors are far below the typical moment
        assert float(np.median(np.abs(c["ref"][k][1]))) > 3 * T.M_FLOOR
        assert float(np.median(np.abs(c["ref"][k][2]))) > 3 * T.V_FLOOR


BWD_MUTANTS = {
    "coupled_decay": dict(step=lambda p, m, v, g, lr, t, hp, dtype=F64, s=None: _coupled_step(
        p, m, v, g, lr, t, hp, dtype, s=s)),
    "decay_after_the_adam_term": dict(step=lambda *a, **k: _after_step(*a, **k)),
    "first_steps_scalars_at_every_step": dict(scal=lambda lr, hp, t: W.make_scalars(lr, hp, T.FIRST)),
}


@pytest.mark.parametrize("name", list(BWD_MUTANTS))
def test_embedding_bwd_apply_mutant_fails(name):
    T.check_bwd_apply(16, cpu_bwd_apply())
    with pytest.raises(AssertionError):
        T.check_bwd_apply(16, cpu_bwd_apply(**BWD_MUTANTS[name]))


# ----------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("D", T.WIDTHS)
def test_one_owed_step_is_twenty_bounds(D):
    """One missing or extra owed step moves every replayed element by at least 20 x the p bound:
    a never-touched one through that step's decay, a touched-history one through the decaying m
    as well.  wd = 0: a never-touched row stands still (held bitwise by the check), and the
    condition is held on m of the touched-history rows."""
    for target, variant in T.REPLAY_CASES:
        c = T.replay_case(D, target, variant)
        fp, sens = T.REPLAY_FP32[(D, target, variant)], T.replay_sensitivity(c)
        q = "m" if variant == "wd0" else "p"
        assert c["lr"](target) > 0
        assert 20 * 4 * fp[q] <= sens[q], (D, target, variant, q, fp[q], sens[q])


# ----------------------------------------------------------------------------- mutants
def _coupled_zero(p, m, v, s, dtype):
    """Coupled L2 in place of decoupled decay: wd p enters the moments, nothing multiplies p."""
    c = {k: dtype(x) for k, x in s.items()}
    g = c["wd"] * p
    m = m + c["w1"] * (g - m)
    v = v * c["b2"] + c["c2"] * g * g
    return p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"]), m, v


def _decay_after(p, m, v, s, dtype):
    """The decay applied after the Adam term instead of before it."""
    c = {k: dtype(x) for k, x in s.items()}
    m, v = c["b1"] * m, v * c["b2"]
    return (p + m / (np.sqrt(v) * c["ra"] + c["rb"])) * c["decay"], m, v


def _k_terms_left(p, m, v, s, dtype):
    """adam0's k1 / k2 terms left in the zero-gradient step."""
    c = {k: dtype(x) for k, x in s.items()}
    m = c["b1"] * m + c["w1"] * c["wd"] * p
    v = c["c2"] * c["wd"] * c["wd"] * p * p + v * c["b2"]
    return p * c["decay"] + m / (np.sqrt(v) * c["ra"] + c["rb"]), m, v


def _with_wd(c, t):
    return dict(W.make_scalars(c["lr"](t), c["hp"](t), t), wd=F32(c["hp"](t)[3]))


CATCHUP, SWEEP8 = ("pairs_catchup_clock", None), ("pairs_sweep_rolling", 8)
BASE, LRC, WDC = ((330, "base"),), ((330, "lr_change"),), ((330, "wd_change"),)
REPLAY_MUTANTS = {
    "coupled_decay": (CATCHUP, BASE, dict(arith=dict(scalars=_with_wd, zero=_coupled_zero))),
    "decay_after_the_adam_term": (CATCHUP, BASE, dict(arith=dict(zero=_decay_after))),
    "decay_with_a_constant_lr": (CATCHUP, LRC, dict(arith=dict(scalars=lambda c, t: dict(
        W.make_scalars(c["lr"](t), c["hp"](t), t),
        decay=F32(1.0 - c["lr"](330) * c["hp"](t)[3]))))),
    "decay_with_a_constant_wd": (CATCHUP, WDC, dict(arith=dict(scalars=lambda c, t: dict(
        W.make_scalars(c["lr"](t), c["hp"](t), t),
        decay=F32(1.0 - c["lr"](t) * c["hp"](330)[3]))))),
    "k_terms_left": (CATCHUP, BASE, dict(arith=dict(scalars=_with_wd, zero=_k_terms_left))),
    "one_step_short": (CATCHUP, BASE, dict(arith=dict(target=329))),
    "one_step_short_sweep": (SWEEP8, BASE, dict(arith=dict(target=329))),
    "rows_past_count": (CATCHUP, BASE, dict(select=dict(all_ids=True))),
    "rolling_slice_last_row": (SWEEP8, BASE, dict(select=dict(drop_last=True))),
    "locked_row_replayed": (CATCHUP, BASE, dict(select=dict(locked_too=True))),
}


def _mutant_impl(kw):
    arith = dict(kw.get("arith") or {})

    def impl(entry, c):
        a = dict(arith)
        if "scalars" in a:
            f = a["scalars"]
            a["scalars"] = lambda t: f(c, t)
        a.setdefault("target", c["target"])
        sel = kw.get("select")
        if sel and sel.get("locked_too"):       # the locked rows replayed as if they were behind
            kinds = [dict(kd, stamp=kd["stamp"] & ~LOCK) for kd in c["kinds"]]
            full = T.replay_all(dict(c, kinds=kinds), c["target"], F32)
            out = cpu_replay(select=sel)(entry, dict(c, f32=full))
            return out
        return cpu_replay(arith=dict(a, dtype=F32) if kw.get("arith") else None, select=sel)(entry, c)
    return impl


@pytest.mark.parametrize("D", [16, 64, 256])
@pytest.mark.parametrize("name", list(REPLAY_MUTANTS))
def test_replay_mutant_fails(name, D):
    entry, cases, kw = REPLAY_MUTANTS[name]
    T.check_replay(D, entry, cpu_replay(), cases=cases)
    with pytest.raises(AssertionError):
        T.check_replay(D, entry, _mutant_impl(kw), cases=cases)


def _coupled_step(p, m, v, g, lr, t, hp, dtype=F64, s=None):
    c = {k: dtype(x) for k, x in s.items()}
    g = g + dtype(T.WD) * p
    m = m + c["w1"] * (g - m)
    v = v * c["b2"] + c["c2"] * g * g
    return p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"]), m, v


def _after_step(p, m, v, g, lr, t, hp, dtype=F64, s=None):
    c = {k: dtype(x) for k, x in s.items()}
    m = m + c["w1"] * (g - m)
    v = v * c["b2"] + c["c2"] * g * g
    return (p + c["neg_step"] * m / (np.sqrt(v) * c["inv_bc"] + c["eps"])) * c["decay"], m, v


GRAD_MUTANTS = {
    "coupled_decay": ("pairs_apply_clock", ("apply", 16, ""), dict(step=_coupled_step)),
    "coupled_decay_flat": ("flat_clock_close", ("flat", 1027, ""), dict(step=_coupled_step)),
    "decay_after_the_adam_term": ("pairs_apply_clock", ("apply", 16, ""), dict(step=_after_step)),
    "no_decay": ("flat", ("flat", 5, ""), dict(
        scal=lambda lr, hp, t: dict(W.make_scalars(lr, hp, t), decay=F32(1)))),
    "bias_correction2_missing": ("table", ("table", 64, "slot"), dict(
        scal=lambda lr, hp, t: dict(W.make_scalars(lr, hp, t), inv_bc=F32(1)))),
    "second_table_skipped": ("pairs_apply_clock", ("apply", 64, ""), dict(tables=(0,))),
}


@pytest.mark.parametrize("name", list(GRAD_MUTANTS))
def test_gradient_step_mutant_fails(name):
    entry, key, kw = GRAD_MUTANTS[name]
    T.check_gradient_step(entry, cpu_gradient(), cases=[key])
    with pytest.raises(AssertionError):
        T.check_gradient_step(entry, cpu_gradient(**kw), cases=[key])


# ----------------------------------------------------------------------------- host logic
def test_plain_adam_accepts_both_spellings_of_decoupled_decay():
    import _ncf_pkg
    _ncf_pkg.load()
    from ncf_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    cases = [(torch.optim.Adam(p), True, False), (torch.optim.AdamW(p), True, True),
             (torch.optim.Adam(p, decoupled_weight_decay=True), True, True),
             (torch.optim.AdamW(p, amsgrad=True), False, True),
             (torch.optim.AdamW(p, maximize=True), False, True),
             (torch.optim.SGD(p, lr=0.1), False, False)]
    for opt, plain, dec in cases:
        assert optim._is_plain_adam(opt) is plain, opt
        if plain:
            assert optim._decoupled(opt, opt.param_groups[0]) is dec, opt


def test_host_side_refusals():
    import _ncf_pkg
    _ncf_pkg.load()
    from ncf_amd.deferred import DeferredTableAdam
    from ncf_amd.distributed import HipShardOps
    from ncf_amd.trainer import FusedTrainStep, ModelTrainer
    untouched = object()            # refused before anything of the model is touched
    with pytest.raises(ValueError, match="fp32 tables"):
        FusedTrainStep(untouched, table_dtype=torch.bfloat16, decoupled_weight_decay=True)
    with pytest.raises(NotImplementedError, match="coupled"):
        HipShardOps(untouched, 4, 4, 1, decoupled_weight_decay=True)
    tables = {k: torch.zeros(4, 16) for k in ("mf_user", "mlp_user", "mf_item", "mlp_item")}
    eng = types.SimpleNamespace(table_params=lambda: tables, deferred=None,
                                model=types.SimpleNamespace(num_users=4, num_products=4))
    with pytest.raises(ValueError, match="step clock"):
        DeferredTableAdam(eng, decoupled_weight_decay=True)
    lp = {k: v.to(torch.bfloat16) for k, v in tables.items()}
    with pytest.raises(ValueError, match="fp32 tables"):
        DeferredTableAdam(eng, clock=torch.zeros(2, dtype=torch.int64), param_tables=lp,
                          decoupled_weight_decay=True)
    assert eng.deferred is None
    net = torch.nn.Linear(2, 2)
    cfg = dict(num_users=4, num_products=4, batch_size=2, learning_rate=1e-3, weight_decay=1e-2)
    assert type(ModelTrainer(net, cfg).optimizer) is torch.optim.Adam
    tr = ModelTrainer(net, dict(cfg, optimizer="adamw"))
    assert type(tr.optimizer) is torch.optim.AdamW
    assert tr.optimizer.param_groups[0]["weight_decay"] == 1e-2
    assert tr.optimizer.param_groups[0]["lr"] == 1e-3
    with pytest.raises(ValueError, match="optimizer"):
        ModelTrainer(net, dict(cfg, optimizer="sgd"))


# ----------------------------------------------------------------------------- sign-flip zone
def _oracle_pair(D, clip):
    """The fp32 oracle run of tests/test_gpu_adamw_step.py's inputs and the same run in float64."""
    m = S.model(D)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    order = [n for n, _ in m.named_parameters()]
    data = S.batches()[:S.STEPS]
    mn = S.CLIP[D] if clip else None
    r32, mom, zones = S.oracle_run(D, init, order, data, max_norm=mn)
    norms = list(S.oracle_run.norms)
    init64 = {k: (v.double() if v.is_floating_point() else v) for k, v in init.items()}
    r64, _, _ = S.oracle_run(D, init64, order, [(u, i, t.double()) for u, i, t in data], max_norm=mn)
    return r32, r64, mom, zones, norms


@pytest.mark.parametrize("D", sorted(S.GEOMS))
@pytest.mark.parametrize("clip", [False, True])
def test_sign_flip_zone_share_of_the_model_cases(D, clip):
    """What the inputs of tests/test_gpu_adamw_step.py were chosen for, from the CPU oracle alone.
    At every step the sign-flip zone of every compared tensor (reference |g| < parity.ZONE, g != 0;
    no wd term) is within parity.ZONE_CAP of its elements, one element in tensors under 1000, as
    parity.assert_params_close caps the elements that may differ.  Every step of a clipped run
    clips.  Outside the zone the fp32 oracle stands within half of assert_params_close's 1e-6 of
    the same oracle in float64 (measured: 3.6e-7 at most)."""
    r32, r64, mom, zones, norms = _oracle_pair(D, clip)
    assert len(zones) > 10 and all(len(z) == S.STEPS for z in zones.values())
    if clip:
        assert len(norms) == S.STEPS and min(norms) > S.CLIP[D], norms
    worst = 0.0
    for k, zs in zones.items():
        if k in parity.ANALYTIC_ZERO_GRAD:
            continue
        cap = max(1, int(parity.ZONE_CAP * zs[0].size))
        for s, z in enumerate(zs):
            assert int(z.sum()) <= cap, (D, clip, k, s, int(z.sum()), zs[0].size)
        d = (r32[k].double() - r64[k]).abs().numpy()[np.sum(zs, axis=0) == 0]
        worst = max(worst, float(d.max()) if d.size else 0.0)
        assert float(mom[k]["step"]) == S.STEPS
    print(f"fp32 oracle vs float64 oracle outside the zone, D {D} clip {clip}: {worst:.3g}")
    assert worst <= 0.5e-6, worst
