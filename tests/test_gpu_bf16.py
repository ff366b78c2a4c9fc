"""The bf16-table configuration (BASELINE.json configs[1] "bf16"; SURVEY 8(d) C2: tables bf16,
Adam moments fp32) on the MI355X.

* Its deferred schedule reproduces its own dense schedule (every table swept every step,
  ncf_adam_table_bf16) bit for bit: parameters (bf16) and moments (fp32).
* Against the fp32 CPU oracle (oracle/ncf_oracle.py, pinned to the reference's goldens) over
  100 training steps: every step's loss within 1% and the final eval probabilities within 2e-2
  (SURVEY 8(c) bf16 tolerances); the fp32 parity path stays the reference (test_gpu_parity).
* Against a float64 reference, rounded once: the table update ncf_adam_table_bf16 alone stores
  round-to-nearest-even of the float64 Adam result (a truncating store, or a moment a few ulps
  off, fails), and one bf16-table step on the fp32 tower (engine.BF16_MM = False: the tables are
  the only bf16 thing) matches the float64 oracle on the widened tables at the fp32 tolerances,
  with dropout off and on: the bf16 gather (both float4 forms) and the bf16 segment reduce.

* The bf16 tower itself (engine.BF16_MM = True, the benchmark's bf16 configuration: the tower's
  nine GEMMs on single-term bf16 MFMA) against tests/bf16_tower.py's restatement of its operand
  rounding, in float64:
  - layer by layer, teacher-forced (test_bf16_tower_layer_by_layer): every reference layer starts
    from the fp32 bits the step itself stored one stage earlier, so only fp32 accumulation order
    separates the two, and the bounds are the number format's (bf16_tower's docstring) with the
    project's fp32 tolerances asserted beside them.  Forward, backward, bias / gamma / beta sums
    and the weight gradients in both forms: wgrad.hip on the stored fp32 dlin and a (MLP_WGRAD
    off: nothing rounded, a mixed-precision step) and the fused bf16 ones of a second, otherwise
    bit-identical run;
  - one step end to end (test_bf16_step_end_to_end_vs_restated_oracle) in the forms that keep
    everything in LDS, against O.train_step(linear=bf16_linear): a quantity is asserted where the
    rounding flips a correct fp32 evaluation shows (measured on the CPU at test time, x 4) stay
    4 x below every wrong rounding and the unrounded oracle (E2E below; tests/test_bf16_tower.py
    re-checks that without a GPU).

Out of scope here: TOWER_SPLIT (off; held to the fp32 MFMA in test_gpu_parity) and the C5 bf16
scan (held to the fp32 scan and the oracle).
"""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")


def _batches(U, I, B, M, n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = (torch.rand(B * M, generator=g) ** 2 * I).long().clamp_max(I - 1)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        out.append((u, i, t.reshape(-1, 1)))
    return out


def _run_bf16(deferred, steps, U=3000, I=500, B=64, seed=31):
    from ncf_amd.trainer import FusedTrainStep
    torch.manual_seed(seed)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, 4).to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, deferred=deferred,
                          table_dtype=torch.bfloat16)
    for u, i, t in _batches(U, I, B, 5, steps, seed + 1):
        step(u.to(DEV), i.to(DEV), t.to(DEV))
    step.sync()
    return ({k: v.detach().cpu().clone() for k, v in step.tables_lp.items()},
            {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
             for k, v in step.state.items()}, m)


def test_bf16_deferred_bitwise_equals_dense_bf16():
    a_t, a_m, _ = _run_bf16(False, 70)
    b_t, b_m, mb = _run_bf16(True, 70)
    for k in a_t:
        assert a_t[k].dtype == torch.bfloat16
        assert torch.equal(a_t[k], b_t[k]), k
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k
    # the model's fp32 table parameters hold the bf16 values after sync (state_dict readers)
    sd = mb.state_dict()
    assert torch.equal(sd["mlp_embedding_collection.embedding_bags.user_id.weight"].cpu(),
                       b_t["mlp_user"].float())


def test_bf16_tables_track_fp32_oracle_over_100_steps():
    from ncf_amd.trainer import FusedTrainStep
    U, I, B, M, steps = 1000, 300, 32, 5, 100
    torch.manual_seed(7)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, M - 1)
    ref = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, table_dtype=torch.bfloat16)
    oopt = O.AdamState(lr=1e-3, weight_decay=1e-5)
    worst = 0.0
    for u, i, t in _batches(U, I, B, M, steps, 8):
        w = step(u.to(DEV), i.to(DEV), t.to(DEV))
        _, oloss, _ = O.train_step(ref, oopt, u, i, t, negative_samples=M - 1, num_heads=4,
                                   temporal_dim=32, n_layers=3)
        rel = abs(float(w.loss.item()) - float(oloss)) / float(oloss)
        worst = max(worst, rel)
    assert worst < 0.01, f"loss drifted {worst:.4%} from the fp32 oracle"
    eu = torch.randint(0, U, (200,), generator=torch.Generator().manual_seed(9))
    ei = torch.randint(0, I, (200,), generator=torch.Generator().manual_seed(10))
    m.eval()
    with torch.no_grad():
        got = m.forward_simple(eu.to(DEV), ei.to(DEV)).cpu()
    want = O.forward(ref, eu, ei, training=False, negative_samples=M - 1, num_heads=4,
                     temporal_dim=32, n_layers=3).reshape(-1)
    assert (got - want).abs().max().item() < 2e-2
    assert np.isfinite(got.numpy()).all()


# ----------------------------------------------------------------------------- float64 references
ADAM_HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-5)
ADAM_ROWS, ADAM_TOUCHED = 1000, 200
# chosen on the CPU: with the fp32 CPU Adam rounded to bf16 in the kernel's place every
# assertion of check_adam_bf16 holds (elements differing from the rounded float64 result per
# step: 0, 0, 0 of 64,000 at D = 64 and 1, 0, 0 of 128,000 at D = 128; largest |fp32 - float64|
# 2.34e-5, on the 1e3 rows, and 0.048 / 0.20 bf16 steps, on elements that cancel to near 0;
# mean signed error at most 7.8e-4 steps against bounds of 1.6e-2 / 1.1e-2)
ADAM_SEED = {64: 1, 128: 1}


def adam_inputs(D, seed):
    """bf16 parameters from N(0, 0.1) with rows of exact 0 (rows 0, 1), 1e3 (2, 3) and 2^-120
    (4); rows 0, 2, 4 and 197 others are touched (a gradient row through the slot map), the
    rest take the weight-decay-only form.  The 2^-120 row is touched only: untouched, its first
    moment is (1 - b1) wd 2^-120 = 7.5e-43, an fp32 denormal with 9 significant bits, and its
    second moment underflows, so no fp32 moment can be within rtol 1e-6 of the float64 one.
    The same gradient every step (so the moments accumulate without cancellation)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(ADAM_ROWS, D, generator=g) * 0.1
    p[0:2] = 0.0
    p[2:4] = 1e3
    p[4] = 2.0 ** -120
    touched = torch.cat([torch.tensor([0, 2, 4]),
                         5 + torch.randperm(ADAM_ROWS - 5, generator=g)[:ADAM_TOUCHED - 3]])
    slot = torch.full((ADAM_ROWS,), -1, dtype=torch.int32)
    slot[touched] = torch.arange(ADAM_TOUCHED, dtype=torch.int32)
    G = torch.randn(ADAM_TOUCHED, D, generator=g)
    return p.to(torch.bfloat16), slot, touched, G


def _adam_ref(p, m, v, grad, t, dtype):
    """Step t of torch's Adam (adam.hip:4-7; oracle.AdamState) from (p, m, v) in ``dtype``."""
    opt = O.AdamState(lr=ADAM_HP["lr"], betas=ADAM_HP["betas"], eps=ADAM_HP["eps"],
                      weight_decay=ADAM_HP["wd"])
    P = {"t": p.to(dtype).clone()}
    opt.state["t"] = {"step": t - 1, "exp_avg": m.to(dtype).clone(),
                      "exp_avg_sq": v.to(dtype).clone()}
    opt.step(P, {"t": grad.to(dtype)})
    return P["t"], opt.state["t"]["exp_avg"], opt.state["t"]["exp_avg_sq"]


def _bf16_step(x):
    """The spacing of bf16 values at |x| (float64): 2^(e - 7), 2^-133 below the normal range."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def cpu_adam_apply(p, m, v, slot, G, grad, t):
    """The fp32 CPU Adam rounded to bf16 (the stand-in the seeds were chosen with)."""
    p32, m32, v32 = _adam_ref(p, m, v, grad, t, torch.float32)
    return p32.to(torch.bfloat16), m32, v32


def check_adam_bf16(D, apply, report=None):
    """Three steps of ``apply`` (p bf16, m, v fp32 -> the same after step t), each against the
    float64 Adam restarted from the state ``apply`` itself left:
    * m, v within rtol 1e-6 of the float64 moments;
    * the stored p equals the float64 p rounded to bf16 (nearest even, the CPU's cast).  An
      element may differ only by exactly one bf16 step and only where the float64 p lies within
      4 x the largest |fp32 torch Adam - float64 Adam| on these inputs of a rounding midpoint
      (both as an absolute distance and counted in bf16 steps at the element, the tighter
      measure for all but the 1e3 rows); at most 0.1% of the elements;
    * the mean signed error in bf16 steps is below 4 / sqrt(count) (truncation: about -0.5)."""
    p, slot, touched, G = adam_inputs(D, ADAM_SEED[D])
    grad = torch.zeros(ADAM_ROWS, D)
    grad[touched] = G
    m, v = torch.zeros(ADAM_ROWS, D), torch.zeros(ADAM_ROWS, D)
    for t in (1, 2, 3):
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        p, m, v = apply(p0, m0, v0, slot, G, grad, t)
        assert p.dtype == torch.bfloat16 and m.dtype == torch.float32
        p64, m64, v64 = _adam_ref(p0, m0, v0, grad, t, torch.float64)
        p32, _, _ = _adam_ref(p0, m0, v0, grad, t, torch.float32)
        torch.testing.assert_close(m.double(), m64, rtol=1e-6, atol=0)
        torch.testing.assert_close(v.double(), v64, rtol=1e-6, atol=0)
        want = p64.to(torch.bfloat16)
        ulp = _bf16_step(p64)
        e32 = (p32.double() - p64).abs()
        e_abs, e_steps = e32.max(), (e32 / ulp).max()
        diff = p.float() != want.float()
        nd = int(diff.sum())
        signed = float(((p.double() - p64) / ulp).mean())
        if report is not None:
            report.append((t, nd, float(e_abs), float(e_steps), signed))
        assert nd <= 1e-3 * p.numel(), (t, nd)
        if nd:
            one = (p.view(torch.int16).int() - want.view(torch.int16).int()).abs() == 1
            assert bool(one[diff].all()), t
            r = p64.abs() / ulp
            mid = ((r - torch.floor(r)) - 0.5).abs()          # in bf16 steps
            assert bool((mid[diff] * ulp[diff] <= 4 * e_abs).all()), t
            assert bool((mid[diff] <= 4 * e_steps).all()), (t, float(mid[diff].max()), float(e_steps))
        assert abs(signed) < 4 / p.numel() ** 0.5, (t, signed)


@pytest.mark.parametrize("D", [64, 128])
def test_adam_table_bf16_rounds_float64_result_to_nearest(D):
    from ncf_amd import _lib
    b1, b2 = ADAM_HP["betas"]
    report = []

    def apply(p0, m0, v0, slot, G, grad, t):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        sl, Gd = slot.to(DEV), G.to(DEV)
        _lib.call("ncf_adam_table_bf16", p.data_ptr(), m.data_ptr(), v.data_ptr(), ADAM_ROWS, D,
                  sl.data_ptr(), Gd.data_ptr(), ADAM_HP["lr"], b1, b2, ADAM_HP["eps"],
                  ADAM_HP["wd"], float(t), _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu()
    try:
        check_adam_bf16(D, apply, report)
    finally:
        for t, nd, ea, es, sg in report:
            print(f"adam bf16 D={D} step {t}: {nd} elements differ; fp32-vs-fp64 {ea:.3g} "
                  f"({es:.3g} bf16 steps); mean signed error {sg:.3g} steps")


@pytest.mark.parametrize("name", ["bf16_d64_p0", "bf16_d64_p02", "bf16_d128_p0", "bf16_d128_p02"])
def test_bf16_table_step_on_fp32_tower_vs_float64_oracle(monkeypatch, name):
    """One FusedTrainStep(table_dtype=bf16, deferred=False) step with engine.BF16_MM = False
    (the tables are the only bf16 thing) against the float64 oracle on the widened tables the
    step object holds, dropout 0 and 0.2 (the restated masks): prob, loss, every dense gradient
    and the compact table gradients at test_gpu_dropout's tolerances (its CASES hold the shapes
    and their CPU-side measurements).  D = 64 gathers a row as one float4 per lane, D = 128 as
    two; ncf_gather_ln_gmf_bf16_fwd and ncf_embedding_bwd_reduce_bf16 are the bf16 kernels in
    the step.  The parameters after Adam are test_adam_table_bf16_rounds_float64_result_to_nearest's."""
    from tests import test_gpu_dropout as TD
    init, batches, rec, final = TD.gpu_run(name, monkeypatch, table_dtype=torch.bfloat16)
    TD.compare(name, init, batches, rec, final, params=False)
    assert [r["seed"] for r in rec] == TD.case_seeds(name, len(rec))


# ----------------------------------------------------------------------------- the bf16 tower
# Layer by layer.  name: the worst fraction the CPU's fp32 evaluation of the same formulas
# (bf16_tower.tower_chain, torch fp32 on rounded operands, one host thread) reaches of (a derived
# bound, a project fp32 tolerance), with the weight gradients unrounded / rounded; both must
# stay below 1/4 (tests/test_bf16_tower.py re-measures).  The b1 case's 0.18 is a weight
# gradient over 5 rows: (5 + 8) u is nearly attained by a sum that short.
LW_CASES = {
    "bf16mm_lw_d64_p0": ((0.047, 0.025), (0.028, 0.025)),
    "bf16mm_lw_d64_p02": ((0.032, 0.053), (0.025, 0.053)),
    "bf16mm_lw_d128_p0": ((0.052, 0.025), (0.031, 0.025)),
    "bf16mm_lw_d128_p02": ((0.053, 0.047), (0.024, 0.047)),
    "bf16mm_lw_b1_p02": ((0.18, 0.031), (0.12, 0.031)),
}


def tower_case(name, data_seed=None):
    """A bf16-tower case's inputs without a GPU: (case, init state with the tables rounded to
    bf16, (u, i, t), the step's seed)."""
    from tests import test_gpu_dropout as TD
    c = TD.CASES[name]
    seed = TD.case_seeds(name, 1)[0]
    sd = TD.make_model(c["D"], c["H"], c["M"], c["p"]).state_dict()
    init = TD.bf16_tables({k: v.detach().clone() for k, v in sd.items()})
    batch = TD.make_batches(c["B"], c["M"], 1, c["data_seed"] if data_seed is None else data_seed)[0]
    return c, init, batch, seed


def cpu_tower(name, rd=None, layers=(0, 1, 2), mask_seed_offset=0):
    """The CPU stand-in for a layer-by-layer case's GPU step: the tower's inputs from the fp32
    oracle's pieces, then bf16_tower.tower_chain in fp32.  Returns what check_tower takes."""
    from tests import bf16_tower as BT
    from tests import test_gpu_dropout as TD
    c, init, (u, i, t), seed = tower_case(name)
    masks = TD.torch_masks(seed, c["B"], c["H"], c["M"], c["p"], torch.float32)
    y, mf = BT.tower_inputs(init, u, i, c["M"], c["H"], masks["attn"])
    T = BT.tower_chain(init, y, mf, masks["mlp"], t, c["D"], rd=rd or BT.RNE, layers=layers)
    return T, init, t, seed


def check_tower(name, T, init, t, seed, wgrad):
    """bf16_tower.tower_checks of a case with the restated masks of ``seed``."""
    from tests import bf16_tower as BT
    from tests import test_gpu_dropout as TD
    c = TD.CASES[name]
    masks = TD.torch_masks(seed, c["B"], c["H"], c["M"], c["p"])
    return BT.tower_checks(T, init, masks["mlp"], t, c["D"], wgrad)


@pytest.mark.parametrize("name", list(LW_CASES))
def test_bf16_tower_layer_by_layer(monkeypatch, name):
    """One FusedTrainStep(table_dtype=bf16, deferred=False) step on the bf16 tower's own launch
    (ncf_mlp_fwd_bf16 / ncf_mlp_bwd_bf16) with a and dlin stored, every stage against the float64
    evaluation of the restated formulas from the step's own previous stage.  Mixed precision of
    this form, asserted as it is: forward and dX round both operands to bf16, while the weight
    gradients (wgrad.hip on the stored fp32 dlin and a) round nothing.  Then the same step with
    the weight gradients fused into the tower backward: everything the two share is bit-identical
    (the same lin_fwd / lin_bwd / ln_bwd code), and its weight gradients are bf(dlin)^T bf(a) of
    the first run's dlin and a, which the second run keeps in LDS."""
    import ncf_amd.engine as E
    from tests import bf16_tower as BT
    from tests import test_gpu_dropout as TD
    init, batches, rec, _ = TD.gpu_run(name, monkeypatch, table_dtype=torch.bfloat16, tower=True)
    assert E.BF16_MM is True and E.MLP_WGRAD is False
    assert [r["seed"] for r in rec] == TD.case_seeds(name, 1)
    (u, i, t), g1 = batches[0], rec[0]
    T = g1["tower"]
    checks = check_tower(name, T, init, t, g1["seed"], "fp32")
    w1 = BT.report(checks, name)
    assert BT.failures(checks) == []
    if TD.CASES[name]["p"] > 0:       # the masks of another seed are another function
        bad = BT.failures(check_tower(name, T, init, t, g1["seed"] + 1, "fp32"))
        assert {"a0", "a1", "a2", "dlin0", "dlin1", "dlin2"} <= set(bad)
    # the fused weight gradients: a second run of the same step
    init2, _, rec2, _ = TD.gpu_run(name + "_fw", monkeypatch, table_dtype=torch.bfloat16, tower=True)
    assert E.MLP_WGRAD is True
    g2 = rec2[0]
    T2 = g2["tower"]
    assert g2["seed"] == g1["seed"] and all(torch.equal(init[k], init2[k]) for k in init)
    for k in ("y", "mf_pred", "prob", "mlp_pred", "dy"):
        assert torch.equal(T[k], T2[k]), k
    for l in range(3):
        for k in ("r", "mean", "rstd"):
            assert torch.equal(T[k][l], T2[k][l]), (k, l)
        for k in BT._names(l)[1:]:
            assert torch.equal(g1["grads"][k], g2["grads"][k]), k
    assert torch.equal(g1["loss"], g2["loss"])
    fused = check_tower(name, dict(T, grads=g2["grads"]), init, t, g1["seed"], "bf16")
    w2 = BT.report([c for c in fused if c.name.endswith(".weight")], name + "_fw")
    assert BT.failures(fused) == []
    # the two forms of the weight gradients differ, and each is held to its own
    assert BT.failures(check_tower(name, T, init, t, g1["seed"], "bf16")) != []
    assert BT.failures(check_tower(name, dict(T, grads=g2["grads"]), init, t, g1["seed"], "fp32")) != []
    print(f"{name}: worst {w1[0]:.3g} / {w1[1]:.3g}; fused weight gradients {w2[0]:.3g} / {w2[1]:.3g}")


# End to end.  The distance of a quantity from the float64 restated oracle is
# bf16_tower.e2e_distance (the largest difference; for a tensor of 1000 elements or more at most
# 0.1% of them may lie beyond it, none beyond 8 x).  Tolerance: 4 x the worst distance of the
# fp32 restated oracle from the float64 one over E2E_SEEDS (the chosen data seeds of the shape;
# one host thread), recorded in E2E_TOL as (tolerance, that worst distance) and re-measured by
# tests/test_bf16_tower.py.  (Recorded, not measured when the GPU test runs: the flips are few
# and discrete, so the figure moves with the host's BLAS kernels; a host whose fp32 oracle
# happens to flip a ReLU would widen the tolerance past the wrong variants.)  E2E[name]: the
# quantities asserted, those whose every wrong variant of bf16_tower.VARIANTS that changes them
# at all, and the unrounded float64 oracle, lie at least 4 x the tolerance away at the case's
# data seed (tests/test_bf16_tower.py asserts it); the figure is the nearest wrong one in
# tolerances.
# Not asserted end to end (the flips of a correct evaluation are as large as a wrong rounding's
# effect): prob, the table gradients, the attention weights' gradients, and the three tower
# weight gradients, whose unrounded form is 0.6 to 1.4 tolerances away; the layer-by-layer test
# holds those.  D = 128, data seed 4 is left out of its seeds: there the fp32 oracle flips a
# layer-0 ReLU (mlp.0.bias 4.5e-3 from float64, 100 x any other seed's).
E2E_SEEDS = {64: (1, 2, 3, 4, 5, 6, 7, 8), 128: (1, 2, 3, 5, 6, 7, 8)}
E2E_TOL = {
    64: {"loss": (1.55e-05, 3.86e-06), "mf_norm.bias": (2.99e-07, 7.45e-08),
         "user_product_attention.out_proj.bias": (8.49e-05, 2.12e-05),
         "mlp.0.bias": (8.43e-05, 2.11e-05), "mlp.2.weight": (8.22e-06, 2.05e-06),
         "mlp.2.bias": (5.71e-06, 1.43e-06), "mlp.4.bias": (6.5e-06, 1.62e-06),
         "mlp.6.bias": (2.14e-06, 5.34e-07), "mlp.8.bias": (3.71e-06, 9.26e-07),
         "mlp.10.weight": (5.68e-06, 1.42e-06), "mlp.10.bias": (2.94e-07, 7.33e-08),
         "mf_output.weight": (2.42e-06, 6.03e-07), "mf_output.bias": (9.86e-07, 2.46e-07),
         "mlp_output.weight": (5.4e-05, 1.35e-05), "mlp_output.bias": (1.8e-06, 4.5e-07),
         "final.0.weight": (4.35e-05, 1.09e-05), "final.0.bias": (4.7e-06, 1.17e-06)},
    128: {"mlp.4.bias": (2.41e-05, 6.01e-06), "mlp.6.bias": (8.8e-06, 2.2e-06),
          "mlp.8.bias": (1.3e-05, 3.23e-06)},
}
E2E = {
    "bf16mm_e2e_small": {
        "loss": 8.9, "mf_norm.bias": 5.2, "user_product_attention.out_proj.bias": 4.7,
        "mlp.0.bias": 7.8, "mlp.2.weight": 4.7, "mlp.2.bias": 9.2, "mlp.4.bias": 11.2,
        "mlp.6.bias": 21.3, "mlp.8.bias": 151.4, "mlp.10.weight": 4.9, "mlp.10.bias": 11.8,
        "mf_output.weight": 6.7, "mf_output.bias": 12.2, "mlp_output.weight": 5.4,
        "mlp_output.bias": 12.2, "final.0.weight": 9.5, "final.0.bias": 11.8},
    "bf16mm_e2e_80": {
        "loss": 5.5, "mf_norm.bias": 5.0, "user_product_attention.out_proj.bias": 4.8,
        "mlp.0.bias": 7.3, "mlp.2.weight": 6.6, "mlp.2.bias": 7.7, "mlp.4.bias": 11.5,
        "mlp.6.bias": 20.1, "mlp.8.bias": 193.6, "mlp.10.weight": 4.5, "mlp.10.bias": 5.5,
        "mf_output.bias": 7.0, "mlp_output.weight": 6.2, "mlp_output.bias": 6.9,
        "final.0.bias": 6.7},
    "bf16mm_e2e_d128": {"mlp.4.bias": 4.7, "mlp.6.bias": 5.3, "mlp.8.bias": 54.9},
}
_e2e_cache = {}


def e2e_quantities(name, data_seed, dtype, linear):
    """prob, loss, every dense gradient and the compact table gradients of the restated oracle's
    step on the case's shape with ``data_seed``'s batch (cached: a reference is computed once)."""
    from tests import test_gpu_dropout as TD
    c = TD.CASES[name]
    key = (c["D"], data_seed, dtype, linear)
    if key not in _e2e_cache:
        c, init, batch, seed = tower_case(name, data_seed)
        rec, _ = TD.oracle_run(init, [batch], [seed], c["H"], c["M"], c["p"], dtype, linear=linear)
        q = {"prob": rec[0]["prob"], "loss": rec[0]["loss"]}
        q.update({k: v for k, v in rec[0]["grads"].items() if k not in TD.TABLE_KEYS.values()})
        for k, K in TD.TABLE_KEYS.items():
            q[K] = rec[0]["grads"][K][torch.unique(batch[0] if "user" in k else batch[1])]
        _e2e_cache[key] = q
    return _e2e_cache[key]


def e2e_fp32_distances(name):
    """The worst e2e_distance of the fp32 restated oracle from the float64 one over the shape's
    data seeds, per quantity (what E2E_TOL records, times 4)."""
    from tests import bf16_tower as BT
    from tests import test_gpu_dropout as TD
    worst = {}
    for s in E2E_SEEDS[TD.CASES[name]["D"]]:
        ref = e2e_quantities(name, s, torch.float64, BT.bf16_linear)
        f32 = e2e_quantities(name, s, torch.float32, BT.bf16_linear)
        for k in ref:
            worst[k] = max(worst.get(k, 0.0), BT.e2e_distance(f32[k], ref[k]))
    return worst


def within(got, want, tol):
    """The capped exclusion: at most 0.1% of the elements beyond tol, none beyond 8 tol."""
    d = (got.double().reshape(want.shape) - want.double()).abs()
    return int((d > tol).sum()) <= int(1e-3 * d.numel()) and float(d.max()) <= 8 * tol


@pytest.mark.parametrize("name", list(E2E))
def test_bf16_step_end_to_end_vs_restated_oracle(monkeypatch, name):
    """One bf16 step (tables and tower) in a form that keeps the tower's activations in LDS: the
    fused attention + tower launch on small and on 80-row tiles (D = 64), the tower's own launch
    with its fused weight gradients (D = 128); p = 0.2.  Against O.train_step(linear=bf16_linear,
    dropout_masks=...) in float64 on the widened tables, the quantities of E2E[name]."""
    import ncf_amd.engine as E
    from tests import bf16_tower as BT
    from tests import test_gpu_dropout as TD
    init, batches, rec, _ = TD.gpu_run(name, monkeypatch, table_dtype=torch.bfloat16)
    assert E.BF16_MM is True and E.MLP_WGRAD is True
    g = rec[0]
    assert g["seed"] == TD.case_seeds(name, 1)[0]
    got = dict(g["grads"], prob=g["prob"], loss=g["loss"])
    got.update({K: g["tab"][k] for k, K in TD.TABLE_KEYS.items()})
    ref = e2e_quantities(name, TD.CASES[name]["data_seed"], torch.float64, BT.bf16_linear)
    assert set(got) == set(ref)
    tol = E2E_TOL[TD.CASES[name]["D"]]
    bad = []
    for k in ref:
        d = BT.e2e_distance(got[k].reshape(ref[k].shape), ref[k])
        if k in E2E[name]:
            print(f"{name} {k}: {d:.3g} from the float64 restated oracle, tolerance {tol[k][0]:.3g}")
            if not within(got[k], ref[k], tol[k][0]):
                bad.append(k)
        else:
            print(f"{name} {k}: {d:.3g} from the float64 restated oracle (not asserted)")
    assert bad == []
