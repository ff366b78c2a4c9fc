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

Out of scope here: BF16_MM = True (the tower's Linears on bf16 MFMA) stays pinned by the
100-step track and by its bitwise tests.  A faithful reference for it needs the operand rounding
restated in the oracle's forward and in its backward, a piece of work of its own.
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
