"""tests/bf16_tower.py (the bf16 MLP tower's operand rounding restated) by itself, no GPU, and
the premises of the GPU tests that use it (tests/test_gpu_bf16.py):

* ``bf`` is round-to-nearest-even, bit for bit against a scalar transcription;
* ``bf16_linear``'s backward is the three written-out products; the oracle's ``linear=`` leaves
  the default bit for bit alone and reaches the tower's three Linears only;
* the layer-by-layer checker accepts the CPU's fp32 evaluation of the same formulas within a
  quarter of every bound, and rejects every wrong variant in every single layer (at checks of
  that layer only), the other form of the weight gradients, and the masks of seed + 1;
* end to end: the fp32 restated oracle stays inside the tolerance's caps, and every asserted
  quantity separates every wrong variant that changes it, and the unrounded oracle, by 4 x.
"""
import pytest
import torch

from oracle import ncf_oracle as O
from tests import bf16_tower as BT


@pytest.fixture(autouse=True)
def one_thread():
    """torch's threaded CPU reductions do not fix their order (test_gpu_fullsize)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ----------------------------------------------------------------------------- bf
def _rne_bits(b):
    """fp32 bits -> bf16 bits, nearest even, in Python integers (finite inputs): add half of the
    dropped field, less one when the kept field is even, and drop the field."""
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


BITS = [
    0x00000000, 0x80000000,             # +0, -0
    0x3F808000, 0x3F818000,             # ties: 1 + 2^-8 -> 1 (even below), 1 + 3 2^-8 -> 1 + 2^-6
    0xBF808000, 0xBF818000,             # the same, negative
    0x3F808001, 0x3F807FFF,             # just above / below a tie
    0x3FFF8000, 0x3FFFFFFF, 0x3FFF7FFF,  # carry into the exponent: -> 2.0, 2.0; not: 1.9921875
    0x7F7F0000, 0x7F7F7FFF,             # the largest finite bf16, and the last value that stays finite
    0x7F7F8000, 0x7F7FFFFF,             # a tie / the largest fp32: nearest even is infinity
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF,   # fp32 denormals
    0x3DCCCCCD, 0x40490FDB, 0xC2F6E979,  # 0.1, pi, -123.456
]


def test_bf_is_round_to_nearest_even_bit_for_bit():
    assert [_rne_bits(b) for b in (0x3F808000, 0x3F818000, 0x3FFF8000, 0x7F7F8000, 0x80000000)] == \
        [0x3F80, 0x3F82, 0x4000, 0x7F80, 0x8000]
    g = torch.Generator().manual_seed(0)
    bits = BITS + torch.randint(0, 0x7F800000, (4000,), generator=g).tolist()
    bits += [b | 0x80000000 for b in bits[len(BITS):len(BITS) + 2000]]
    x = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits],
                     dtype=torch.int32).view(torch.float32)
    want = [_rne_bits(b) << 16 for b in bits]
    for dtype in (torch.float32, torch.float64):
        got = BT.bf(x.to(dtype))
        assert got.dtype == dtype
        gb = (got.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).tolist()
        assert gb == want
    # the wrong convert differs: it never rounds up in magnitude
    tb = (BT.bf_trunc(x).view(torch.int32).to(torch.int64) & 0xFFFFFFFF).tolist()
    assert tb == [b & 0xFFFF0000 for b in bits]
    assert sum(a != b for a, b in zip(tb, want)) > 1000


# ----------------------------------------------------------------------------- bf16_linear
@pytest.mark.parametrize("variant", [None] + list(BT.VARIANTS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_bf16_linear_backward_is_the_three_products(variant, dtype):
    """torch.autograd.gradcheck does not apply: the function is piecewise constant in its
    rounded operands (its true derivative in x and w is 0 almost everywhere); the backward is
    the kernels' definition, checked against the products written out."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 12, generator=g).to(dtype).requires_grad_(True)
    w = (torch.randn(5, 12, generator=g) * 0.3).to(dtype).requires_grad_(True)
    b = torch.randn(5, generator=g).to(dtype).requires_grad_(True)
    dy = (torch.randn(7, 5, generator=g) * 1e-3).to(dtype)
    rd = BT.rounding(variant)
    y = BT.make_linear(variant)(x, w, b)
    assert y.dtype == dtype
    assert torch.equal(y.detach(), rd.fx(x.detach()) @ rd.fw(w.detach()).t() + b.detach())
    y.backward(dy)
    xd, wd = x.detach(), w.detach()
    assert torch.equal(x.grad, rd.bdy(dy) @ rd.bw(wd))
    assert torch.equal(w.grad, rd.wdy(dy).t() @ rd.wx(xd))
    assert torch.equal(b.grad, dy.sum(0))
    if variant is None:     # every operand is a bf16 value; the plain products differ
        for t in (BT.bf(xd), BT.bf(wd), BT.bf(dy)):
            assert torch.equal(t.float().to(torch.bfloat16).to(dtype), t)
        assert not torch.equal(x.grad, dy @ wd) and not torch.equal(w.grad, dy.t() @ xd)


def _tiny_step(linear=None, dtype=torch.float64):
    from tests import test_gpu_bf16 as TB
    from tests import test_gpu_dropout as TD
    c, init, (u, i, t), seed = TB.tower_case("bf16mm_lw_b1_p02")
    p = TD.cast_state(init, dtype)
    masks = TD.torch_masks(seed, c["B"], c["H"], c["M"], c["p"], dtype)
    kw = {} if linear is None else {"linear": linear}
    return O.train_step(p, O.AdamState(lr=TD.LR, weight_decay=TD.WD), u, i, t.to(dtype),
                        negative_samples=c["M"] - 1, num_heads=c["H"], temporal_dim=TD.TDIM,
                        n_layers=3, dropout_masks=masks, **kw), p


def test_oracle_linear_argument_reaches_the_tower_only():
    (p0, l0, g0), q0 = _tiny_step()
    (p1, l1, g1), q1 = _tiny_step(O.linear)
    assert torch.equal(p0, p1) and torch.equal(l0, l1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0) and all(torch.equal(q0[k], q1[k]) for k in q0)
    # the unrounded Function is the same function: its hand-written backward is autograd's
    (p2, l2, g2), _ = _tiny_step(BT.make_linear(BT.UNROUNDED))
    torch.testing.assert_close(p2, p0, rtol=1e-13, atol=0)
    for k in g0:
        torch.testing.assert_close(g2[k], g0[k], rtol=1e-10, atol=1e-18, msg=k)
    # a Linear outside the tower never sees the argument
    seen = []

    def spy(x, w, b):
        seen.append(tuple(w.shape))
        return O.linear(x, w, b)
    _tiny_step(spy)
    assert seen == [(256, 96), (128, 256), (64, 128)]
    # rounded, the step is another one
    (p3, _, g3), _ = _tiny_step(BT.bf16_linear)
    assert (p3 - p0).abs().max() > 1e-5 and not torch.equal(g3["mlp.4.weight"], g0["mlp.4.weight"])


# ----------------------------------------------------------------------------- layer by layer
def _lw_cases():
    from tests import test_gpu_bf16 as TB
    return list(TB.LW_CASES)


@pytest.mark.parametrize("name", _lw_cases())
def test_layer_checker_accepts_fp32_and_rejects_wrong_roundings(name):
    from tests import test_gpu_bf16 as TB
    from tests import test_gpu_dropout as TD
    # accepted: the fp32 evaluation, with the weight gradients in either form, within a quarter
    for (wgrad, rd), recorded in zip((("fp32", BT.VARIANTS["dw_unrounded"]), ("bf16", BT.RNE)),
                                     TB.LW_CASES[name]):
        T, init, t, seed = TB.cpu_tower(name, rd)
        checks = TB.check_tower(name, T, init, t, seed, wgrad)
        assert {c.name for c in checks} >= {"r0", "r1", "r2", "a2", "prob", "dlin0", "dlin2", "dy",
                                            "mlp.0.weight", "mlp.4.bias", "mlp.10.weight"}
        worst = BT.report(checks, f"{name} ({wgrad} weight gradients)")
        assert BT.failures(checks, 0.25) == []
        # the figures beside the case are these, measured
        assert worst[0] <= recorded[0] * 1.05 and worst[1] <= recorded[1] * 1.05, (worst, recorded)
    rne = TB.cpu_tower(name)
    # the other form of the weight gradients is rejected, at the weight gradients
    assert set(BT.failures(TB.check_tower(name, *rne, "fp32"))) == \
        {"mlp.0.weight", "mlp.4.weight", "mlp.8.weight"}
    T, init, t, seed = TB.cpu_tower(name, BT.VARIANTS["dw_unrounded"])
    assert set(BT.failures(TB.check_tower(name, T, init, t, seed, "bf16"))) == \
        {"mlp.0.weight", "mlp.4.weight", "mlp.8.weight"}
    # every wrong variant, in one layer at a time, fails, and only at checks of that layer
    for variant, rd in BT.VARIANTS.items():
        for l in range(3):
            T, init, t, seed = TB.cpu_tower(name, rd, layers=(l,))
            checks = TB.check_tower(name, T, init, t, seed, "bf16")
            bad = [c for c in checks if c.name in BT.failures(checks)]
            assert bad, (variant, l)
            assert all(c.layer == l for c in bad), (variant, l, [c.name for c in bad])
            worst = max(BT.fractions(c)[0] for c in bad)
            assert worst > 16, (variant, l, worst)      # far outside, not marginally
            if variant != "dw_unrounded" and variant != "bwd_unrounded":
                assert f"r{l}" in [c.name for c in bad], (variant, l)
    # the masks of another seed
    if TD.CASES[name]["p"] > 0:
        bad = BT.failures(TB.check_tower(name, *rne[:3], seed + 1, "bf16"))
        assert {"a0", "a1", "a2", "dlin0", "dlin1", "dlin2"} <= set(bad)


def test_project_fp32_tolerances_alone_would_miss_wrong_roundings():
    """Why the derived bounds are there: at the project's fp32 tolerances (ISSUE_TOL) alone,
    unrounded weight gradients pass (0.03 to 0.14 of the tolerance on the 185- and 114-row
    cases), as do unrounded activations in layer 0's forward."""
    from tests import test_gpu_bf16 as TB
    T, init, t, seed = TB.cpu_tower("bf16mm_lw_d64_p02", BT.VARIANTS["dw_unrounded"])
    checks = TB.check_tower("bf16mm_lw_d64_p02", T, init, t, seed, "bf16")
    w = [BT.fractions(c) for c in checks if c.name in ("mlp.0.weight", "mlp.4.weight", "mlp.8.weight")]
    assert all(issue < 1 < tight for tight, issue in w)


# ----------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["bf16mm_e2e_small", "bf16mm_e2e_80", "bf16mm_e2e_d128"])
def test_end_to_end_premises(name):
    from tests import test_gpu_bf16 as TB
    from tests import test_gpu_dropout as TD
    c = TD.CASES[name]
    assert c["data_seed"] in TB.E2E_SEEDS[c["D"]]
    worst = TB.e2e_fp32_distances(name)
    tol = {k: v[0] for k, v in TB.E2E_TOL[c["D"]].items()}
    assert set(TB.E2E[name]) <= set(tol)
    # the recorded tolerance is 4 x the worst fp32 distance (recorded rounded up to 3 digits),
    # and the fp32 evaluation stays inside both caps of every asserted quantity at a quarter
    for k, (t4, w) in TB.E2E_TOL[c["D"]].items():
        assert 4 * worst[k] <= t4 <= 4 * w * 1.01, (k, worst[k], t4, w)
    for s in TB.E2E_SEEDS[c["D"]]:
        ref = TB.e2e_quantities(name, s, torch.float64, BT.bf16_linear)
        f32 = TB.e2e_quantities(name, s, torch.float32, BT.bf16_linear)
        for k in TB.E2E[name]:
            assert TB.within(f32[k], ref[k], tol[k] / 4), (s, k)
    # separation at the case's data seed
    ref = TB.e2e_quantities(name, c["data_seed"], torch.float64, BT.bf16_linear)
    assert set(TB.E2E[name]) <= set(ref)
    rejected_by = {}
    for variant in list(BT.VARIANTS) + ["unrounded"]:
        rd = BT.UNROUNDED if variant == "unrounded" else BT.VARIANTS[variant]
        wrong = TB.e2e_quantities(name, c["data_seed"], torch.float64, BT.make_linear(rd))
        for k in TB.E2E[name]:
            d = BT.e2e_distance(wrong[k], ref[k])
            if d > 0:       # (a variant that leaves the quantity bit for bit alone is not wrong there)
                assert d >= 4 * tol[k], (variant, k, d / tol[k])
                assert not TB.within(wrong[k], ref[k], tol[k]), (variant, k)
                rejected_by.setdefault(variant, []).append(k)
    # every wrong rounding but one is rejected by some asserted quantity; unrounded weight
    # gradients change the three tower weight gradients only, which are not asserted end to end
    # (0.6 to 1.4 tolerances away): the layer-by-layer test holds them
    assert set(rejected_by) == set(BT.VARIANTS) - {"dw_unrounded"} | {"unrounded"}
    for k in ("mlp.0.weight", "mlp.4.weight", "mlp.8.weight"):
        assert k not in TB.E2E[name]
    for k, fig in TB.E2E[name].items():
        print(f"{name} {k}: fp32 {worst[k]:.3g}, tolerance {tol[k]:.3g}, recorded nearest wrong {fig}")
