"""The opt-in backward of forward_simple(user_ids, product_ids, hour) on the MI355X
(``model.hour_backward = True``; hour_bwd.hip).

Gradients are held to |d| <= 1e-6 + 1e-4 |ref| against float64 autograd through
oracle.forward_simple_hour (tests/hour_cases.py; tests/test_hour_bwd_golden.py holds that oracle to
F11, the reference's own gradients, on the CPU).  The reduction's own sums are held to the
summation bound of their length: k fp32 additions of terms x_i err by at most k u sum|x_i|,
u = 2^-24."""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O
from tests import hour_cases as C
from tests.parity import assert_params_close, zone_from_grads

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import _lib, ops, optim, tapes  # noqa: E402

DEV = torch.device("cuda:0")
F = 0.3


def model_from(sd, U, I, D, T, hid, H, dropout=0.0):
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, T, hid, H, dropout, 4)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    m.hour_backward = True
    return m


def rand_case(U, I, D, T, hid, H, n, seed, hours=(0, 3, 23)):
    torch.manual_seed(seed)
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, T, hid, H, 0.0, 4)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for k in ("mf_norm", "mlp_norm"):         # (LayerNorms off their identity init)
        sd[k + ".weight"] = 1 + 0.2 * torch.randn(D, generator=g)
        sd[k + ".bias"] = 0.1 * torch.randn(D, generator=g)
    c = dict(U=U, I=I, D=D, T=T, hid=list(hid), H=H, n=n, sd=sd,
             u=torch.randint(0, U, (n,), generator=g), p=torch.randint(0, I, (n,), generator=g),
             hour=torch.tensor(hours)[torch.randint(0, len(hours), (n,), generator=g)],
             targets=(torch.rand(n, generator=g) < 0.4).float(), proj=None)
    if T != D:
        c["proj"] = (0.2 * torch.randn(D, T, generator=g), 0.1 * torch.randn(D, generator=g))
    return c


def f11_case(tag):
    c = C.case(tag)
    t = C.T_({k: c[k] for k in ("u", "p", "hour", "targets")})
    c.update(t, sd=C.T_(C.sub(c, "sd/")), proj=None)
    if "proj_w" in c:
        c["proj"] = (torch.from_numpy(c["proj_w"]), torch.from_numpy(c["proj_b"]))
    return c


def build(c, dropout=0.0):
    return model_from(c["sd"], c["U"], c["I"], c["D"], c["T"], c["hid"], c["H"], dropout)


def collect(m, accumulate=False):
    m.engine.materialize_table_grads(accumulate=accumulate)
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


def call(m, c, projection="case", seed=None, via_model=False):
    u, p, h = (c[k].to(DEV) for k in ("u", "p", "hour"))
    if via_model:
        return m.forward_simple(u, p, h)
    proj = c["proj"] if projection == "case" else projection
    return ops.forward_simple_hour(m, u, p, h, projection=proj, seed=seed)


def bce(out, c):
    return torch.nn.functional.binary_cross_entropy(out, c["targets"].to(DEV))


def check_against_oracle(c, got, ref, D):
    for name, g in ref.items():
        if name in ("proj_w", "proj_b"):
            continue
        if g is None:
            assert name not in got, f"{name}: a gradient where the reference leaves none"
            continue
        assert name in got, f"{name}: no gradient"
        C.assert_grad_close(name, got[name].numpy(), g.numpy())
    for nm in ("q_proj", "k_proj"):           # zero TENSORS, as autograd gives the reference
        for t in ("weight", "bias"):
            assert not got[f"user_product_attention.{nm}.{t}"].any()
    assert got["mlp.0.weight"][:, D:].abs().max() > 1e-5
    gh = got[C.HOUR_W]
    absent = sorted(set(range(24)) - set(c["hour"].tolist()))
    assert gh.shape == (24, c["T"]) and not gh[absent].any()
    assert all(gh[h].abs().sum() > 0 for h in set(c["hour"].tolist()))
    for n_ in got:
        assert not n_.startswith(C.UNTOUCHED), n_


# ----------------------------------------------------------------------------- 1. parity
CASES = {"d128": dict(U=6, I=5, D=128, T=32, hid=[64], H=8, n=5, seed=128)}


@pytest.mark.parametrize("tag", C.CASES + ["d128"])
def test_gradients_vs_float64_oracle(tag):
    c = f11_case(tag) if tag in C.CASES else rand_case(**CASES[tag])
    m = build(c)
    via_model = c["T"] == c["D"]              # (T != D: the module call draws its own projection)
    out = call(m, c, via_model=via_model)
    assert out.shape == (c["n"],) and out.requires_grad
    bce(out, c).backward()
    got = collect(m)
    ref_out, ref = C.oracle_grads(c["sd"], c["u"], c["p"], c["hour"], c["targets"], c["proj"],
                                  c["H"], len(c["hid"]))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.numpy(), atol=2e-6, rtol=0)
    if "out" in c:
        np.testing.assert_allclose(out.detach().cpu().numpy(), c["out"], atol=2e-6, rtol=0)
    check_against_oracle(c, got, ref, c["D"])
    # the dense gradients are views of the flat buffer; the no-grad call is untouched
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in m.engine.grad_views())
    with torch.no_grad():
        again = call(m, c, via_model=via_model)
    assert not again.requires_grad
    np.testing.assert_allclose(again.cpu().numpy(), out.detach().cpu().numpy(), atol=2e-6, rtol=0)


# ----------------------------------------------------------------------------- 2. dropout
def test_dropout_forward_equals_nograd_and_gradients_vs_oracle():
    c = f11_case("h64_32")
    m = build(c, dropout=0.25)
    n, H, D, hid = c["n"], c["H"], c["D"], c["hid"]
    seed = 12345

    def keep(cols, group, sd_):
        s_ = torch.empty(n, cols // group, device=DEV)
        o_ = torch.empty(n, cols, device=DEV)
        x_ = torch.ones(n, cols, device=DEV)
        _lib.call("ncf_dropout_rows", x_.data_ptr(), n, cols, group, 0.25, sd_, o_.data_ptr(),
                  s_.data_ptr(), _lib.stream_ptr(DEV))
        return s_.cpu()
    with torch.no_grad():
        plain = call(m, c, seed=seed)
        other = call(m, c, seed=seed + 1)
    out = call(m, c, seed=seed)
    assert out.requires_grad
    np.testing.assert_allclose(out.detach().cpu().numpy(), plain.cpu().numpy(), atol=2e-6, rtol=0)
    assert not torch.equal(other, out.detach())
    bce(out, c).backward()
    got = collect(m)
    sa = keep(D, D // H, seed).view(n, H, 1, 1)
    ms = [keep(w_, 1, (seed + 0x9E37 * (l + 1)) & (2 ** 63 - 1)) for l, w_ in enumerate(hid)]
    assert (sa == 0).any() and (sa > 1).any()
    ref_out, ref = C.oracle_grads(c["sd"], c["u"], c["p"], c["hour"], c["targets"], c["proj"], H,
                                  len(hid), attn_drop=sa, mlp_masks=ms)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.numpy(), atol=2e-6, rtol=0)
    check_against_oracle(c, got, ref, D)


def test_dropout_under_a_bound_optimizer_step_clock():
    """Once torch.optim.Adam is bound, the tower's dropout stream is offset by the device step
    clock's per-step seed (the attention's single-key dropout is not, as in the no-grad call): the
    forward still equals the no-grad call of the same seed and the gradients the float64 oracle's
    with the kernels' own keep-scales."""
    c = f11_case("h64_32")
    m = build(c, dropout=0.25)
    n, H, D, hid = c["n"], c["H"], c["D"], c["hid"]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    opt.zero_grad()
    bce(call(m, c, seed=7), c).backward()
    opt.step()
    assert m.engine.clock is not None
    clock_seed = int(m.engine.clock.cpu()[1].item()) % 2 ** 64
    seed = 4242

    def keep(cols, group, sd_):
        s_ = torch.empty(n, cols // group, device=DEV)
        o_ = torch.empty(n, cols, device=DEV)
        x_ = torch.ones(n, cols, device=DEV)
        _lib.call("ncf_dropout_rows", x_.data_ptr(), n, cols, group, 0.25, sd_, o_.data_ptr(),
                  s_.data_ptr(), _lib.stream_ptr(DEV))
        return s_.cpu()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        plain = call(m, c, seed=seed)
    opt.zero_grad()
    out = call(m, c, seed=seed)
    np.testing.assert_allclose(out.detach().cpu().numpy(), plain.cpu().numpy(), atol=2e-6, rtol=0)
    bce(out, c).backward()
    got = collect(m)
    sa = keep(D, D // H, seed).view(n, H, 1, 1)
    ms = [keep(w_, 1, (((seed + 0x9E37 * (l + 1)) & (2 ** 63 - 1)) + clock_seed) % 2 ** 64)
          for l, w_ in enumerate(hid)]
    ref_out, ref = C.oracle_grads(sd, c["u"], c["p"], c["hour"], c["targets"], c["proj"], H,
                                  len(hid), attn_drop=sa, mlp_masks=ms)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.numpy(), atol=2e-6, rtol=0)
    check_against_oracle(c, got, ref, D)


# ----------------------------------------------------------------------------- 3. s = 0
def test_scale_factor_at_zero():
    """T == D = 16, one hour_embed row at -1/0.3 in half its columns: s = 1 + 0.3 tp is 0 or about
    1e-8 there.  Nothing may divide by it: every gradient finite and within tolerance."""
    c = rand_case(U=9, I=7, D=16, T=16, hid=[32, 16], H=2, n=29, seed=160, hours=(4, 4, 9))
    hw = c["sd"][C.HOUR_W]
    hw[4, ::2] = -1.0 / 0.3
    s = 1 + np.float32(0.3) * hw[4, ::2].numpy()
    assert np.abs(s).max() < 1e-6
    m = build(c)
    out = call(m, c, via_model=True)
    bce(out, c).backward()
    got = collect(m)
    assert all(torch.isfinite(g).all() for g in got.values())
    _, ref = C.oracle_grads(c["sd"], c["u"], c["p"], c["hour"], c["targets"], None, c["H"], 2)
    check_against_oracle(c, got, ref, 16)


# ----------------------------------------------------------------------------- 4. the kernels
def hour_grad(hour, dte, add=None):
    n, T = hour.numel(), dte.shape[1] - 8
    out = torch.full((24, T), float("nan"), device=DEV)
    ws = torch.empty(max(1, _lib.query("ncf_hour_grad_workspace", n, T)), device=DEV)
    _lib.call("ncf_hour_grad", hour.data_ptr(), n, dte.data_ptr() + 32, dte.shape[1],
              None if add is None else add.data_ptr(), T, T, out.data_ptr(), ws.data_ptr(),
              ws.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("T", [8, 32, 96])
def test_hour_grad_reduction_shapes(T):
    chunk = ops.HOUR_GRAD_CHUNK
    assert chunk == _lib.query("ncf_hour_grad_chunk")
    g = torch.Generator().manual_seed(T)
    shapes = {"one_row": torch.tensor([7]),
              "one_hour": torch.full((chunk + 3,), 11),
              "ends": torch.tensor([0, 23, 23, 0, 0]),
              "ragged": torch.randint(0, 24, (2 * chunk + 5,), generator=g) % 7 * 3}
    for name, hour in shapes.items():
        n = hour.numel()
        dte = torch.randn(n, T + 8, generator=g)       # (read in place: columns 8.., ld = T + 8)
        add = torch.randn(n, T, generator=g) if name in ("ragged", "ends") else None
        a = hour_grad(hour.to(DEV), dte.to(DEV), None if add is None else add.to(DEV))
        b = hour_grad(hour.to(DEV), dte.to(DEV), None if add is None else add.to(DEV))
        assert torch.equal(a, b), name                  # deterministic: bitwise
        terms = dte[:, 8:].double() + (0 if add is None else add.double())
        mag = dte[:, 8:].double().abs() + (0 if add is None else add.double().abs())
        ref = torch.zeros(24, T, dtype=torch.float64).index_add_(0, hour, terms)
        cnt = torch.bincount(hour, minlength=24).double()[:, None]
        bound = (cnt + 1) * 2.0 ** -24 * torch.zeros(24, T, dtype=torch.float64).index_add_(0, hour, mag)
        assert ((a.double() - ref).abs() <= bound).all(), name
        absent = cnt[:, 0] == 0
        assert absent.any() and not a[absent].any() and torch.isfinite(a).all(), name
        if name == "ragged":
            # the rows of one hour reordered among themselves: every other hour bitwise unchanged
            h0 = int(hour[0])
            idx = (hour == h0).nonzero().flatten()
            perm = torch.arange(n)
            perm[idx] = idx.flip(0)
            assert len(idx) > 2 * 3
            c_ = hour_grad(hour[perm].to(DEV), dte[perm].to(DEV), add[perm].to(DEV))
            keep = torch.arange(24) != h0
            assert torch.equal(c_[keep], a[keep])
            assert ((c_[h0].double() - ref[h0]).abs() <= bound[h0]).all()


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_item_scale_bwd_vs_float64_and_bad_id(D):
    """g *= s in place, dtp = f (g_mf y + g_mlp z) with y, z recomputed from the table rows; an
    out-of-range id reads row 0 and raises the flag, as the gather does."""
    g = torch.Generator().manual_seed(D)
    I, n = 9, 37
    tm, tl = torch.randn(I, D, generator=g), torch.randn(I, D, generator=g)
    gam = [1 + 0.2 * torch.randn(D, generator=g) for _ in range(2)]
    bet = [0.1 * torch.randn(D, generator=g) for _ in range(2)]
    tp = torch.randn(n, D, generator=g)
    tp[3, :5] = -1.0 / 0.3
    ga, gb = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
    ids = torch.randint(0, I, (n,), generator=g)
    for bad in (False, True):
        if bad:
            ids = ids.clone()
            ids[5], ids[6] = I, -1
        d = [t.to(DEV).contiguous() for t in (ids, tm, tl, gam[0], bet[0], gam[1], bet[1], tp,
                                               ga.clone(), gb.clone())]
        dtp = torch.full((n, D), float("nan"), device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.call("ncf_item_scale_bwd", d[0].data_ptr(), n, d[1].data_ptr(), d[2].data_ptr(), I, D,
                  d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), 1e-5,
                  d[7].data_ptr(), F, d[8].data_ptr(), d[9].data_ptr(), dtp.data_ptr(),
                  err.data_ptr(), _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert int(err.item()) == int(bad)
        safe = torch.where((ids < 0) | (ids >= I), torch.zeros_like(ids), ids)
        y = O.layer_norm(tm.double()[safe], gam[0].double(), bet[0].double())
        z = O.layer_norm(tl.double()[safe], gam[1].double(), bet[1].double())
        s = 1 + 0.3 * tp.double()
        C.assert_grad_close("g_imf", d[8].cpu().numpy(), (ga.double() * s).numpy())
        C.assert_grad_close("g_xi", d[9].cpu().numpy(), (gb.double() * s).numpy())
        # (two products of magnitude up to ~10 summed: the bound's rtol on each product)
        ref = 0.3 * (ga.double() * y + gb.double() * z)
        mag = 0.3 * ((ga.double() * y).abs() + (gb.double() * z).abs())
        assert ((dtp.cpu().double() - ref).abs() <= 1e-6 + 1e-4 * mag).all()


# ----------------------------------------------------------------------------- 5. projection
def test_projection_gradients():
    c = f11_case("h16_8")
    m = build(c)
    lin = torch.nn.Linear(c["T"], c["D"]).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(c["proj"][0])
        lin.bias.copy_(c["proj"][1])
    out = call(m, c, projection=lin)
    bce(out, c).backward()
    got = collect(m)
    _, ref = C.oracle_grads(c["sd"], c["u"], c["p"], c["hour"], c["targets"], c["proj"], c["H"], 2)
    C.assert_grad_close("proj_w", lin.weight.grad.cpu().numpy(), ref["proj_w"].numpy())
    C.assert_grad_close("proj_b", lin.bias.grad.cpu().numpy(), ref["proj_b"].numpy())
    check_against_oracle(c, got, ref, c["D"])
    # a second backward adds to the projection's gradient too
    w1 = lin.weight.grad.clone()
    bce(call(m, c, projection=lin), c).backward()
    C.assert_grad_close("proj_w x2", lin.weight.grad.cpu().numpy(), (2 * w1).cpu().numpy())
    # a tuple is a constant: the call runs and leaves nothing behind
    m.zero_grad(set_to_none=True)
    pw, pb = (t.to(DEV) for t in c["proj"])
    bce(call(m, c, projection=(pw, pb)), c).backward()
    assert pw.grad is None and pb.grad is None and not pw.requires_grad
    C.assert_grad_close(C.HOUR_W, collect(m)[C.HOUR_W].numpy(), ref[C.HOUR_W].numpy())


# ----------------------------------------------------------------------------- 6. accumulation
def test_two_backwards_accumulate():
    a = rand_case(U=9, I=7, D=32, T=32, hid=[64, 32], H=4, n=41, seed=61)
    b = dict(a, **{k: v for k, v in rand_case(U=9, I=7, D=32, T=32, hid=[64, 32], H=4, n=41,
                                              seed=62, hours=(3, 8, 23)).items()
                   if k in ("u", "p", "hour", "targets")})
    m = build(a)
    single = []
    for c in (a, b):
        m.zero_grad(set_to_none=True)
        bce(call(m, c, via_model=True), c).backward()
        single.append(collect(m))
    m.zero_grad(set_to_none=True)
    for c in (a, b):
        bce(call(m, c, via_model=True), c).backward()
    both = collect(m, accumulate=True)
    assert set(both) == set(single[0]) and C.HOUR_W in both
    for k in both:
        C.assert_grad_close(k, both[k].numpy(), (single[0][k].double() + single[1][k].double()).numpy())
    assert both[C.HOUR_W][[0, 8]].abs().sum(1).min() > 0       # (an hour of each batch alone)


# ----------------------------------------------------------------------------- 7. optimizer
def test_three_adam_steps_vs_float64():
    c = rand_case(U=40, I=30, D=64, T=32, hid=[256, 128, 64], H=4, n=70, seed=70, hours=(1, 5, 22))
    m = build(c)
    lr, wd = 1e-3, 1e-5
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=wd)
    p64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in c["sd"].items()}
    oopt = O.AdamState(lr=lr, weight_decay=wd)
    gen = torch.Generator().manual_seed(71)
    zones = {}
    hw = m.temporal_encoding.hour_embed.weight
    for step in range(3):
        u = torch.randint(0, c["U"], (c["n"],), generator=gen)
        p = torch.randint(0, c["I"], (c["n"],), generator=gen)
        h = torch.tensor([1, 5, 22])[torch.randint(0, 3, (c["n"],), generator=gen)]
        t = (torch.rand(c["n"], generator=gen) < 0.4).float()
        out = ops.forward_simple_hour(m, u.to(DEV), p.to(DEV), h.to(DEV), projection=c["proj"])
        loss = torch.nn.functional.binary_cross_entropy(out, t.to(DEV))
        opt.zero_grad()
        loss.backward()
        assert hw.grad is not None and m.engine.pending is not None
        opt.step()
        _, grads = C.oracle_grads(p64, u, p, h, t, c["proj"], c["H"], 3)
        grads = {k: v for k, v in grads.items() if k not in ("proj_w", "proj_b")}
        for k, v in grads.items():
            if v is not None:
                zones.setdefault(k, []).append(zone_from_grads(v.numpy(), p64[k].numpy(), wd))
        with torch.no_grad():
            oopt.step(p64, grads)
    sd = m.state_dict()
    assert C.HOUR_W in zones and "mlp.0.weight" in zones
    for k, zs in zones.items():
        assert_params_close(k, sd[k].cpu().numpy(), p64[k].numpy(), zs, lr)
    for k in sd:                                  # what got no gradient did not move
        if k.startswith(C.UNTOUCHED):
            assert torch.equal(sd[k].cpu(), c["sd"][k]), k
    b = optim.binding_of(opt, m)
    assert b is not None and b.D is not None and b.uniform
    assert opt.state[m.mlp[0].weight]["step"] is b.step_t and float(b.step_t) == 3
    assert float(opt.state[hw]["step"]) == 3 and id(hw) not in b._all_ids


# ----------------------------------------------------------------------------- 8. tapes
def _interleaved(monkeypatch, enabled):
    monkeypatch.setattr(tapes, "ENABLED", enabled)
    c = rand_case(U=50, I=40, D=32, T=32, hid=[64, 32], H=4, n=48, seed=80)
    m = build(c)
    D = c["D"]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    u, p = c["u"].to(DEV), c["p"].to(DEV)
    tp = m.engine.tapes
    info = {}

    def plain():
        loss = torch.nn.functional.binary_cross_entropy(m.forward_simple(u, p), c["targets"].to(DEV))
        opt.zero_grad()
        loss.backward()
    for _ in range(5):            # (tapes record once the geometry has come round)
        plain()
        opt.step()
    info["recorded"], r0 = tp.recorded, tp.replays
    out = call(m, c, via_model=True)
    opt.zero_grad()
    bce(out, c).backward()
    assert m.mlp[0].weight.grad[:, D:].abs().max() > 0
    opt.step()
    info["hour_replays"] = tp.replays - r0
    plain()
    torch.cuda.synchronize()
    info["temporal_cols_zero"] = not m.mlp[0].weight.grad[:, D:].any().item()
    opt.step()
    plain()
    opt.step()
    info["replays"] = tp.replays
    return {k: v.cpu().clone() for k, v in m.state_dict().items()}, info


def test_interleaved_with_plain_steps_and_tapes(monkeypatch):
    on, i_on = _interleaved(monkeypatch, True)
    off, i_off = _interleaved(monkeypatch, False)
    assert i_on["recorded"] > 0 and i_off["recorded"] == 0 and i_off["replays"] == 0
    assert i_on["hour_replays"] == 0
    assert i_on["temporal_cols_zero"] and i_off["temporal_cols_zero"]
    for k in on:
        assert torch.equal(on[k], off[k]), k


# ----------------------------------------------------------------------------- 9. refusals
def test_refusals_and_plain_backward_after_hour():
    c = rand_case(U=9, I=7, D=16, T=16, hid=[32, 16], H=2, n=11, seed=90)
    m = build(c)
    m.hour_backward = False
    with pytest.raises(NotImplementedError, match="hour_backward"):
        call(m, c, via_model=True)
    del m.hour_backward
    with pytest.raises(NotImplementedError, match="hour_backward"):
        call(m, c, via_model=True)
    m.hour_backward = True
    bad = dict(c, hour=c["hour"].clone())
    bad["hour"][2] = 24
    with pytest.raises(IndexError):
        call(m, bad, via_model=True)
    assert m.engine.pending is None
    # the zeroed-once cache: a plain backward after an hour backward finds the columns 0 again
    bce(call(m, c, via_model=True), c).backward()
    assert m.mlp[0].weight.grad[:, 16:].abs().max() > 0
    m.zero_grad(set_to_none=True)
    bce(m.forward_simple(c["u"].to(DEV), c["p"].to(DEV)), c).backward()
    assert not m.mlp[0].weight.grad[:, 16:].any()
    assert m.temporal_encoding.hour_embed.weight.grad is None
    # eval and no_grad calls are untouched by the switch
    m.eval()
    assert not call(m, c, via_model=True).requires_grad
    # split widths keep the reference's failure
    ms = ncf.AdvancedNCF(9, 7, 5, 24, 32, 16, 32, [32, 16], 2, 0.0, 4).to(DEV).train()
    ms.hour_backward = True
    with pytest.raises(RuntimeError):
        ms.forward_simple(c["u"].to(DEV), c["p"].to(DEV), c["hour"].to(DEV))
