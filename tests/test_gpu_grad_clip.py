"""Global gradient-norm clipping over the compact table gradients and the dense gradients
(ncf_amd.clip_grad_norm_, FusedTrainStep(max_grad_norm=), ModelTrainer(clip_gradients=);
csrc/grad_clip.hip).  MI355X only.

References are float64, computed here from snapshots of the gradients.  Tolerances: the returned
norm to relative 1e-6 (fp64 accumulation leaves the fp32 rounding of the result, 6e-8; the rest is
margin); every scaled element to relative 2^-21 (two fp32 roundings: the coefficient and the
product); Adam's first moment to rel 1e-5 / abs 1e-9."""
import math

import pytest
import torch

import _ncf_pkg

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import _lib, clip, ops, optim, tapes  # noqa: E402

DEV = torch.device("cuda:0")
M = 5
KEYS = ("mf_user", "mlp_user", "mf_item", "mlp_item")
SMALL = dict(U=301, I=97, B=8)
LARGE = dict(U=3000, I=700, B=4096)      # several chunks per segment, count far below capacity
REL_NORM, REL_ELEM = 1e-6, 2.0 ** -21
LR, WD, B1 = 1e-3, 1e-5, 0.9
# The multi-step runs must clip at EVERY step with max_norm at half the first step's norm.  At
# lr 1e-3 Adam's first two steps on this tiny problem cut the gradient norm ninefold (3.25, 1.64,
# 0.37 measured), so those runs take a small lr: the norms then stay near the first one.
LR_STEPS = 1e-5


def kjt(u, i):
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([u, i]),
        lengths=torch.ones(2 * u.numel(), dtype=torch.long, device=u.device))


def batch(U, I, B, seed=5):
    """B groups of M rows; a user and an item repeated so that num_unique < n."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, U, (B,), generator=g)
    u[1] = u[0]
    i = torch.randint(0, I, (B * M,), generator=g)
    i[7] = i[2]
    t = torch.zeros(B, M)
    t[:, 0] = 1
    return u.repeat_interleave(M).to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)


def batches(n, U, I, B, seed=5):
    return [batch(U, I, B, seed + 17 * s) for s in range(n)]


def model(U, I, D=64, Dm=None, seed=11, **_):
    torch.manual_seed(seed)
    H = 4 if D >= 32 else 2        # (the attention kernels take head dims 8 .. 64)
    return ncf.AdvancedNCF(U, I, 5, 24, Dm or D, D, 32, [256, 128, 64], H, 0.0, M - 1).to(DEV).train()


def backward(m, data):
    u, i, t = data
    torch.nn.BCELoss()(m(kjt(u, i)), t).backward()


def counts(w):
    """{key: valid rows of w.G[key]} (a host read)."""
    nu = w.num_unique.tolist()
    nm = w.split["num_unique"].tolist() if w.split is not None else nu
    return {k: (nm if k.startswith("mf") else nu)[0 if k.endswith("user") else 1] for k in KEYS}


def snapshot(m, poison=True):
    """(counts, {key: clone of w.G[key]}, clone of flat_grad) of the pending backward; rows of
    every G at and past its count are then filled with NaN."""
    eng = m.engine
    w = eng.pending
    assert w is not None
    cnt = counts(w)
    G = {k: w.G[k].clone() for k in KEYS}
    if poison:
        for k in KEYS:
            w.G[k][cnt[k]:] = float("nan")
    return cnt, G, eng.flat_grad.clone()


def norm64(tensors, inf=False):
    if inf:
        return max(float(t.double().abs().max()) for t in tensors if t.numel())
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in tensors))


def coef(N, max_norm):
    return min(1.0, max_norm / (N + 1e-6))


def assert_scaled(got, before, c, what):
    ref = before.double() * c
    err = (got.double() - ref).abs()
    assert bool((err <= REL_ELEM * ref.abs()).all()), (what, float((err / ref.abs().clamp_min(1e-300)).max()))


def assert_norm(total, N):
    v = float(total)
    assert math.isfinite(v) and abs(v - N) <= REL_NORM * N, (v, N)


# ----------------------------------------------------------------------------- 1. norm and scale
@pytest.mark.parametrize("cfg", [dict(SMALL), dict(SMALL, D=16), dict(SMALL, D=64, Dm=32),
                                 dict(LARGE), dict(SMALL, inf=True), dict(LARGE, inf=True)],
                         ids=["small", "d16", "split_widths", "large", "small_inf", "large_inf"])
def test_norm_and_scale_vs_float64(cfg):
    inf = cfg.pop("inf", False)
    nt = math.inf if inf else 2.0
    m = model(**cfg)
    backward(m, batch(cfg["U"], cfg["I"], cfg["B"]))
    n = cfg["B"] * M
    cnt, G, flat = snapshot(m)
    assert all(0 < cnt[k] < n for k in KEYS), cnt
    valid = [G[k][:cnt[k]] for k in KEYS] + [flat]
    N = norm64(valid, inf)
    max_norm = N / 2
    c = coef(N, max_norm)
    assert c < 1
    total = ncf.clip_grad_norm_(m.parameters(), max_norm, norm_type=nt)
    assert total.shape == () and total.dtype == torch.float32 and total.is_cuda
    assert_norm(total, N)
    w = m.engine.pending
    for k in KEYS:
        assert_scaled(w.G[k][:cnt[k]], G[k][:cnt[k]], c, k)
        assert bool(torch.isnan(w.G[k][cnt[k]:]).all()), k       # poisoned rows untouched
    assert_scaled(m.engine.flat_grad, flat, c, "flat_grad")
    # the dense .grad views are the scaled buffer, the tables still hold no dense .grad
    assert all(p.grad is None for p in m.engine.table_params().values())
    assert m.mlp[0].weight.grad.data_ptr() == m.engine.gptr("mlp.0.weight")


@pytest.mark.parametrize("kind", [0, 1])
def test_c_abi_scalar_path_empty_counts_and_many_chunks(kind):
    """ncf_grad_clip on hand-made segments: a [24, 7] tensor (odd width: scalar loads), a width-8
    segment at a base that is not 16-byte aligned (scalar), a [5000, 64] segment with 37 valid
    rows (chunks wholly past the count), one with a count of 0, one without a count spanning a
    ragged last chunk; rows past the counts hold NaN."""
    g = torch.Generator().manual_seed(3 + kind)
    chunk = _lib.query("ncf_grad_clip_chunk")
    raw = torch.randn(1 + 30 * 8, generator=g).to(DEV)
    shapes = [(24, 7, None), (30, 8, None), (5000, 64, 37), (50, 16, 0), (1, 2 * chunk + 5, None),
              (700, 32, 700)]
    tens, cnts = [], torch.tensor([c or 0 for _, _, c in shapes], dtype=torch.int32, device=DEV)
    for j, (r, d, c) in enumerate(shapes):
        t = raw[1:].view(30, 8) if j == 1 else torch.randn(r, d, generator=g).to(DEV)
        if c is not None:
            t[c:] = float("nan")
        tens.append(t)
    assert tens[1].data_ptr() % 16 == 4
    raw0 = float(raw[0])
    before = [t.clone() for t in tens]
    valid = [t if c is None else t[:c] for t, (_, _, c) in zip(before, shapes)]
    N = norm64(valid, kind == 1)
    c_ = coef(N, N / 3)
    segs = [(t, None if c is None else cnts.data_ptr() + 4 * j, r, d)
            for j, (t, (r, d, c)) in enumerate(zip(tens, shapes))]
    out = clip.run(segs, kind, N / 3, DEV)
    torch.cuda.synchronize()
    assert_norm(out[0], N)
    assert abs(float(out[1]) - c_) <= 2.0 ** -23 * c_
    for t, b, (_, _, c) in zip(tens, before, shapes):
        k = t.shape[0] if c is None else c
        assert_scaled(t[:k], b[:k], c_, tuple(t.shape))
        assert bool(torch.isnan(t[k:]).all())
    assert float(raw[0]) == raw0        # (the float in front of the misaligned segment)
    # the norm alone (max_norm = +inf) writes nothing; an empty list is norm 0, coefficient 1
    now = [t.clone() for t in tens]
    out2 = clip.run(segs, kind, math.inf, DEV)
    out0 = clip.run([], kind, 1.0, DEV)
    torch.cuda.synchronize()
    assert float(out2[1]) == 1.0 and out0.tolist() == [0.0, 1.0]
    assert_norm(out2[0], N * c_)
    for t, b in zip(tens, now):
        assert torch.equal(torch.nan_to_num(t, nan=7.0), torch.nan_to_num(b, nan=7.0))


# ----------------------------------------------------------------------------- 2. no-op
def test_noop_keeps_every_bit_and_grad_norm_matches():
    m = model(**SMALL)
    backward(m, batch(**SMALL))
    cnt, G, flat = snapshot(m)
    N = norm64([G[k][:cnt[k]] for k in KEYS] + [flat])
    gn = ncf.grad_norm(m.parameters())
    total = ncf.clip_grad_norm_(m.parameters(), 10 * N)
    assert_norm(total, N)
    assert torch.equal(gn, total) and gn.shape == ()
    w = m.engine.pending
    for k in KEYS:
        assert torch.equal(w.G[k][:cnt[k]], G[k][:cnt[k]]), k
    assert torch.equal(m.engine.flat_grad, flat)
    assert torch.equal(ncf.grad_norm(m), total)            # (the module itself as `parameters`)


# ----------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["small", "large"])
def test_identical_twins_give_identical_bits(cfg):
    runs = []
    data = batch(**cfg)
    for _ in range(2):
        m = model(**cfg)
        backward(m, data)
        cnt, G, flat = snapshot(m, poison=False)
        N = norm64([G[k][:cnt[k]] for k in KEYS] + [flat])
        total = ncf.clip_grad_norm_(m.parameters(), N / 2)
        w = m.engine.pending
        runs.append((total.clone(), [w.G[k][:cnt[k]].clone() for k in KEYS],
                     m.engine.flat_grad.clone()))
    (ta, Ga, fa), (tb, Gb, fb) = runs
    assert torch.equal(ta, tb)
    assert all(torch.equal(x, y) for x, y in zip(Ga, Gb)) and torch.equal(fa, fb)


# ----------------------------------------------------------------------------- 4. other sources
def _dense_reference(m):
    """{parameter: clone of its dense .grad} over every parameter that has one."""
    return {p: p.grad.clone() for p in m.parameters() if p.grad is not None}


def _check_dense(m, before, extra=()):
    N = norm64(list(before.values()))
    max_norm = N / 2
    c = coef(N, max_norm)
    total = ncf.clip_grad_norm_(list(m.parameters()) + list(extra), max_norm)
    assert_norm(total, N)
    assert m.engine.pending is None
    for p, g in before.items():
        assert_scaled(p.grad, g, c, tuple(p.shape))
    return c


def test_materialised_table_gradients():
    m = model(**SMALL)
    backward(m, batch(**SMALL))
    m.engine.materialize_table_grads()
    before = _dense_reference(m)
    assert all(p in before for p in m.engine.table_params().values())
    _check_dense(m, before)


def test_two_backwards_without_zero_grad():
    """The second backward leaves dense table .grad (the first one's) beside pending rows: the
    call sums them as the optimizer binding does.  Reference: a twin run the same way whose
    pending rows the test materialises itself."""
    d0, d1 = batch(**SMALL), batch(seed=9, **SMALL)
    twin, m = model(**SMALL), model(**SMALL)
    for mm in (twin, m):
        backward(mm, d0)
        backward(mm, d1)
    twin.engine.materialize_table_grads(accumulate=True)
    ref = {n: p.grad.clone() for n, p in twin.named_parameters() if p.grad is not None}
    assert m.engine.pending is not None
    assert all(p.grad is not None for p in m.engine.table_params().values())
    N = norm64(list(ref.values()))
    c = coef(N, N / 2)
    total = ncf.clip_grad_norm_(m.parameters(), N / 2)
    assert_norm(total, N)
    assert m.engine.pending is None
    got = dict(m.named_parameters())
    for n, g in ref.items():
        assert_scaled(got[n].grad, g, c, n)


def test_hour_backward_with_a_pinned_projection():
    """forward_simple(hour) under model.hour_backward: hour_embed.weight and the nn.Linear
    projection hold dense gradients of their own beside the compact rows and the flat buffer."""
    torch.manual_seed(4)
    U, I, D, T, n = 301, 97, 32, 16, 40
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, T, [64, 32], 4, 0.0, M - 1).to(DEV).train()
    m.hour_backward = True
    lin = torch.nn.Linear(T, D).to(DEV)
    g = torch.Generator().manual_seed(5)
    u = torch.randint(0, U, (n,), generator=g)
    u[1] = u[0]
    p = torch.randint(0, I, (n,), generator=g)
    p[3] = p[2]
    h = torch.randint(0, 24, (n,), generator=g)
    tg = (torch.rand(n, generator=g) < 0.4).float()
    out = ops.forward_simple_hour(m, u.to(DEV), p.to(DEV), h.to(DEV), projection=lin)
    torch.nn.functional.binary_cross_entropy(out, tg.to(DEV)).backward()
    cnt, G, flat = snapshot(m)
    hw = m.temporal_encoding.hour_embed.weight
    for t in (hw.grad, lin.weight.grad, lin.bias.grad):
        t.mul_(100.0)          # (so that leaving them out of the norm would show at 1e-6)
    own = [hw.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()]
    N = norm64([G[k][:cnt[k]] for k in KEYS] + [flat] + own)
    assert N > norm64([G[k][:cnt[k]] for k in KEYS] + [flat]) * (1 + 1e-4)   # (they carry weight)
    c = coef(N, N / 2)
    total = ncf.clip_grad_norm_(list(m.parameters()) + list(lin.parameters()), N / 2)
    assert_norm(total, N)
    w = m.engine.pending
    for k in KEYS:
        assert_scaled(w.G[k][:cnt[k]], G[k][:cnt[k]], c, k)
    assert_scaled(m.engine.flat_grad, flat, c, "flat_grad")
    for t, b in zip((hw.grad, lin.weight.grad, lin.bias.grad), own):
        assert_scaled(t, b, c, tuple(t.shape))


def test_frozen_table_is_left_out():
    m = model(**SMALL)
    m.engine.table_params()["mf_item"].requires_grad_(False)
    backward(m, batch(**SMALL))
    cnt, G, flat = snapshot(m)
    rest = [k for k in KEYS if k != "mf_item"]
    N = norm64([G[k][:cnt[k]] for k in rest] + [flat])
    c = coef(N, N / 2)
    total = ncf.clip_grad_norm_(m.parameters(), N / 2)
    assert_norm(total, N)
    w = m.engine.pending
    for k in rest:
        assert_scaled(w.G[k][:cnt[k]], G[k][:cnt[k]], c, k)
    assert torch.equal(w.G["mf_item"][:cnt["mf_item"]], G["mf_item"][:cnt["mf_item"]])


# ----------------------------------------------------------------------------- 5. Adam
def _assert_moment(got, g, p, c, what):
    ref = (1 - B1) * (c * g.double() + WD * p.double())
    err = (got.double() - ref).abs()
    assert bool((err <= 1e-9 + 1e-5 * ref.abs()).all()), (what, float(err.max()))


def test_adam_consumes_the_clipped_gradient():
    m = model(**SMALL)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    backward(m, batch(**SMALL))
    eng = m.engine
    w = eng.pending
    cnt, G, flat = snapshot(m, poison=False)
    uniq = {"user": w.uniq_u[:cnt["mf_user"]].clone(), "item": w.uniq_i[:cnt["mf_item"]].clone()}
    dense_g = {n: p.grad.clone() for n, p in eng.dense_params()}
    p0 = {n: p.detach().clone() for n, p in eng.dense_params()}
    t0 = {k: p.detach().clone() for k, p in eng.table_params().items()}
    N = norm64([G[k][:cnt[k]] for k in KEYS] + [flat])
    c = coef(N, N / 2)
    assert c < 1
    ncf.clip_grad_norm_(m.parameters(), N / 2)
    opt.step()
    torch.cuda.synchronize()
    for n, p in eng.dense_params():
        _assert_moment(opt.state[p]["exp_avg"], dense_g[n], p0[n], c, n)
    for k, p in eng.table_params().items():
        rows = uniq["user" if k.endswith("user") else "item"]
        _assert_moment(opt.state[p]["exp_avg"][rows], G[k][:cnt[k]], t0[k][rows], c, k)


# ----------------------------------------------------------------------------- 6. composition
def _first_norm(cfg, data):
    m = model(**cfg)
    backward(m, data[0])
    return float(ncf.grad_norm(m.parameters()))


def _clipped_loop(data, max_norm, cfg=SMALL):
    m = model(**cfg)
    opt = torch.optim.Adam(m.parameters(), lr=LR_STEPS, weight_decay=WD)
    crit = torch.nn.BCELoss()
    norms = []
    for u, i, t in data:
        loss = crit(m(kjt(u, i)), t)
        opt.zero_grad()
        loss.backward()
        norms.append(ncf.clip_grad_norm_(m.parameters(), max_norm))
        opt.step()
    assert all(float(x) > max_norm for x in norms), (norms, max_norm)    # clipping bit every step
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    st = {k: {n: (v.cpu().clone() if torch.is_tensor(v) else v) for n, v in s.items()}
          for k, s in opt.state_dict()["state"].items()}
    return sd, st, torch.stack(norms).cpu(), m


def _assert_same_run(a, b):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        for n in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a[1][k][n], b[1][k][n]), (k, n)
    assert torch.equal(a[2], b[2])


def test_deferred_schedule_bitwise_equals_dense(monkeypatch):
    data = batches(3, **SMALL)
    max_norm = _first_norm(SMALL, data) / 2
    monkeypatch.setattr(optim, "SCHEDULE", "dense")
    a = _clipped_loop(data, max_norm)
    monkeypatch.setattr(optim, "SCHEDULE", "deferred")
    b = _clipped_loop(data, max_norm)
    _assert_same_run(a, b)
    assert a[3].engine.deferred is None and b[3].engine.deferred is not None


def test_launch_tapes_bitwise_equal_eager(monkeypatch):
    """(6 steps: the tapes of a geometry are recorded after tapes.RECORD_AFTER eager ones, so the
    last steps replay the forward, the backward and the optimizer step around the clip.)"""
    data = batches(6, **SMALL)
    max_norm = _first_norm(SMALL, data) / 2
    monkeypatch.setattr(tapes, "ENABLED", False)
    a = _clipped_loop(data, max_norm)
    monkeypatch.setattr(tapes, "ENABLED", True)
    b = _clipped_loop(data, max_norm)
    _assert_same_run(a, b)
    assert b[3].engine.tapes.replays > 0 and a[3].engine.tapes.replays == 0


# ----------------------------------------------------------------------------- 7. FusedTrainStep
def _fused(data, cfg=SMALL, prefetch=False, lr=LR, **kw):
    from ncf_amd.trainer import FusedTrainStep
    m = model(**cfg)
    step = FusedTrainStep(m, lr=lr, weight_decay=WD, **kw)
    norms = []
    for s, (u, i, t) in enumerate(data):
        nxt = data[s + 1][:2] if prefetch and s + 1 < len(data) else None
        step(u, i, t, next=nxt)
        if step.last_grad_norm is not None:
            norms.append(step.last_grad_norm.clone())
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    step.sync()
    mom = {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
           for k, v in step.state.items()}
    return sd, mom, (step.m_flat.cpu().clone(), step.v_flat.cpu().clone()), norms, step


def _assert_same_fused(a, b):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1]), k
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])


@pytest.mark.parametrize("cfg", [SMALL, LARGE], ids=["small", "large"])
def test_fused_step_reordered_keeps_the_bits(cfg):
    """max_grad_norm = 1e30 (the reordered step: separate apply behind the clip, no late
    catch-up left behind) against None (the apply fused into the embedding backward), three
    steps with the next batch prefetched."""
    data = batches(3, **cfg)
    a = _fused(data, cfg, prefetch=True)
    b = _fused(data, cfg, prefetch=True, max_grad_norm=1e30)
    _assert_same_fused(a, b)
    assert a[4].last_grad_norm is None and len(b[3]) == 3
    assert b[4]._late_next is None


def _fused_first_step_check(**kw):
    from ncf_amd.trainer import FusedTrainStep
    data = batch(**SMALL)
    twin = model(**SMALL)
    ts = FusedTrainStep(twin, lr=LR, weight_decay=WD, **kw)
    w = ts(*data)
    cnt = counts(w)
    G = {k: w.G[k][:cnt[k]].clone() for k in KEYS}
    flat = twin.engine.flat_grad.clone()
    uniq = {"user": w.uniq_u[:cnt["mf_user"]].clone(), "item": w.uniq_i[:cnt["mf_item"]].clone()}
    N = norm64(list(G.values()) + [flat])
    c = coef(N, N / 2)
    assert c < 1
    m = model(**SMALL)
    step = FusedTrainStep(m, lr=LR, weight_decay=WD, max_grad_norm=N / 2, **kw)
    p_flat = m.engine.flat.clone()
    t0 = {k: p.detach().clone() for k, p in m.engine.table_params().items()}
    step(*data)
    torch.cuda.synchronize()
    assert_norm(step.last_grad_norm, N)
    _assert_moment(step.m_flat, flat, p_flat, c, "flat")
    for k in KEYS:
        rows = uniq["user" if k.endswith("user") else "item"]
        _assert_moment(step.state[k]["exp_avg"][rows], G[k], t0[k][rows], c, k)


def test_fused_step_clips_vs_float64():
    _fused_first_step_check()


def test_fused_step_clips_bf16_tables():
    _fused_first_step_check(table_dtype=torch.bfloat16)


def test_fused_step_graph_bitwise_equals_eager_clock():
    data = batches(3, **SMALL)
    max_norm = _first_norm(SMALL, data) / 2
    a = _fused(data, lr=LR_STEPS, clock=True, max_grad_norm=max_norm)
    b = _fused(data, lr=LR_STEPS, graph=True, max_grad_norm=max_norm)
    _assert_same_fused(a, b)
    assert b[4]._g is not None                         # (the third step was captured and replayed)
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3])) and len(b[3]) == 3
    assert all(float(x) > max_norm for x in b[3])


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from ncf_amd.trainer import FusedTrainStep
    m = model(**SMALL)
    backward(m, batch(**SMALL))
    cnt, G, flat = snapshot(m, poison=False)
    with pytest.raises(NotImplementedError, match="norm_type"):
        ncf.clip_grad_norm_(m.parameters(), 1.0, norm_type=1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            ncf.clip_grad_norm_(m.parameters(), bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedTrainStep(model(**SMALL), max_grad_norm=bad)
    many = [torch.nn.Parameter(torch.ones(4, device=DEV)) for _ in range(33)]
    for p in many:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError, match="segments"):
        ncf.clip_grad_norm_(many, 1.0)
    cpu = torch.nn.Parameter(torch.ones(4))
    cpu.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="CPU"):
        ncf.clip_grad_norm_(list(m.parameters()) + [cpu], 1.0)
    dbl = torch.nn.Parameter(torch.ones(4, device=DEV, dtype=torch.float64))
    dbl.grad = torch.ones_like(dbl)
    with pytest.raises(RuntimeError, match="float64"):
        ncf.clip_grad_norm_([dbl], 1.0)
    w = m.engine.pending
    w.sent_rows = True          # as engine.backward(grad_rows=...) of the row-sharded step marks it
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ncf.clip_grad_norm_(m.parameters(), 1.0)
    w.sent_rows = False
    # none of the refused calls scaled anything
    for k in KEYS:
        assert torch.equal(w.G[k][:cnt[k]], G[k][:cnt[k]]), k
    assert torch.equal(m.engine.flat_grad, flat)
    # a parameter list without gradients: torch's 0
    assert float(ncf.clip_grad_norm_([torch.nn.Parameter(torch.ones(3, device=DEV))], 1.0)) == 0.0


def test_error_if_nonfinite_raises_before_scaling():
    m = model(**SMALL)
    backward(m, batch(**SMALL))
    cnt, G, flat = snapshot(m, poison=False)
    N = norm64([G[k][:cnt[k]] for k in KEYS] + [flat])
    assert_norm(ncf.clip_grad_norm_(m.parameters(), 10 * N, error_if_nonfinite=True), N)
    m.engine.flat_grad[3] = float("inf")
    flat = m.engine.flat_grad.clone()
    with pytest.raises(RuntimeError, match="non-finite"):
        ncf.clip_grad_norm_(m.parameters(), N / 2, error_if_nonfinite=True)
    w = m.engine.pending
    for k in KEYS:
        assert torch.equal(w.G[k][:cnt[k]], G[k][:cnt[k]]), k
    assert torch.equal(m.engine.flat_grad, flat)
    assert math.isinf(float(ncf.grad_norm(m.parameters())))


def test_model_trainer_clips_only_when_asked(monkeypatch):
    """ModelTrainer(clip_gradients=True) clips to config['gradient_clipping'] every batch;
    the default mirrors the reference's dead guard (the key is there, nothing is clipped)."""
    import ncf_amd.trainer as Tr
    calls = []
    orig = Tr.clip_grad_norm_

    def counted(params, max_norm, *a, **k):
        out = orig(params, max_norm, *a, **k)
        calls.append((max_norm, out))
        return out
    monkeypatch.setattr(Tr, "clip_grad_norm_", counted)
    loader = [(kjt(u, i), t) for u, i, t in batches(3, **SMALL)]
    config = dict(num_users=SMALL["U"], num_products=SMALL["I"], batch_size=SMALL["B"],
                  learning_rate=LR, negative_samples=M - 1, gradient_clipping=1e-3)
    tr = Tr.ModelTrainer(model(**SMALL), config, clip_gradients=True)
    loss = tr.train_epoch(loader)
    assert math.isfinite(loss) and len(calls) == 3
    assert all(mn == 1e-3 and float(n) > 1e-3 for mn, n in calls)       # and it bit
    first = float(calls[0][1])
    del calls[:]
    tr = Tr.ModelTrainer(model(**SMALL), config)
    loss2 = tr.train_epoch(loader)
    assert math.isfinite(loss2) and calls == []
    # ... and ends, bit for bit, where the reference loop without clipping ends
    m = model(**SMALL)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=1e-5)
    for f, t in loader:
        l_ = torch.nn.BCELoss()(m(f), t)
        opt.zero_grad()
        l_.backward()
        opt.step()
    want, got = m.state_dict(), tr.model.state_dict()
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert first > 1e-3
