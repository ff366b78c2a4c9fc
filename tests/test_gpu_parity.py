"""GPU parity: the HIP path (through the C-ABI library) against the reference's golden vectors
and the CPU oracle.  Runs on a real MI355X only (marker ``gpu``).

Tolerances (tests/parity.py): fp32 forward abs <= 2e-6 on probabilities; gradients
rel 1e-4 / abs 1e-6 (summation order differs from ATen's CPU kernels); post-Adam parameters abs
1e-6 outside the sign-flip zone (<= 2*lr per step inside it)."""
import ctypes

import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O
from tests.conftest import sub
from tests.parity import (assert_moment_close, assert_params_close, zone_from_grads,
                          zone_masks)

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import deferred as _D  # noqa: E402
from ncf_amd import engine as _E  # noqa: E402
DEV = torch.device("cuda:0")

# Tests that hold two code paths to the same bits where one of them runs the fused attention +
# tower: both sides in its 80-row tiles (the small-batch tiles, engine.SMALL_TILE_GROUPS, round the
# input gradients differently: test_small_batch_tiles_vs_80_row_tiles compares the two forms)
_EIGHTY_ROW_TILES = {"test_attn_block_recompute_bitwise_equals_stash",
                     "test_attn_o_recompute_bitwise_equals_o_stash",
                     "test_attn_shared_q_matches_per_row",
                     # (the standalone 16-group backward on the fused forward's stash, whose
                     # per-workgroup shared-Q records follow the forward's tiles)
                     "test_attn_stash_backward_reads_the_forwards_q_record"}


@pytest.fixture(autouse=True)
def _eighty_row_tiles(request, monkeypatch):
    if request.node.originalname in _EIGHTY_ROW_TILES:
        monkeypatch.setattr(_E, "SMALL_TILE_GROUPS", 0)


def kjt(u, i):
    u = torch.as_tensor(u, dtype=torch.long)
    i = torch.as_tensor(i, dtype=torch.long)
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([u, i]),
        lengths=torch.ones(2 * u.numel(), dtype=torch.long)).to(DEV)


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


# ----------------------------------------------------------------------------- F1
def test_f1_eval_known_answer(f1):
    sd = T(sub(f1, "sd/"))
    m = ncf.AdvancedNCF(int(f1["cfg"][0]), int(f1["cfg"][1]), 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    with torch.no_grad():
        out = m(kjt(f1["user_ids"], f1["item_ids"])).cpu().numpy().reshape(-1)
        # batches of 32 like local_inference.py:121-129
        outb = np.concatenate([m(kjt(f1["user_ids"][s:s + 32], f1["item_ids"][s:s + 32]))
                               .cpu().numpy().reshape(-1) for s in range(0, 1000, 32)])
    # fp32 forward abs 1e-6 (the reference's own re-run is 2.98e-7 from the CSV)
    assert np.abs(out - f1["csv_pred"]).max() < 1e-6
    assert np.abs(out - f1["ref_pred"]).max() < 1e-6
    assert np.array_equal(out, outb)


# ----------------------------------------------------------------------------- F2/F3
def _train_run(g, n_layers, materialize_step0):
    U, I, D, Tt, H, B, M, steps = [int(x) for x in g["cfg"]]
    hidden = [int(x) for x in g["hidden"]]
    lr, wd = [float(x) for x in g["hparams"]]
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, Tt, hidden, H, 0.0, M - 1)
    m.load_state_dict(T(sub(g, "init/")), strict=True)
    m = m.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=wd)
    crit = torch.nn.BCELoss()
    rec = {}
    for s in range(steps):
        m.train()
        out = m(kjt(g[f"step{s}/user_ids"], g[f"step{s}/item_ids"]))
        loss = crit(out, torch.from_numpy(g[f"step{s}/targets"]).to(DEV))
        opt.zero_grad()
        loss.backward()
        rec[f"prob{s}"] = out.detach().cpu().numpy()
        rec[f"loss{s}"] = loss.item()
        if s == 0 and materialize_step0:
            m.engine.materialize_table_grads()
            rec["grads0"] = {n: p.grad.detach().cpu().numpy().copy()
                             for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        if s in (0, steps - 1):
            rec[f"params{s}"] = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    rec["state"] = {n: {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v)
                        for k, v in opt.state[p].items()}
                    for n, p in m.named_parameters() if p in opt.state}
    rec["model"] = m
    return rec


@pytest.mark.parametrize("fx,nl", [("f2", 3), ("f3", 2)])
@pytest.mark.parametrize("materialize", [False, True])
def test_train_goldens(fx, nl, materialize, request):
    g = request.getfixturevalue(fx)
    steps = int(g["cfg"][7])
    lr, wd = [float(x) for x in g["hparams"]]
    rec = _train_run(g, nl, materialize)
    for s in range(steps):
        # fp32 forward abs 1e-6 (measured <= 3.9e-7 for F2, round 3)
        assert np.abs(rec[f"prob{s}"] - g[f"step{s}/prob"]).max() < 1e-6, s
        assert abs(rec[f"loss{s}"] - float(g[f"step{s}/loss"])) < 2e-6, s
    if materialize:
        gold = sub(g, "grad0/")
        got = rec["grads0"]
        assert set(got) == set(gold), set(got) ^ set(gold)
        for k, v in gold.items():
            np.testing.assert_allclose(got[k], v, rtol=1e-4, atol=1e-6, err_msg=k)
    for s in (0, steps - 1):
        for k, v in sub(g, f"after{s}/param/").items():
            assert_params_close(k, rec[f"params{s}"][k], v, zone_masks(g, k, s + 1), lr)
    # unused parameters (grad None in the reference) never move
    for k in g["grad_none0"].tolist():
        assert np.array_equal(rec[f"params{steps - 1}"][k], g["init/" + k]), k
    for k, v in sub(g, f"after{steps - 1}/exp_avg/").items():
        zs = zone_masks(g, k, steps)
        assert_moment_close(k, rec["state"][k]["exp_avg"], v, zs)
        assert_moment_close(k, rec["state"][k]["exp_avg_sq"], g[f"after{steps - 1}/exp_avg_sq/" + k],
                            zs, atol=1e-12)
        assert float(rec["state"][k]["step"]) == steps
    # eval forward on the trained weights (M = 1) and forward_simple
    m = rec["model"]
    m.eval()
    with torch.no_grad():
        ev = m(kjt(g["eval/user_ids"], g["eval/item_ids"])).cpu().numpy()
        fs = m.forward_simple(torch.from_numpy(g["eval/user_ids"]).to(DEV),
                              torch.from_numpy(g["eval/item_ids"]).to(DEV)).cpu().numpy()
    assert np.abs(ev - g["eval/prob"]).max() < 1e-4
    assert np.abs(fs - g["eval/simple"]).max() < 1e-4


def test_train_deterministic(f2):
    a = _train_run(f2, 3, False)
    b = _train_run(f2, 3, False)
    for k, v in a["params2"].items():
        assert np.array_equal(v, b["params2"][k]), k


# ----------------------------------------------------------------------------- larger vs oracle
@pytest.mark.parametrize("U,I,D,H,hidden,B,M,Dm", [
    (5000, 1000, 64, 4, [256, 128, 64], 256, 5, 64),
    (943, 1682, 16, 1, [64, 32], 256, 5, 16),       # C1 shape (ML-100K)
    (3000, 700, 128, 4, [256, 128, 64], 64, 5, 128),  # C4 dims (hd = 32)
    # mf_embedding_dim != mlp_embedding_dim (architecture.py:122-133, 153-190: the two
    # collections at their own widths; ragged group count)
    (3000, 700, 64, 4, [256, 128, 64], 61, 5, 32),
    (943, 1682, 16, 1, [64, 32], 99, 5, 128),
])
def test_train_vs_oracle(U, I, D, H, hidden, B, M, Dm):
    """Two steps of the reference call pattern (model(kjt) -> BCE -> backward -> Adam.step)
    against the oracle's training step: probabilities, loss, step-0 gradients of every
    parameter, and the parameters after both steps."""
    torch.manual_seed(3)
    m = ncf.AdvancedNCF(U, I, 5, 24, Dm, D, 32, hidden, H, 0.0, M - 1)
    ref = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    oopt = O.AdamState(lr=1e-3, weight_decay=1e-5)
    gen = torch.Generator().manual_seed(4)
    zones = {}
    for step in range(2):
        # Zipf-ish items (hot ids repeat many times) exercise long segments
        users = torch.randint(0, U, (B,), generator=gen).repeat_interleave(M)
        items = (torch.rand(B * M, generator=gen) ** 3 * I).long().clamp_max(I - 1)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        t = t.reshape(-1, 1)
        m.train()
        out = m(kjt(users, items))
        loss = torch.nn.functional.binary_cross_entropy(out, t.to(DEV))
        opt.zero_grad()
        loss.backward()
        if step == 0:
            m.engine.materialize_table_grads()
            grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        before = {k: v.clone() for k, v in ref.items()}
        prob, oloss, ograds = O.train_step(ref, oopt, users, items, t, negative_samples=M - 1,
                                           num_heads=H, temporal_dim=32, n_layers=len(hidden))
        for k, v in ograds.items():
            zones.setdefault(k, []).append(zone_from_grads(v.numpy(), before[k].numpy(), 1e-5))
        assert (out.detach().cpu() - prob).abs().max().item() < 5e-6
        assert abs(loss.item() - float(oloss)) < 5e-6
        if step == 0:
            for k, v in ograds.items():
                np.testing.assert_allclose(grads[k].numpy(), v.numpy(), rtol=2e-4, atol=2e-6,
                                           err_msg=k)
    sd = m.state_dict()
    for k, zs in zones.items():
        assert_params_close(k, sd[k].cpu().numpy(), ref[k].numpy(), zs, 1e-3, atol=5e-6)
    if Dm != D:
        # the eval forward and forward_simple at split widths against the oracle's
        m.eval()
        users = torch.randint(0, U, (77,), generator=gen)
        items = torch.randint(0, I, (77,), generator=gen)
        with torch.no_grad():
            ev = m(kjt(users, items)).cpu()
            fs = m.forward_simple(users.to(DEV), items.to(DEV)).cpu()
        oev = O.forward({k: v for k, v in ref.items()}, users, items, training=False,
                        negative_samples=M - 1, num_heads=H, temporal_dim=32,
                        n_layers=len(hidden))
        assert (ev - oev).abs().max().item() < 5e-6
        assert (fs - oev[:, 0]).abs().max().item() < 5e-6
        with pytest.raises(RuntimeError):     # the reference's broadcast fails the same way
            m.forward_simple(users.to(DEV), items.to(DEV), torch.zeros(77, dtype=torch.long,
                                                                      device=DEV))


def test_split_widths_fused_step_equals_reference_call_pattern():
    """FusedTrainStep at mf_embedding_dim != mlp_embedding_dim (the dense table schedule) against
    the reference call pattern on the same batches: after 3 steps, parameters within 1e-6 but for
    the elements whose gradient is summation noise (the fused step's BCE gradient is its own
    kernel's, torch's BCE backward the other's)."""
    from ncf_amd.trainer import FusedTrainStep
    U, I, B, M = 900, 300, 37, 5
    g = torch.Generator().manual_seed(8)
    bs = []
    for _ in range(3):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = torch.randint(0, I, (B * M,), generator=g)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        bs.append((u, i, t.reshape(-1, 1)))
    out = []
    for fused in (False, True):
        torch.manual_seed(9)
        m = ncf.AdvancedNCF(U, I, 5, 24, 32, 64, 32, [256, 128, 64], 4, 0.0, M - 1).to(DEV)
        if fused:
            step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
            assert step.deferred is None
            for u, i, t in bs:
                step(u.to(DEV), i.to(DEV), t.to(DEV))
        else:
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
            m.train()
            for u, i, t in bs:
                loss = torch.nn.functional.binary_cross_entropy(m(kjt(u, i)), t.to(DEV))
                opt.zero_grad()
                loss.backward()
                opt.step()
        out.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    # Adam's first steps move each element by about lr x sign(g): an element whose gradient is
    # summation noise (|g| near eps) may move differently in the two runs (the two BCE
    # gradients differ in the last bit), by at most 2 lr per step; every other element agrees
    for k in out[0]:
        d = (out[1][k] - out[0][k]).abs()
        assert d.max().item() <= 3 * 2e-3 + 1e-6, (k, d.max().item())
        # (k_proj.bias: its exact gradient is 0 — softmax ignores a per-query constant)
        assert (d > 1e-6).sum().item() <= max(2, 0.01 * d.numel()), (k, (d > 1e-6).sum().item())


def test_forward_simple_train_mode_vs_oracle():
    """forward_simple(users, items) in training mode (architecture.py:409-485 under
    model.train(): one item per group, the attention over a single key) is differentiable: two
    steps of forward_simple -> BCE -> backward -> torch.optim.Adam against the oracle's training
    step with negative_samples = 0 (the same math), probabilities / loss / step-0 gradients and
    the parameters after both steps (dropout 0: the reference's masks are torch's RNG).  With
    dropout active the output is a fresh draw every call and the backward runs."""
    U, I, D, H, hidden, B = 700, 300, 64, 4, [256, 128, 64], 333
    torch.manual_seed(13)
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, 32, hidden, H, 0.0, 4)
    ref = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    oopt = O.AdamState(lr=1e-3, weight_decay=1e-5)
    gen = torch.Generator().manual_seed(14)
    zones = {}
    for step in range(2):
        users = torch.randint(0, U, (B,), generator=gen)
        items = (torch.rand(B, generator=gen) ** 3 * I).long().clamp_max(I - 1)
        t = (torch.rand(B, generator=gen) < 0.3).float()
        out = m.forward_simple(users.to(DEV), items.to(DEV))
        assert out.shape == (B,) and out.requires_grad
        loss = torch.nn.functional.binary_cross_entropy(out, t.to(DEV))
        opt.zero_grad()
        loss.backward()
        if step == 0:
            m.engine.materialize_table_grads()
            grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        before = {k: v.clone() for k, v in ref.items()}
        prob, oloss, ograds = O.train_step(ref, oopt, users, items, t.reshape(-1, 1),
                                           negative_samples=0, num_heads=H, temporal_dim=32,
                                           n_layers=len(hidden))
        for k, v in ograds.items():
            zones.setdefault(k, []).append(zone_from_grads(v.numpy(), before[k].numpy(), 1e-5))
        assert (out.detach().cpu() - prob.reshape(-1)).abs().max().item() < 5e-6
        assert abs(loss.item() - float(oloss)) < 5e-6
        if step == 0:
            for k, v in ograds.items():
                np.testing.assert_allclose(grads[k].numpy(), v.numpy(), rtol=2e-4, atol=2e-6,
                                           err_msg=k)
    sd = m.state_dict()
    for k, zs in zones.items():
        assert_params_close(k, sd[k].cpu().numpy(), ref[k].numpy(), zs, 1e-3, atol=5e-6)
    # dropout active: fresh masks per call, gradients flow
    torch.manual_seed(15)
    md = ncf.AdvancedNCF(U, I, 5, 24, D, D, 32, hidden, H, 0.5, 4).to(DEV).train()
    u = torch.randint(0, U, (B,), device=DEV)
    i = torch.randint(0, I, (B,), device=DEV)
    a, b = md.forward_simple(u, i), md.forward_simple(u, i)
    assert not torch.equal(a, b)
    md.eval()
    with torch.no_grad():
        e = md.forward_simple(u, i)
    md.train()
    a.sum().backward()
    g = md.mlp[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    assert (a - e).abs().max().item() > 1e-4      # not the eval output


# ----------------------------------------------------------------------------- op level (F4)
@pytest.mark.parametrize("tag", ["mha5", "mha50", "mha5_h1"])
def test_f4_mha(f4, tag):
    Bn, L, D, H = [int(x) for x in f4[f"{tag}/shape"]]
    mod = ncf.MultiHeadAttention(D, H, dropout=0.0)
    mod.load_state_dict(T(sub(f4, f"{tag}/w/")))
    mod = mod.to(DEV)
    q, k, v = [torch.from_numpy(f4[f"{tag}/{n}"]).to(DEV).requires_grad_(True) for n in "qkv"]
    y = mod(q, k, v)
    np.testing.assert_allclose(y.detach().cpu().numpy(), f4[f"{tag}/y"], atol=2e-5, rtol=1e-5)
    y.backward(torch.from_numpy(f4[f"{tag}/gy"]).to(DEV))
    for n, t in zip("qkv", (q, k, v)):
        np.testing.assert_allclose(t.grad.cpu().numpy(), f4[f"{tag}/g{n}"], atol=2e-5, rtol=1e-4)
    for n, p in mod.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), f4[f"{tag}/gw/{n}"], atol=5e-5, rtol=1e-4,
                                   err_msg=n)


@pytest.mark.parametrize("kind", ["causal", "padding", "per_head"])
def test_mha_mask_vs_oracle(f4, kind):
    """MultiHeadAttention.forward's mask (architecture.py:36, 47-48: masked_fill(mask == 0,
    -inf) broadcast against the [B, H, L, L] scores) on the F4 mha5 module and inputs: a causal
    [L, L] mask, a key-padding [B, 1, 1, L] mask and a random per-head [B, H, L, L] mask (every
    row keeps at least one key), forward and backward against the oracle's restatement with the
    same mask (the reference's fixtures hold no masked call: that part of the pin is the
    restatement of :47-48).  A fully masked row comes out NaN, as torch's softmax makes it."""
    Bn, L, D, H = [int(x) for x in f4["mha5/shape"]]
    w = T(sub(f4, "mha5/w/"))
    mod = ncf.MultiHeadAttention(D, H, dropout=0.0)
    mod.load_state_dict(w)
    mod = mod.to(DEV)
    g = torch.Generator().manual_seed(3)
    if kind == "causal":
        mask = torch.tril(torch.ones(L, L, dtype=torch.bool))
    elif kind == "padding":
        lens = torch.randint(1, L + 1, (Bn,), generator=g)
        mask = (torch.arange(L)[None, :] < lens[:, None]).view(Bn, 1, 1, L)
    else:
        mask = torch.rand(Bn, H, L, L, generator=g) < 0.6
        mask[..., 0] = True
    qkv = [torch.from_numpy(f4[f"mha5/{n}"]) for n in "qkv"]
    gy = torch.from_numpy(f4["mha5/gy"])
    xs = [t.to(DEV).requires_grad_(True) for t in qkv]
    y = mod(*xs, mask=mask.to(DEV))
    y.backward(gy.to(DEV))
    ps = {f"a.{k}": v.clone().requires_grad_(True) for k, v in w.items()}
    rs = [t.clone().requires_grad_(True) for t in qkv]
    ry = O.mha(ps, "a.", *rs, H, mask=mask)
    ry.backward(gy)
    torch.testing.assert_close(y.detach().cpu(), ry.detach(), atol=2e-5, rtol=1e-5)
    for a_, b_ in zip(xs, rs):
        torch.testing.assert_close(a_.grad.cpu(), b_.grad, atol=2e-5, rtol=1e-4)
    for n, p in mod.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), ps[f"a.{n}"].grad, atol=5e-5, rtol=1e-4)
    # a fully masked row (group 0, head 0, query 0): NaN in that group's outputs, like torch
    if kind == "per_head":
        m2 = mask.clone()
        m2[0, 0, 0, :] = False
        with torch.no_grad():
            y2 = mod(*[t.detach() for t in xs], mask=m2.to(DEV)).cpu()
            r2 = O.mha({k: v.detach() for k, v in ps.items()}, "a.", *qkv, H, mask=m2)
        assert torch.isnan(y2[0]).any() and torch.equal(torch.isnan(y2), torch.isnan(r2))
        torch.testing.assert_close(y2[1:], r2[1:], atol=2e-5, rtol=1e-5)


def test_f4_temporal(f4):
    te = ncf.TemporalEncoding(32)
    te.load_state_dict({**T(sub(f4, "te/w/")), "pe": torch.from_numpy(f4["te/pe"])})
    te = te.to(DEV)
    args = [torch.from_numpy(f4[f"te/{n}"]).to(DEV) for n in ("hour", "day", "month", "days_since")]
    y = te(*args)
    np.testing.assert_allclose(y.detach().cpu().numpy(), f4["te/y"], atol=1e-6)
    y.backward(torch.from_numpy(f4["te/gy"]).to(DEV))
    for n in ("hour_embed.weight", "day_embed.weight", "month_embed.weight"):
        mod = getattr(te, n.split(".")[0])
        np.testing.assert_allclose(mod.weight.grad.cpu().numpy(), f4["te/gw/" + n], atol=1e-5,
                                   rtol=1e-5)


# ----------------------------------------------------------------------------- scoring (F5)
def test_f5_scoring_and_embeddings(f5):
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    items = torch.arange(366, device=DEV)
    with torch.no_grad():
        sc = torch.stack([m.forward_simple(torch.full_like(items, u), items) for u in range(nu)])
        ts, ti = sc.topk(10, dim=1)
        ue = m.get_user_embeddings({"user_features": kjt(torch.arange(nu), torch.zeros(nu))})
        pid = torch.from_numpy(f5["emb_pids"])
        pe = m.get_product_embeddings({
            "product_features": kjt(torch.zeros_like(pid), pid),
            "category_features": {"department_ids": torch.from_numpy(f5["emb_dept"]).to(DEV),
                                  "category_ids": torch.from_numpy(f5["emb_cat"]).to(DEV)}})
    np.testing.assert_allclose(sc.cpu().numpy(), f5["scores"], atol=2e-6)
    assert (ti.cpu().numpy() == f5["top_items"]).all()
    np.testing.assert_allclose(ue["mf"].cpu().numpy(), f5["emb_user_mf"], atol=2e-6)
    np.testing.assert_allclose(ue["mlp"].cpu().numpy(), f5["emb_user_mlp"], atol=2e-6)
    np.testing.assert_allclose(pe["mf"].cpu().numpy(), f5["emb_item_mf"], atol=2e-6)
    np.testing.assert_allclose(pe["mlp"].cpu().numpy(), f5["emb_item_mlp"], atol=2e-6)
    np.testing.assert_allclose(pe["category"].cpu().numpy(), f5["emb_item_category"], atol=1e-5)


def test_category_hierarchy_train_mode_vs_oracle(f5):
    """CategoryHierarchy.forward in training mode (architecture.py:111-119, its two nn.Dropouts
    active; the drop-in used to refuse it): against a float64 restatement of the reference
    module on the F5 model's department / category tables with the kernel's own keep-scales
    (the attention weight over the single key: one keep-or-drop per (row, head); the output:
    one per element), fresh masks per call, keep fractions near 1 - p, and p = 0 equal to eval."""
    from ncf_amd import ops
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24, dropout=0.3).to(DEV)
    m.load_state_dict(sd, strict=True)
    ch = m.category_hierarchy.train()
    g = torch.Generator().manual_seed(3)
    n = 48
    dept = torch.randint(0, 5, (n,), generator=g)
    cat = torch.randint(0, 24, (n,), generator=g)
    scales = {}
    with torch.no_grad():
        out = ops._category_hierarchy_train(ch, dept.to(DEV), cat.to(DEV), 0.3, 0.3, seed=77,
                                            scales=scales)
    D = ch.department_embed.weight.shape[1]
    H = ch.hierarchy_attn.num_heads
    P = {k: v.detach().cpu().double() for k, v in ch.state_dict().items()}
    sa, so = scales["attn"].cpu().double(), scales["out"].cpu().double()
    v = P["department_embed.weight"][dept] @ P["hierarchy_attn.v_proj.weight"].T + \
        P["hierarchy_attn.v_proj.bias"]                                  # softmax over 1 key = 1
    v = (v.view(n, H, D // H) * sa[:, :, None]).reshape(n, D)           # attention dropout (:51)
    a = (v @ P["hierarchy_attn.out_proj.weight"].T + P["hierarchy_attn.out_proj.bias"]) * so
    h = a[:, None, :] + P["category_embed.weight"][cat][None, :, :]     # [n,1,D] + [n,D] (:119)
    ref = torch.nn.functional.layer_norm(h, (D,), P["norm.weight"], P["norm.bias"], 1e-5)
    np.testing.assert_allclose(out.cpu().double().numpy(), ref.numpy(), atol=2e-5, rtol=1e-5)
    for x, cnt in ((sa, n * H), (so, n * D)):
        assert all(abs(u) < 1e-9 or abs(u - 1 / 0.7) < 1e-5 for u in x.unique().tolist())
        keep = (x > 0).double().mean().item()
        assert abs(keep - 0.7) < 4 * (0.21 / cnt) ** 0.5 + 0.01, keep
    # the public module: runs in training mode, fresh masks per call; p = 0 is the eval output
    with torch.no_grad():
        y1 = ch(dept.to(DEV), cat.to(DEV))
        y2 = ch(dept.to(DEV), cat.to(DEV))
        assert y1.shape == (n, n, D) and not torch.equal(y1, y2)
        ch.eval()
        ye = ch(dept.to(DEV), cat.to(DEV))
        ch.train()
        z = ops._category_hierarchy_train(ch, dept.to(DEV), cat.to(DEV), 0.0, 0.0, seed=5)
    torch.testing.assert_close(z, ye, rtol=1e-6, atol=2e-6)


# ----------------------------------------------------------------------------- kernels vs torch
@pytest.mark.parametrize("a_t,b_t", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("Mm,Nn,Kk", [(77, 130, 45), (256, 64, 1000), (1, 5, 3)])
def test_gemm_vs_torch(a_t, b_t, Mm, Nn, Kk):
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(Mm + Nn + Kk)
    A = torch.randn(Mm, Kk, generator=g)
    Bm = torch.randn(Kk, Nn, generator=g) * torch.arange(1, Nn + 1)  # asymmetric
    bias = torch.randn(Nn, generator=g)
    As = (A.t().contiguous() if a_t else A).to(DEV)
    Bs = (Bm.t().contiguous() if b_t else Bm).to(DEV)
    C = torch.empty(Mm, Nn, device=DEV)
    _lib.call("ncf_gemm_f32", Mm, Nn, Kk, As.data_ptr(), Mm if a_t else Kk, a_t, Bs.data_ptr(),
              Kk if b_t else Nn, b_t, C.data_ptr(), Nn, bias.to(DEV).data_ptr(), 1,
              _lib.stream_ptr(DEV))
    ref = torch.relu(A.double() @ Bm.double() + bias.double()).float()
    np.testing.assert_allclose(C.cpu().numpy(), ref.numpy(), atol=1e-4 * (Kk ** 0.5), rtol=1e-4)
    # split-K path (+ row sums of A), inline and deferred through ncf_reduce_batch: bit-identical
    ws = torch.empty(_lib.query("ncf_gemm_splitk_workspace", Mm, Nn, 7), device=DEV)
    C2, rs = torch.empty(Mm, Nn, device=DEV), torch.empty(Mm, device=DEV)
    _lib.call("ncf_gemm_f32_splitk", Mm, Nn, Kk, As.data_ptr(), Mm if a_t else Kk, a_t,
              Bs.data_ptr(), Kk if b_t else Nn, b_t, C2.data_ptr(), Nn, 0, rs.data_ptr(), 7,
              ws.data_ptr(), ws.numel(), None, _lib.stream_ptr(DEV))
    ref2 = (A.double() @ Bm.double()).float()
    np.testing.assert_allclose(C2.cpu().numpy(), ref2.numpy(), atol=1e-4 * (Kk ** 0.5), rtol=1e-4)
    np.testing.assert_allclose(rs.cpu().numpy(), A.double().sum(1).float().numpy(),
                               atol=1e-4 * (Kk ** 0.5), rtol=1e-4)
    lst = _lib.ReduceList()
    C3, rs3 = torch.empty(Mm, Nn, device=DEV), torch.empty(Mm, device=DEV)
    _lib.call("ncf_gemm_f32_splitk", Mm, Nn, Kk, As.data_ptr(), Mm if a_t else Kk, a_t,
              Bs.data_ptr(), Kk if b_t else Nn, b_t, C3.data_ptr(), Nn, 0, rs3.data_ptr(), 7,
              ws.data_ptr(), ws.numel(), lst.address, _lib.stream_ptr(DEV))
    assert lst.count == 2
    scr = torch.empty(max(1, _lib.query("ncf_reduce_batch_scratch", lst.address)), device=DEV)
    _lib.call("ncf_reduce_batch", lst.address, scr.data_ptr(), scr.numel(), _lib.stream_ptr(DEV))
    assert torch.equal(C2, C3) and torch.equal(rs, rs3)


def test_reduce_batch_matches_inline_reduce():
    """Many descriptors (> one launch), P on both sides of the 2-stage threshold, strided outputs,
    accumulate and scale: ncf_reduce_batch == fp64 sums, and == ncf_gemm_f32_splitk's inline
    reduce order (checked above)."""
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(5)
    lst = _lib.ReduceList()
    cases = []
    for j in range(30):
        P = [1, 3, 64, 128, 129, 200, 1000][j % 7]
        L = [1, 7, 64, 65, 300][j % 5]
        cols = 1 if j % 2 == 0 else L
        part = torch.randn(P, L + 3, generator=g).to(DEV)      # stride L + 3
        rows = (L + cols - 1) // cols
        ldo = cols + 2
        out = torch.randn(rows * ldo, generator=g).to(DEV)
        acc, scale = j % 3 == 0, [1.0, 0.5][j % 2]
        d = lst.d[lst.count]
        d.part, d.out, d.stride, d.ldo = part.data_ptr(), out.data_ptr(), L + 3, ldo
        d.L, d.cols, d.P, d.accumulate, d.scale = L, cols, P, int(acc), scale
        lst.count += 1
        cases.append((part, out.clone(), out, L, cols, ldo, acc, scale))
    scr = torch.empty(max(1, _lib.query("ncf_reduce_batch_scratch", lst.address)), device=DEV)
    _lib.call("ncf_reduce_batch", lst.address, scr.data_ptr(), scr.numel(), _lib.stream_ptr(DEV))
    for part, before, out, L, cols, ldo, acc, scale in cases:
        s = part[:, :L].double().sum(0).cpu() * scale
        exp = before.double().cpu().clone()
        for i in range(L):
            k = (i // cols) * ldo + i % cols
            exp[k] = s[i] + (exp[k] if acc else 0.0)
        np.testing.assert_allclose(out.cpu().double().numpy(), exp.numpy(), rtol=1e-5, atol=1e-4)


def test_reduce_batch_vec_lanes_bitwise_equal_scalar():
    """ncf_reduce_batch with 16-byte lanes (four columns per lane, ncf_reduce_set_vec 1, the
    default; 2: 32 loads in flight per thread) against one column per lane, bit for bit: one- and
    two-stage descriptors (P up to 1000), L and stride multiples of 4 (vec) beside ones that are
    not (scalar in the same launch), a partial base 8 bytes off a 16-byte boundary (scalar),
    accumulate and scale."""
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(9)
    specs = []
    for j in range(27):
        P = [1, 5, 64, 129, 256, 257, 1000, 300, 2][j % 9]
        L = [4, 64, 300, 1024, 7, 66, 2048][j % 7]
        stride = L + [0, 4, 1][j % 3]
        off = 2 if j % 5 == 4 else 0
        cols = 1 if j % 2 == 0 else L
        specs.append((P, L, stride, off, cols, j % 3 == 0, [1.0, 0.25][j % 2]))
    parts = [torch.randn(P * stride + off, generator=g).to(DEV) for P, L, stride, off, *_ in specs]
    outs0 = [torch.randn(((L + cols - 1) // cols) * (cols + 2), generator=g).to(DEV)
             for P, L, stride, off, cols, *_ in specs]
    res = []
    for vec in (0, 1):
        prev = _lib.query("ncf_reduce_set_vec", vec)
        try:
            lst = _lib.ReduceList()
            outs = [o.clone() for o in outs0]
            for (P, L, stride, off, cols, acc, scale), part, out in zip(specs, parts, outs):
                d = lst.d[lst.count]
                d.part, d.out, d.stride, d.ldo = part.data_ptr() + 4 * off, out.data_ptr(), stride, cols + 2
                d.L, d.cols, d.P, d.accumulate, d.scale = L, cols, P, int(acc), scale
                lst.count += 1
            scr = torch.empty(max(1, _lib.query("ncf_reduce_batch_scratch", lst.address)), device=DEV)
            _lib.call("ncf_reduce_batch", lst.address, scr.data_ptr(), scr.numel(), _lib.stream_ptr(DEV))
            torch.cuda.synchronize()
            res.append(outs)
        finally:
            _lib.query("ncf_reduce_set_vec", prev)
    for k, (a, *b) in enumerate(zip(*res)):
        assert all(torch.equal(a, x) for x in b), (k, specs[k])
    P, L, stride, off, cols, acc, scale = specs[1]      # and the sums themselves
    s = parts[1][:P * stride].view(P, stride)[:, :L].double().sum(0).cpu() * scale
    np.testing.assert_allclose(res[1][1].cpu().double().view(-1, cols + 2)[:, :cols].reshape(-1)[:L]
                               .numpy(), s.numpy(), rtol=1e-5, atol=1e-4)


def test_embedding_bwd_segment_reduce():
    """Sort + segment-reduce + LN backward against a torch fp64 index_add reference, with heavy
    duplication (one id repeated 3000x), empty tables rows and 3 radix passes."""
    from ncf_amd import _lib
    n, D, U, I = 9000, 64, 300000, 70000
    g = torch.Generator().manual_seed(5)
    uid = torch.randint(0, U, (n,), generator=g)
    uid[:3000] = 123456
    iid = (torch.rand(n, generator=g) ** 4 * I).long()
    tabs = {k: torch.randn(U if "u" in k else I, D, generator=g) * 0.1 for k in ("mfu", "mlpu", "mfi", "mlpi")}
    dys = {k: torch.randn(n, D, generator=g) for k in ("mfu", "mlpu", "mfi", "mlpi")}
    gm, gl = torch.randn(D, generator=g), torch.randn(D, generator=g)
    d = {k: v.to(DEV) for k, v in {**tabs, **{"d" + k: v for k, v in dys.items()}}.items()}
    G = {k: torch.zeros(n, D, device=DEV) for k in ("mfu", "mlpu", "mfi", "mlpi")}
    uu = torch.empty(n, dtype=torch.int64, device=DEV)
    ui = torch.empty(n, dtype=torch.int64, device=DEV)
    su = torch.full((U,), -1, dtype=torch.int32, device=DEV)
    si = torch.full((I,), -1, dtype=torch.int32, device=DEV)
    nu = torch.zeros(2, dtype=torch.int32, device=DEV)
    pg = [torch.empty(D, device=DEV) for _ in range(4)]
    ws = torch.empty(_lib.query("ncf_embedding_bwd_workspace", n, D), dtype=torch.uint8, device=DEV)
    ud, idd, gmd, gld = uid.to(DEV), iid.to(DEV), gm.to(DEV), gl.to(DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    _lib.call("ncf_embedding_bwd", P(ud), P(idd), n, D, U, I, P(d["dmfu"]), P(d["dmlpu"]),
              P(d["dmfi"]), P(d["dmlpi"]), P(d["mfu"]), P(d["mlpu"]), P(d["mfi"]), P(d["mlpi"]),
              P(gmd), P(gld), 1e-5, P(G["mfu"]), P(G["mlpu"]), P(G["mfi"]), P(G["mlpi"]), P(uu),
              P(ui), P(su), P(si), P(nu), P(pg[0]), P(pg[1]), P(pg[2]), P(pg[3]), P(ws), ws.numel(),
              _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    # reference: autograd through gather + LayerNorm in fp64
    def ref(tab, ids, dy, gamma):
        t = tab.double().requires_grad_(True)
        gam = gamma.double().requires_grad_(True)
        bet = torch.zeros(D, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.layer_norm(t[ids], (D,), gam, bet, 1e-5)
        y.backward(dy.double())
        return t.grad, gam.grad, bet.grad
    nun = nu.cpu().tolist()
    uq = torch.unique(uid)
    iq = torch.unique(iid)
    assert nun == [uq.numel(), iq.numel()]
    assert torch.equal(uu[:nun[0]].cpu(), uq) and torch.equal(ui[:nun[1]].cpu(), iq)
    assert torch.equal(su[uq.to(DEV)].cpu(), torch.arange(uq.numel(), dtype=torch.int32))
    gsum = [torch.zeros(D, dtype=torch.float64) for _ in range(4)]
    for k, ids, uniq, gi in (("mfu", uid, uq, 0), ("mlpu", uid, uq, 2), ("mfi", iid, iq, 0), ("mlpi", iid, iq, 2)):
        gt, gg, gb = ref(tabs[k], ids, dys[k], gm if k.startswith("mf") and not k.startswith("mlp") else gl)
        got = G[k][:uniq.numel()].cpu().double()
        np.testing.assert_allclose(got.numpy(), gt[uniq].numpy(), rtol=1e-4, atol=1e-4, err_msg=k)
        gsum[gi] += gg
        gsum[gi + 1] += gb
    for j in range(4):
        np.testing.assert_allclose(pg[j].cpu().double().numpy(), gsum[j].numpy(), rtol=1e-4, atol=1e-3)
    # slot reset restores the all -1 invariant
    _lib.call("ncf_slot_reset", P(uu), P(nu), 0, P(su), n, _lib.stream_ptr(DEV))
    _lib.call("ncf_slot_reset", P(ui), P(nu), 1, P(si), n, _lib.stream_ptr(DEV))
    assert int((su != -1).sum()) == 0 and int((si != -1).sum()) == 0


def test_adam_table_kernel_matches_torch():
    from ncf_amd import _lib
    rows, D = 1000, 64
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(rows, D, generator=g)
    touched = torch.tensor([3, 17, 999, 500])
    grad = torch.zeros(rows, D)
    Gc = torch.randn(4, D, generator=g)
    grad[touched] = Gc
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-3, weight_decay=1e-5)
    p = p0.clone().to(DEV)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    slot = torch.full((rows,), -1, dtype=torch.int32)
    slot[touched] = torch.arange(4, dtype=torch.int32)
    slot, Gd = slot.to(DEV), Gc.to(DEV)
    for step in (1, 2, 3):
        p_ref.grad = grad.clone()
        opt.step()
        _lib.call("ncf_adam_table", p.data_ptr(), m.data_ptr(), v.data_ptr(), rows, D,
                  slot.data_ptr(), Gd.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 1e-5, float(step),
                  _lib.stream_ptr(DEV))
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.detach().numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(m.cpu().numpy(), opt.state[p_ref]["exp_avg"].numpy(), atol=1e-9, rtol=1e-5)


# ----------------------------------------------------------------------------- behaviour
def test_dropout_statistics(monkeypatch):
    # per-layer weight-gradient launches: the forward then saves the dropped activations a
    # (the fused tower backward recomputes them instead)
    monkeypatch.setattr(_E, "MLP_WGRAD", False)
    torch.manual_seed(0)
    m = ncf.AdvancedNCF(1000, 500, 5, 24, dropout=0.2).to(DEV)
    n = 4096 * 5
    u = torch.randint(0, 1000, (4096,)).repeat_interleave(5)
    i = torch.randint(0, 500, (n,))
    m.train()
    k = kjt(u, i)
    a = m(k).detach()
    b = m(k).detach()
    assert not torch.equal(a, b)             # fresh masks per forward
    m.eval()
    with torch.no_grad():
        e1 = m(kjt(u[:100], i[:100]))
        e2 = m(kjt(u[:100], i[:100]))
    assert torch.equal(e1, e2)               # eval is deterministic
    # keep rate of the MLP dropout: count exact zeros in a dropped LN output
    w = m.engine.ws[(n, 5, True)]
    frac = (w.a[0] == 0).float().mean().item()
    assert abs(frac - 0.2) < 0.01, frac


def test_out_of_range_id_raises():
    m = ncf.AdvancedNCF(10, 10, 5, 24).to(DEV)
    m.eval()
    with pytest.raises(IndexError):
        with torch.no_grad():
            m(kjt([1, 2], [3, 10]))


def test_batch_not_multiple_of_group():
    m = ncf.AdvancedNCF(10, 10, 5, 24).to(DEV)
    m.train()
    with pytest.raises(RuntimeError, match="multiple"):
        m(kjt([1, 2, 3], [3, 4, 5]))


def test_non_adam_optimizer_gets_dense_table_grads(f2):
    g = f2
    U, I, D, Tt, H, B, M, steps = [int(x) for x in g["cfg"]]
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, Tt, [256, 128, 64], H, 0.0, M - 1)
    m.load_state_dict(T(sub(g, "init/")), strict=True)
    m = m.to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    m.train()
    out = m(kjt(g["step0/user_ids"], g["step0/item_ids"]))
    loss = torch.nn.BCELoss()(out, torch.from_numpy(g["step0/targets"]).to(DEV))
    opt.zero_grad()
    loss.backward()
    opt.step()
    k = "mf_embedding_collection.embedding_bags.user_id.weight"
    exp = g["init/" + k] - 0.1 * g["grad0/" + k]
    np.testing.assert_allclose(m.state_dict()[k].cpu().numpy(), exp, atol=1e-6)


# ----------------------------------------------------------------------------- deferred Adam
def _fused_run(deferred, steps, sweep_every=64, U=3000, I=500, B=64, seed=11, dropout=0.0,
               lr_at=None, on_step=None, pipelined=False, D=64, hidden=(256, 128, 64), H=4, **kw):
    """``pipelined``: every step is told the next batch (FusedTrainStep(next=...): the id sort
    and the early catch-up of the next batch's rows run a step ahead on the side stream).
    ``D``, ``hidden``, ``H``: the embedding width of both collections, the tower, the heads."""
    from ncf_amd.trainer import FusedTrainStep
    torch.manual_seed(seed)
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, 32, list(hidden), H, dropout, 4).to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, deferred=deferred, sweep_every=sweep_every,
                          **kw)
    g = torch.Generator().manual_seed(seed + 1)
    batches = []
    for s in range(steps):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(5).to(DEV)
        i = torch.randint(0, I, (B * 5,), generator=g).to(DEV)
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        batches.append((u, i, t.reshape(-1, 1).to(DEV)))
    for s, (u, i, t) in enumerate(batches):
        if lr_at and s in lr_at:
            step.lr = lr_at[s]          # (a scheduler's change between steps)
        nxt = batches[s + 1][:2] if pipelined and s + 1 < steps else None
        step(u, i, t, next=nxt)
        if on_step is not None:
            on_step(step, s)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}   # syncs deferred rows
    step.sync()
    mom = {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone()) for k, v in step.state.items()}
    return sd, mom


@pytest.mark.parametrize("D,H,M,B", [(64, 4, 5, 37), (64, 1, 5, 16), (64, 8, 3, 50), (64, 2, 6, 33),
                                     (64, 4, 1, 20), (128, 4, 5, 37), (128, 8, 6, 19),
                                     (128, 2, 3, 41), (128, 4, 1, 9)])
def test_attn_block_matches_unfused(monkeypatch, D, H, M, B):
    """The one-launch attention block (attn_block.hip) vs the unfused launches (projection
    GEMMs + attention.hip core), dropout on (same stream): one fused train step's probabilities,
    dense gradients and compact table gradients agree to the grads tolerance.  B not a multiple
    of the 16-group (D = 64) / 8-group (D = 128, C4) tile exercises the ragged last workgroup;
    D = 128 with M = 5 also has zero padding rows inside every tile (40 rows in 3 row tiles)."""
    from ncf_amd.trainer import FusedTrainStep
    out = []
    for flag in ("0", "1"):
        monkeypatch.setattr(_E, "ATTN_BLOCK", (flag) == "1")
        torch.manual_seed(21)
        m = ncf.AdvancedNCF(400, 300, 5, 24, D, D, 32, [256, 128, 64], H, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        assert m.engine.attn_block(D, H, M) == (flag == "1")
        g = torch.Generator().manual_seed(22)
        u = torch.randint(0, 400, (B,), generator=g).repeat_interleave(M).to(DEV)
        i = torch.randint(0, 300, (B * M,), generator=g).to(DEV)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        w = step(u, i, t.reshape(-1, 1).to(DEV))
        torch.cuda.synchronize()
        nu = w.num_unique.cpu().tolist()   # compact rows in use: [users, items]
        out.append((w.prob.cpu().clone(), m.engine.flat_grad.cpu().clone(),
                    {k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone() for k, v in w.G.items()},
                    w.y.cpu().clone()))
    (p0, g0, G0, y0), (p1, g1, G1, y1) = out
    torch.testing.assert_close(y1, y0, rtol=0, atol=2e-6)
    torch.testing.assert_close(p1, p0, rtol=0, atol=2e-6)
    torch.testing.assert_close(g1, g0, rtol=1e-4, atol=1e-6)
    for k in G0:
        torch.testing.assert_close(G1[k], G0[k], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("D,H,M,B,drop", [(64, 4, 5, 37, 0.2), (64, 1, 5, 16, 0.2),
                                           (64, 8, 3, 50, 0.2), (64, 2, 6, 33, 0.0),
                                           (64, 4, 1, 20, 0.2), (128, 4, 5, 37, 0.2),
                                           (128, 8, 6, 19, 0.0)])
def test_attn_block_recompute_bitwise_equals_stash(monkeypatch, D, H, M, B, drop):
    """The recompute backward (ncf_attn_block_bwd_rc: q/k/v re-projected and the core forward
    re-run in LDS, nothing stashed by the forward) against the stashing form: same code for the
    projections and the core, so the step's probabilities, every dense gradient and the compact
    table gradients are bit-identical, dropout on, ragged last workgroup."""
    from ncf_amd.trainer import FusedTrainStep
    out = []
    for flag in ("0", "1"):
        monkeypatch.setattr(_E, "ATTN_RC", (flag) == "1")
        torch.manual_seed(23)
        m = ncf.AdvancedNCF(400, 300, 5, 24, D, D, 32, [256, 128, 64], H, drop, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        assert m.engine.attn_rc(D, H, M) == (flag == "1")
        g = torch.Generator().manual_seed(24)
        u = torch.randint(0, 400, (B,), generator=g).repeat_interleave(M).to(DEV)
        i = torch.randint(0, 300, (B * M,), generator=g).to(DEV)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        for _ in range(2):
            w = step(u, i, t.reshape(-1, 1).to(DEV))
        torch.cuda.synchronize()
        nu = w.num_unique.cpu().tolist()
        out.append((w.prob.cpu().clone(), m.engine.flat_grad.cpu().clone(),
                    {k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone() for k, v in w.G.items()},
                    {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (p0, g0, G0, s0), (p1, g1, G1, s1) = out
    assert torch.equal(p0, p1)
    assert torch.equal(g0, g1)
    for k in G0:
        assert torch.equal(G0[k], G1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


@pytest.mark.parametrize("D,H,M,B,uniform,rc", [(64, 4, 5, 37, True, "0"), (64, 4, 5, 37, True, "1"),
                                               (128, 4, 5, 19, True, "0"),
                                               (64, 4, 5, 37, False, "0"),
                                               (64, 2, 3, 50, True, "1")])
def test_attn_shared_q_matches_per_row(monkeypatch, D, H, M, B, uniform, rc):
    """Q projected once per interaction group (fact 6: the M rows of a group hold one user;
    attn_block.hip groups_uniform / put_tile_expand) against every row projected
    (engine.ATTN_SHARE_Q = False): same probabilities, gradients and table gradients.  With one
    user per group the workgroups take the shared path; with a random user per row
    (uniform=False) none does.  Both backward forms (stash, recompute)."""
    import ncf_amd.engine as E
    from ncf_amd.trainer import FusedTrainStep
    monkeypatch.setattr(_E, "ATTN_RC", (rc) == "1")
    out = []
    for flag in (False, True):
        monkeypatch.setattr(E, "ATTN_SHARE_Q", flag)
        torch.manual_seed(41)
        m = ncf.AdvancedNCF(400, 300, 5, 24, D, D, 32, [256, 128, 64], H, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        g = torch.Generator().manual_seed(42)
        if uniform:
            u = torch.randint(0, 400, (B,), generator=g).repeat_interleave(M).to(DEV)
        else:
            u = torch.randint(0, 400, (B * M,), generator=g).to(DEV)
        i = torch.randint(0, 300, (B * M,), generator=g).to(DEV)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        for _ in range(2):
            w = step(u, i, t.reshape(-1, 1).to(DEV))
        torch.cuda.synchronize()
        nu = w.num_unique.cpu().tolist()
        out.append((w.prob.cpu().clone(), m.engine.flat_grad.cpu().clone(),
                    {k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone() for k, v in w.G.items()}))
    (p0, g0, G0), (p1, g1, G1) = out
    print(f"shared Q D={D} uniform={uniform} rc={rc}: bitwise prob {torch.equal(p0, p1)} "
          f"grad {torch.equal(g0, g1)}; max |dprob| {(p1 - p0).abs().max().item():.3g}")
    torch.testing.assert_close(p1, p0, rtol=0, atol=1e-6)
    torch.testing.assert_close(g1, g0, rtol=1e-4, atol=1e-6)
    for k in G0:
        torch.testing.assert_close(G1[k], G0[k], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("wgrad", ["1", "0"])
@pytest.mark.parametrize("B,drop,D", [(37, 0.2, 64), (64, 0.0, 64), (1, 0.2, 64), (300, 0.2, 64),
                                      (37, 0.2, 128), (64, 0.0, 128), (300, 0.2, 128)])
@pytest.mark.parametrize("split", [True, False])
def test_mlp_tower_matches_unfused(monkeypatch, B, drop, D, wgrad, split):
    """The one-launch MLP tower (mlp_tower.hip, forward + backward) vs the per-layer launches
    (GEMM + rowops + head), same dropout stream: probabilities, saved activations, dense and
    compact table gradients agree to the grads tolerance; n = 5B rows not a multiple of the
    32-row tile exercises the ragged last workgroup.  D = 128 is C4's input width.  ``split``:
    the fused tower's Linears on split-operand bf16 MFMA (engine.TOWER_SPLIT) or fp32 MFMA."""
    import ncf_amd.engine as E
    from ncf_amd.trainer import FusedTrainStep
    monkeypatch.setattr(E, "TOWER_SPLIT", split)
    # (the tower's own launch: fused behind the attention block its dy never reaches HBM;
    # test_attn_tower_fused_bitwise_equals_two_launches holds that form to this one)
    monkeypatch.setattr(E, "FUSE_ATTN_TOWER", False)
    out = []
    monkeypatch.setattr(_E, "MLP_WGRAD", (wgrad) == "1")
    for flag in ("0", "1"):
        monkeypatch.setattr(_E, "MLP_FUSED", (flag) == "1")
        torch.manual_seed(31)
        m = ncf.AdvancedNCF(400, 300, 5, 24, D, D, 32, [256, 128, 64], 4, drop, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        assert m.engine.mlp_fused(D, [256, 128, 64]) == (flag == "1")
        g = torch.Generator().manual_seed(32)
        u = torch.randint(0, 400, (B,), generator=g).repeat_interleave(5).to(DEV)
        i = torch.randint(0, 300, (B * 5,), generator=g).to(DEV)
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        w = step(u, i, t.reshape(-1, 1).to(DEV))
        torch.cuda.synchronize()
        nu = w.num_unique.cpu().tolist()
        out.append(dict(prob=w.prob.cpu().clone(), mlp=w.mlp_pred.cpu().clone(),
                        loss=w.loss.cpu().clone(), dumf=w.dumf.cpu().clone(),
                        grad=m.engine.flat_grad.cpu().clone(), dy=w.dy.cpu().clone(),
                        a=[x.cpu().clone() for x in w.a], r=[x.cpu().clone() for x in w.r],
                        G={k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone()
                           for k, v in w.G.items()}))
    a, b = out
    for k in ("prob", "mlp"):
        torch.testing.assert_close(b[k], a[k], rtol=0, atol=2e-6)
    torch.testing.assert_close(b["loss"], a["loss"], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(b["dumf"], a["dumf"], rtol=1e-4, atol=1e-7)
    # with the weight gradients fused, the tower forward does not save a (its backward
    # recomputes it from r), so a is compared only on the per-layer weight-gradient path
    acts = (lambda o: o["r"] + o["a"]) if wgrad == "0" else (lambda o: o["r"])
    for x, y in zip(acts(b), acts(a)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(b["dy"], a["dy"], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(b["grad"], a["grad"], rtol=1e-4, atol=1e-6)
    for k in a["G"]:
        torch.testing.assert_close(b["G"][k], a["G"][k], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("D", [64, 128])
def test_mlp_tower_split_matches_fp32_mfma(monkeypatch, D):
    """The fused tower on split-operand bf16 MFMA (ncf_mlp_fwd_split / ncf_mlp_bwd_split: x =
    h + m + l in bf16, six products per fp32 product) against the same tower on fp32 MFMA, with
    dropout.  The first step (same weights): probabilities, loss, the saved pre-LN rows, dense
    and compact table gradients at fp32 rounding distance (much tighter than the grads
    tolerance).  The second step runs on weights one Adam step apart, where Adam turns rounding
    noise in near-zero gradients into +-lr moves: held to the F2 tolerances."""
    import ncf_amd.engine as E
    from ncf_amd.trainer import FusedTrainStep
    out = []
    for split in (False, True):
        monkeypatch.setattr(E, "TOWER_SPLIT", split)
        torch.manual_seed(71)
        m = ncf.AdvancedNCF(600, 400, 5, 24, D, D, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        g = torch.Generator().manual_seed(72)
        rec = []
        for _ in range(2):
            u = torch.randint(0, 600, (77,), generator=g).repeat_interleave(5).to(DEV)
            i = torch.randint(0, 400, (385,), generator=g).to(DEV)
            t = torch.zeros(77, 5)
            t[:, 0] = 1
            w = step(u, i, t.reshape(-1, 1).to(DEV))
            torch.cuda.synchronize()
            nu = w.num_unique.cpu().tolist()
            rec.append(dict(prob=w.prob.cpu().clone(), loss=w.loss.cpu().clone(),
                            r=[x.cpu().clone() for x in w.r],
                            grad=m.engine.flat_grad.cpu().clone(),
                            G={k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone()
                               for k, v in w.G.items()}))
        out.append(rec)
    for s_, (a, b) in enumerate(zip(out[0], out[1])):
        dp = (b["prob"] - a["prob"]).abs().max().item()
        dg = (b["grad"] - a["grad"]).abs().max().item()
        print(f"split vs fp32 MFMA D={D} step {s_}: |dprob| {dp:.3g}, max |dgrad| {dg:.3g}")
        tight = s_ == 0
        # (step 1: after one Adam step the two roundings' sign-flip zone elements have moved
        # +-lr apart — measured up to 2.1e-6 at D = 128)
        torch.testing.assert_close(b["prob"], a["prob"], rtol=0, atol=5e-7 if tight else 1e-5)
        torch.testing.assert_close(b["loss"], a["loss"], rtol=1e-6, atol=1e-7)
        for x, y in zip(b["r"], a["r"]):
            torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6 if tight else 1e-4)
        torch.testing.assert_close(b["grad"], a["grad"], rtol=2e-5 if tight else 1e-4,
                                   atol=1e-7 if tight else 1e-6)
        for k in a["G"]:
            torch.testing.assert_close(b["G"][k], a["G"][k], rtol=2e-5 if tight else 1e-4,
                                       atol=1e-8 if tight else 1e-6)


@pytest.mark.parametrize("tables", ["fp32", "bf16"])
def test_attn_tower_fused_bitwise_equals_two_launches(monkeypatch, tables):
    """The attention block and the MLP tower as one launch per direction (tower_fused.hip:
    ncf_attn_mlp_fwd hands the attention's output to the tower in LDS, ncf_attn_mlp_bwd the
    tower's input gradient to the attention backward) against the two launches each way
    (ncf_attn_block_fwd -> y -> ncf_mlp_fwd; ncf_mlp_bwd -> dy -> ncf_attn_block_bwd): the same
    device code, so the same bits — probabilities, parameters and Adam moments over 6 training
    steps with dropout and a ragged last workgroup (B = 61 groups), and with bf16 tables
    (single-term bf16 tower)."""
    import ncf_amd.engine as E
    from ncf_amd.trainer import FusedTrainStep
    monkeypatch.setattr(E, "SMALL_TILE_GROUPS", 0)     # (80-row tiles, as the two launches)
    U, I, B, M = 3000, 500, 61, 5
    g = torch.Generator().manual_seed(81)
    batches = []
    for _ in range(6):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = torch.randint(0, I, (B * M,), generator=g)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        batches.append((u.to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)))
    out = []
    for fused in (True, False):
        monkeypatch.setattr(E, "FUSE_ATTN_TOWER", fused)
        torch.manual_seed(82)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5,
                              table_dtype=torch.bfloat16 if tables == "bf16" else torch.float32)
        assert m.engine.attn_mlp_fused(64, 4, M, [256, 128, 64]) == fused
        probs = []
        for u, i, t in batches:
            w = step(u, i, t)
            probs.append(w.prob.cpu().clone())
        step.sync()
        out.append((probs, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
                     for k, v in step.state.items()}))
    (pa, sa, ma), (pb, sb, mb) = out
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for k in ma:
        assert torch.equal(ma[k][0], mb[k][0]) and torch.equal(ma[k][1], mb[k][1]), k


@pytest.mark.parametrize("B", [256, 61, 7])
def test_small_batch_tiles_vs_80_row_tiles(monkeypatch, B):
    """The fused attention + tower in small-batch tiles (tower_fused_small.hip: 3 groups = 15 rows
    per workgroup; engine.SMALL_TILE_GROUPS) against the 80-row tiles on the same batches: the
    forward's probabilities bit for bit, the first backward's compact table gradients and dense
    gradients to fp32 rounding (row-tile GEMMs of another tile count, partial sums of another
    grouping), and 4 training steps (dropout on, B = 256: the
    reference's default batch, config.yaml:65; 61 and 7: ragged last workgroups) to 1e-6."""
    import ncf_amd.engine as E
    from ncf_amd.trainer import FusedTrainStep
    U, I, M = 3000, 500, 5
    g = torch.Generator().manual_seed(B)
    batches = []
    for _ in range(4):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = (torch.rand(B * M, generator=g) ** 2 * I).long()
        t = torch.zeros(B, M)
        t[:, 0] = 1
        batches.append((u.to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)))
    out = []
    for small in (True, False):
        monkeypatch.setattr(E, "SMALL_TILE_GROUPS", 1 << 30 if small else 0)
        torch.manual_seed(91)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        probs, first = [], None
        for s_, (u, i, t) in enumerate(batches):
            w = step(u, i, t)
            probs.append(w.prob.cpu().clone())
            if s_ == 0:
                torch.cuda.synchronize()
                nu = w.num_unique.cpu().tolist()
                first = ({k: v[:nu[0 if k.endswith("user") else 1]].cpu().clone()
                          for k, v in w.G.items()}, m.engine.flat_grad.cpu().clone())
        step.sync()
        out.append((probs, first, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (pa, (ga, fa), sa), (pb, (gb, fb), sb) = out
    assert torch.equal(pa[0], pb[0])
    for k in ga:   # (the MLP rows' input gradients go through the tower's and the attention's
        #            row-tile GEMMs, whose tile count differs: fp32 rounding, not bits)
        torch.testing.assert_close(ga[k], gb[k], rtol=1e-5, atol=1e-8, msg=k)
    torch.testing.assert_close(fa, fb, rtol=1e-5, atol=1e-7)
    for x, y in zip(pa, pb):
        torch.testing.assert_close(x, y, rtol=0, atol=1e-6)
    # parameters: Adam's first steps are lr x sign(g), so an element whose gradient is summation
    # noise (e.g. k_proj.bias, exactly 0 in exact arithmetic) may step either way in the two runs
    # (at most 2 lr per step apart); every other element agrees to 1e-5
    for k in sa:
        d = (sa[k] - sb[k]).abs()
        assert d.max().item() <= 4 * 2e-3 + 1e-6, k
        assert (d > 1e-5).float().mean().item() < 0.02, k


def test_mlp_tower_eval_matches_unfused(monkeypatch):
    res = []
    for flag in ("0", "1"):
        monkeypatch.setattr(_E, "MLP_FUSED", (flag) == "1")
        torch.manual_seed(33)
        m = ncf.AdvancedNCF(300, 200, 5, 24).to(DEV).eval()
        u = torch.randint(0, 300, (1001,), device=DEV)
        i = torch.randint(0, 200, (1001,), device=DEV)
        with torch.no_grad():
            res.append(m.forward_simple(u, i).cpu())
    torch.testing.assert_close(res[1], res[0], rtol=0, atol=2e-6)


def test_attn_block_eval_forward_matches_unfused(monkeypatch):
    """Eval (M = 1): the block's no-core form (o = v) vs the unfused v/out projections."""
    res = []
    for flag in ("0", "1"):
        monkeypatch.setattr(_E, "ATTN_BLOCK", (flag) == "1")
        torch.manual_seed(23)
        m = ncf.AdvancedNCF(300, 200, 5, 24).to(DEV).eval()
        u = torch.randint(0, 300, (1000,), device=DEV)
        i = torch.randint(0, 200, (1000,), device=DEV)
        with torch.no_grad():
            res.append(m.forward_simple(u, i).cpu())
    torch.testing.assert_close(res[1], res[0], rtol=0, atol=2e-6)


@pytest.mark.parametrize("sweep_every,steps", [(64, 70), (128, 140), (0, 70)])
def test_deferred_adam_bitwise_equals_dense(sweep_every, steps):
    """The deferred schedule reproduces the dense-exact sweep bit for bit (crossing a periodic
    sweep at 64 / at 128, FusedTrainStep's default; sweep_every=0 exercises long catch-up chains
    only)."""
    a_sd, a_m = _fused_run(False, steps)
    b_sd, b_m = _fused_run(True, steps, sweep_every=sweep_every)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


@pytest.mark.parametrize("D,H,hidden", [(16, 1, (64, 32)), (32, 2, (256, 128, 64)),
                                        (128, 4, (256, 128, 64)), (256, 4, (256, 128, 64))])
def test_deferred_adam_bitwise_equals_dense_other_widths(D, H, hidden):
    """The deferred + clock schedule against the dense sweep, bit for bit, at the other widths
    NCF_DISPATCH_DIM takes: 24 steps across three rounds of the rolling sweep (sweep_every = 8).
    D < 64 shares a wave among 4 or 2 rows in the replay, D = 256 gives a lane 4 columns.
    FusedTrainStep(deferred=True) refuses none of the four: trainer.py refuses only
    mf_embedding_dim != mlp_embedding_dim, and engine.py sends a tower or an attention shape the
    fused kernels do not take down the per-layer path (head dims 16, 16, 32, 64 here)."""
    kw = dict(U=700, I=300, D=D, H=H, hidden=hidden)
    a_sd, a_m = _fused_run(False, 24, **kw)
    b_sd, b_m = _fused_run(True, 24, sweep_every=8, clock=True, **kw)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_clock_mode_bitwise_equals_dense():
    """The step-clock form of the deferred schedule (every step value read on the device) is
    still bit-identical to the dense sweep."""
    a_sd, a_m = _fused_run(False, 70)
    b_sd, b_m = _fused_run(True, 70, clock=True)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


@pytest.mark.parametrize("tables", ["fp32", "bf16"])
def test_early_catchup_bitwise_equals_dense(monkeypatch, tables):
    """The next batch's rows caught up a step ahead on the side stream (deferred.EARLY_CATCHUP:
    this step's rows locked by its catch-up, NCF_STAMP_LOCK, and skipped) against the dense
    sweep, bit for bit, parameters and both moments, over 40 steps of heavily overlapping
    batches (400 users, 150 items: most rows of a batch are in the previous one too) with a
    rolling sweep every 4 steps crossing the locked rows; the early catch-up must have run on
    every step but the last.  bf16 tables: against the same pipelined schedule without the
    early catch-up (the dense bf16 sweep leaves the fp32 parameter copies stale)."""
    import ncf_amd.deferred as Dm
    ran = []
    orig = Dm.DeferredTableAdam.early_catchup

    def count(self, *a):
        r = orig(self, *a)
        ran.append(r)
        return r
    monkeypatch.setattr(Dm.DeferredTableAdam, "early_catchup", count)
    dt = torch.bfloat16 if tables == "bf16" else torch.float32
    kw = dict(sweep_every=4, U=400, I=150, pipelined=True, clock=True, overlap_sweep=True,
              table_dtype=dt)
    if tables == "bf16":
        monkeypatch.setattr(Dm, "EARLY_CATCHUP", False)
        a_sd, a_m = _fused_run(True, 40, **kw)
        assert not any(ran)
    else:
        a_sd, a_m = _fused_run(False, 40, U=400, I=150)
    monkeypatch.setattr(Dm, "EARLY_CATCHUP", True)     # (on by default below 10,240 rows)
    b_sd, b_m = _fused_run(True, 40, **kw)
    assert sum(ran) >= 38, ran
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_early_reduce_bitwise_equals_dense(monkeypatch):
    """The fused backward's dense-gradient reductions on the sweep's side stream
    (trainer.EARLY_REDUCE, off by default) against the dense sweep, bit for bit."""
    import ncf_amd.trainer as Tr
    monkeypatch.setattr(Tr, "EARLY_REDUCE", True)
    a_sd, a_m = _fused_run(False, 30)
    b_sd, b_m = _fused_run(True, 30, clock=True, overlap_sweep=True, pipelined=True)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


@pytest.mark.parametrize("tables", ["fp32", "bf16"])
def test_fused_apply_bitwise_equals_separate_apply(monkeypatch, tables):
    """The table Adam's apply fused into the embedding backward (trainer.FUSE_APPLY,
    ncf_embedding_bwd_reduce_apply_clock: single-piece segments step in the reduce, longer ones in
    the fix-up) against the separate ncf_adam_pairs_apply_clock launch, bit for bit: 24 steps with
    dropout, the overlapped sweep every 8 steps, the pipelined sort, hot items (40 of them: long
    multi-piece segments) and fp32 / bf16 tables."""
    import ncf_amd.trainer as Tr
    out = []
    for fuse in (False, True):
        monkeypatch.setattr(Tr, "FUSE_APPLY", fuse)
        out.append(_fused_run(True, 24, sweep_every=8, I=40, dropout=0.2, clock=True,
                              overlap_sweep=True, pipelined=True,
                              table_dtype=torch.bfloat16 if tables == "bf16" else torch.float32))
    (a_sd, a_m), (b_sd, b_m) = out
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_late_catchup_bitwise_equals_dense(monkeypatch):
    """The next batch's catch-up queued behind this step's fused table apply, beside the
    dense-gradient reductions (deferred.LATE_CATCHUP), and the next step skipping its own
    catch-up, against the dense schedule bit for bit (dropout, sweep every 8 steps); and against
    the late catch-up off.  The skip must have happened on every step but the first (deferred
    late_skips), with the sweep forked at the default point of this geometry and in the backward
    ("mlp_bwd": the prefetch, and the late catch-up, queued after the forward)."""
    import ncf_amd.deferred as Dm
    import ncf_amd.trainer as Tr
    monkeypatch.setattr(Tr, "FUSE_APPLY", True)
    monkeypatch.setattr(Dm, "EARLY_CATCHUP", False)     # (on by default at this batch size)
    seen = []
    orig = Dm.DeferredTableAdam.prepare

    def prep(self, *a):
        seen.append(self)
        return orig(self, *a)
    monkeypatch.setattr(Dm.DeferredTableAdam, "prepare", prep)

    def run(late, **kw):
        seen.clear()
        monkeypatch.setattr(Dm, "LATE_CATCHUP", late)
        out = _fused_run(True, 30, sweep_every=8, clock=True, overlap_sweep=True, pipelined=True,
                         **kw)
        skips = max(d.late_skips for d in seen)
        assert (skips >= 28) if late else skips == 0, (late, kw, skips)
        return out
    pairs = []
    for drop in (0.2, 0.0):
        pairs.append([run(late, dropout=drop) for late in (True, False)])
    pairs.append([pairs[1][0], _fused_run(False, 30)])   # (the dense schedule: no dropout)
    monkeypatch.setattr(Dm, "SWEEP_FORK", "mlp_bwd")    # the prefetch inside the backward
    pairs.append([pairs[0][0], run(True, dropout=0.2)])
    for (b_sd, b_m), (a_sd, a_m) in pairs:
        for k in a_sd:
            assert torch.equal(a_sd[k], b_sd[k]), k
        for k in a_m:
            assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_eager_on_fresh_step():
    """FusedTrainStep.eager() as the first call ever on a step (no __call__ before it: the late
    catch-up hand-over starts empty) against a twin whose first call was step(): parameters and
    Adam moments bit for bit, after that call and two ordinary steps (dropout on, B = 61 groups
    of 5: the last workgroup ragged)."""
    from ncf_amd.trainer import FusedTrainStep
    U, I, B = 3000, 500, 61
    g = torch.Generator().manual_seed(29)
    batches = []
    for _ in range(3):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(5).to(DEV)
        i = torch.randint(0, I, (B * 5,), generator=g).to(DEV)
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        batches.append((u, i, t.reshape(-1, 1).to(DEV)))
    out = []
    for eager in (True, False):
        torch.manual_seed(13)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        (step.eager if eager else step)(*batches[0])
        for u, i, t in batches[1:]:
            step(u, i, t)
        step.sync()
        out.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
                     for k, v in step.state.items()},
                    step.m_flat.cpu().clone(), step.v_flat.cpu().clone()))
    (a_sd, a_m, a_mf, a_vf), (b_sd, b_m, b_mf, b_vf) = out
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k
    assert torch.equal(a_mf, b_mf) and torch.equal(a_vf, b_vf)


def test_pipelined_dedup_bitwise_equals_inline():
    """FusedTrainStep(next=...) sorts the next batch's ids on a side stream under the current
    step (two alternating dedup buffer sets); results are bit for bit those of the inline sort,
    including a step whose prefetch is discarded (ids not the ones announced) and a step told no
    next batch."""
    from ncf_amd.trainer import FusedTrainStep
    U, I, B = 3000, 500, 64
    g = torch.Generator().manual_seed(21)
    batches = []
    for _ in range(9):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(5).to(DEV)
        i = torch.randint(0, I, (B * 5,), generator=g).to(DEV)
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        batches.append((u, i, t.reshape(-1, 1).to(DEV)))
    out = []
    for pipe in (False, True):
        torch.manual_seed(11)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        for s_, (u, i, t) in enumerate(batches):
            if not pipe:
                step(u, i, t)
            elif s_ == 4:      # announce a different batch: the prefetch must be ignored
                step(u, i, t, next=(batches[0][0], batches[0][1]))
            elif s_ == 6:      # no next batch: the following step sorts inline
                step(u, i, t)
            else:
                nxt = batches[s_ + 1][:2] if s_ + 1 < len(batches) else None
                step(u, i, t, next=nxt)
        out.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("graph,fork", [(False, "mlp_bwd"), (True, "mlp_bwd"),
                                        (False, "tower,mlp_bwd,reduce"),
                                        (True, "tower,attn_bwd"),
                                        (False, "emb_bwd,nowhere"),
                                        (False, "gather"), (True, "gather"),
                                        (False, "off")])
def test_overlapped_sweep_bitwise_equals_dense(monkeypatch, graph, fork):
    """The overlapped rolling sweep (side stream; the default fork point is the tower
    backward, joined before the apply; or split into consecutive parts forked at several points
    (ncf_adam_pairs_sweep_rolling_part), a part whose fork point the step never passes settled
    before the apply) is bit-identical to the dense sweep, eager and hipGraph-captured ("off":
    the sweep on the step's own stream)."""
    monkeypatch.setattr(_D, "SWEEP_FORK", fork)
    a_sd, a_m = _fused_run(False, 70)
    b_sd, b_m = _fused_run(True, 70, clock=True, graph=graph, overlap_sweep=fork != "off")
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


@pytest.mark.parametrize("fuse_apply,early_reduce", [(True, False), (False, False),
                                                     (True, True), (False, True)])
@pytest.mark.parametrize("mixed", [False, True])
def test_group_rows_bitwise_equals_every_row(monkeypatch, mixed, fuse_apply, early_reduce):
    """The gather writing each group's LN'd user rows once (group_rows = M; the
    attention block and the tower's head backward reading the group's row) against every row
    written: parameters and Adam moments bit-identical over 6 FusedTrainStep steps.  ``mixed``:
    a third of the groups hold several users (those rows are their own source rows) and the last
    workgroup is ragged.  Over the schedule switches the r05y fault could have run under
    (trainer.FUSE_APPLY, trainer.EARLY_REDUCE; tests/test_gpu_guard.py audits the same paths
    for reads past any buffer's end)."""
    from ncf_amd import engine as E
    from ncf_amd import trainer as Tr
    from ncf_amd.trainer import FusedTrainStep
    monkeypatch.setattr(Tr, "FUSE_APPLY", fuse_apply)
    monkeypatch.setattr(Tr, "EARLY_REDUCE", early_reduce)
    U, I, B, M = 3000, 500, 61, 5
    g = torch.Generator().manual_seed(23)
    batches = []
    for _ in range(6):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        if mixed:
            pick = torch.rand(B * M, generator=g) < 0.1
            u = torch.where(pick & (torch.arange(B * M) % M != 0),
                            torch.randint(0, U, (B * M,), generator=g), u)
        i = torch.randint(0, I, (B * M,), generator=g)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        batches.append((u.to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)))
    out = []
    for on in (True, False):
        monkeypatch.setattr(E, "GROUP_ROWS", on)
        torch.manual_seed(24)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        for u, i, t in batches:
            step(u, i, t)
        ws = next(iter(m.engine.ws.values()))
        assert ws.group_rows == (M if on else 0)
        step.sync()
        out.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
                     for k, v in step.state.items()}))
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
    for k in out[0][1]:
        assert torch.equal(out[0][1][k][0], out[1][1][k][0]), k
        assert torch.equal(out[0][1][k][1], out[1][1][k][1]), k


def test_step_teardown_with_side_work_queued_then_new_step():
    """A FusedTrainStep dropped right after a step that queued side-stream work (the next
    batch's id sort behind the overlapped sweep, the late catch-up, the early reductions), with
    no host sync, and a second model + step built and run at once: the caching allocator hands
    the second one blocks the first one freed (same stream), so any work of the first still
    touching them would corrupt it.  The second run is bit for bit the same run made after a
    device drain.  Covers the dedup fork at the step's entry (a side stream the step does NOT
    join before it returns) as well as the default fork behind the sweep."""
    import gc
    import ncf_amd.trainer as Tr
    from ncf_amd.trainer import FusedTrainStep
    U, I, B = 3000, 500, 61

    def leave_in_flight(seed):
        torch.manual_seed(seed)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, sweep_every=8)
        g = torch.Generator().manual_seed(seed)
        bs = [(torch.randint(0, U, (B,), generator=g).repeat_interleave(5).to(DEV),
               torch.randint(0, I, (B * 5,), generator=g).to(DEV)) for _ in range(6)]
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        t = t.reshape(-1, 1).to(DEV)
        for s_ in range(5):
            step(bs[s_][0], bs[s_][1], t, next=bs[s_ + 1])   # the last prefetch never consumed

    ref = _fused_run(True, 12, sweep_every=8, B=B, seed=31, dropout=0.2, clock=True,
                     overlap_sweep=True, pipelined=True)
    for fork, early in (("sweep", False), ("entry", True)):
        old = (Tr.DEDUP_FORK, Tr.EARLY_REDUCE)
        Tr.DEDUP_FORK, Tr.EARLY_REDUCE = fork, early
        try:
            leave_in_flight(7)       # (its objects are unreachable on return: freed now)
            gc.collect()
            got = _fused_run(True, 12, sweep_every=8, B=B, seed=31, dropout=0.2, clock=True,
                             overlap_sweep=True, pipelined=True)
        finally:
            Tr.DEDUP_FORK, Tr.EARLY_REDUCE = old
        for k in ref[0]:
            assert torch.equal(ref[0][k], got[0][k]), (fork, k)
        for k in ref[1]:
            assert torch.equal(ref[1][k][0], got[1][k][0]), (fork, k)
            assert torch.equal(ref[1][k][1], got[1][k][1]), (fork, k)


def test_attn_o_recompute_bitwise_equals_o_stash(monkeypatch):
    """The attention backward recomputing O = dropout(P) V from the forward's stashed P and V
    (attn_pv, the forward's own accumulation; the forward then stashes no O) against the O
    stash: parameters and Adam moments bit-identical over 6 FusedTrainStep steps with dropout,
    the last workgroup ragged."""
    from ncf_amd import engine as E
    from ncf_amd.trainer import FusedTrainStep
    U, I, B, M = 3000, 500, 61, 5
    g = torch.Generator().manual_seed(37)
    batches = []
    for _ in range(6):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = torch.randint(0, I, (B * M,), generator=g)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        batches.append((u.to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)))
    out = []
    for stash in (True, False):
        monkeypatch.setattr(E, "_STASH_O", stash)
        torch.manual_seed(38)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, M - 1).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        for u, i, t in batches:
            step(u, i, t)
        step.sync()
        out.append(({k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
                     for k, v in step.state.items()}))
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
    for k in out[0][1]:
        assert torch.equal(out[0][1][k][0], out[1][1][k][0]), k
        assert torch.equal(out[0][1][k][1], out[1][1][k][1]), k


@pytest.mark.parametrize("mixed", [False, True])
def test_attn_stash_backward_reads_the_forwards_q_record(mixed):
    """the stash backward takes the shared-Q decision the forward recorded
    beside its per-group Q stash (attn_block.hip kQGroupTag), not the ids it is handed, so a
    backward called without user ids reads the same Q rows.  After a training forward with ids
    (one user per group; with ``mixed`` one group of the first workgroup has two users, so that
    workgroup stashes every row and the others share), the backward with the ids and with NULL
    ids give bit-identical dQ / dK / dV / dX_u / dX_i."""
    from ncf_amd import _lib
    from ncf_amd._lib import ptr
    from ncf_amd.trainer import FusedTrainStep
    U, I, B, M, D, H = 3000, 500, 45, 5, 64, 4
    g = torch.Generator().manual_seed(7)
    u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
    if mixed:
        u[3 * M + 2] = (u[3 * M] + 1) % U
    i = torch.randint(0, I, (B * M,), generator=g)
    t = torch.zeros(B, M)
    t[:, 0] = 1
    u, i, t = u.to(DEV), i.to(DEV), t.reshape(-1, 1).to(DEV)
    torch.manual_seed(3)
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, 32, [256, 128, 64], H, 0.0, M - 1).to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
    w = step(u, i, t)
    torch.cuda.synchronize()
    a = m.user_product_attention
    n = B * M
    outs = []
    for ids in (u, None):
        dq, dk, dv, dxu, dxi = (torch.full((n, D), 7.0, device=DEV) for _ in range(5))
        _lib.call("ncf_attn_block_bwd", ptr(w.dy), ptr(w.q), ptr(w.k), ptr(w.v), ptr(w.P), B, M,
                  H, D, ptr(a.q_proj.weight), ptr(a.k_proj.weight), ptr(a.v_proj.weight),
                  ptr(a.out_proj.weight), 0.0, 0, ptr(m.engine.clock), None, ptr(w.xu),
                  ptr(w.xi), None, None, 0, None, ptr(dq), ptr(dk), ptr(dv), ptr(dxu), ptr(dxi),
                  ptr(ids) if ids is not None else None, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        outs.append([x.cpu() for x in (dq, dk, dv, dxi, dxu)])
    for name, x, y in zip(("dq", "dk", "dv", "dxi", "dxu"), outs[0], outs[1]):
        assert torch.equal(x, y), name
        assert not (x == 7.0).all(dim=1).any(), name       # every row written


@pytest.mark.parametrize("D,G", [(32, 0), (64, 0), (64, 5), (128, 3), (256, 0)])
def test_gather_two_float4_lanes_bitwise_equals_one_float4(D, G):
    """k_gather_ln_gmf with D/8 lanes per row (two float4 each, the plain entry point's kernel)
    against the D/4-lane kernel (taken by the scaled entry point; scale 1 + 0 * s == 1 exactly):
    every output bit-identical, including the group-rows copy skip and out-of-range ids."""
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(D + G)
    U, I, n = 700, 300, 1003 if G == 0 else 200 * G
    uid = torch.randint(0, U, (n,), generator=g)
    if G:
        uid = uid.view(-1, G)[:, :1].repeat(1, G).reshape(-1)
        uid[G * 7 + 2] = 5          # a row that leaves its group's user
    iid = torch.randint(0, I, (n,), generator=g)
    iid[11] = I + 4                 # out of range: row 0 and the error bit
    t = lambda *s: (torch.randn(*s, generator=g) * 0.7 + 0.1).to(DEV)
    tabs = [t(U, D), t(I, D), t(U, D), t(I, D)]
    par = [t(D), t(D), t(D), t(D), t(D), t(1)]
    uid, iid = uid.to(DEV), iid.to(DEV)
    P = lambda x: x.data_ptr()
    res = []
    for scaled in (False, True):
        outs = [torch.full((n,), 7.0, device=DEV)] + [torch.full((n, D), 7.0, device=DEV)
                                                      for _ in range(4)]
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        head = [P(uid), P(iid), n, *map(P, tabs), U, I, D, *map(P, par), 1e-5]
        zs = torch.zeros(n, D, device=DEV) if scaled else None
        _lib.call("ncf_gather_ln_gmf_scaled_fwd", *head, P(zs) if scaled else 0, 0.0, G,
                  *map(P, outs), P(err), _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        res.append([o.cpu() for o in outs] + [err.cpu()])
    assert res[0][-1].item() & 1
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a,
                           b.view(torch.int32) if b.is_floating_point() else b)


def test_graph_replay_bitwise_equals_eager_clock():
    """hipGraph capture + replay of the whole training step (dropout on: the per-step stream
    comes from the device clock) == the same clock-driven steps run eagerly, bit for bit, across
    a rolling-sweep wrap (70 steps)."""
    a_sd, a_m = _fused_run(True, 70, dropout=0.2, clock=True)
    b_sd, b_m = _fused_run(True, 70, dropout=0.2, graph=True)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_graph_replay_lr_change_bitwise_equals_eager_clock():
    """An lr change between steps (ReduceLROnPlateau-style, the reference's scheduler) under
    graph=True: the per-step scalar table is refilled in place, so the captured graph keeps
    reading live scalars (or is re-captured when the buffer had to move); bit for bit the same
    as the eager clock path taking the same changes."""
    lr_at = {10: 5e-4, 40: 2.5e-4, 41: 3e-4}
    a_sd, a_m = _fused_run(True, 70, dropout=0.2, clock=True, lr_at=lr_at)
    b_sd, b_m = _fused_run(True, 70, dropout=0.2, graph=True, lr_at=lr_at)
    c_sd, _ = _fused_run(True, 70, dropout=0.2, clock=True)
    assert any(not torch.equal(a_sd[k], c_sd[k]) for k in a_sd)      # the changes took effect
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_graph_recapture_table_move_lr_change_bitwise_equals_eager_clock(monkeypatch):
    """The geometry of round 4's r4i fault (an illegal address in the replay after an lr change
    under graph=True): a capture horizon of 8 steps and a scalar pad of 16
    make the step graph expire, get dropped and re-captured every few steps while the per-step
    scalar table grows (moves) under it, with lr changes before, between and right at those
    points.  Dropping a graph drains the stream first, a growing table drains the device; bit
    for bit the eager clock path taking the same changes."""
    import ncf_amd.deferred as de
    import ncf_amd.trainer as tr
    monkeypatch.setattr(tr, "GRAPH_HORIZON", 8)
    monkeypatch.setattr(de, "SCALAR_PAD", 16)
    lr_at = {5: 5e-4, 11: 2.5e-4, 12: 3e-4, 23: 4e-4, 24: 6e-4, 37: 2e-4}
    seen = {"tables": set(), "captures": 0}
    capture = tr.FusedTrainStep._capture

    def counted(self, *a, **k):
        seen["captures"] += 1
        return capture(self, *a, **k)
    monkeypatch.setattr(tr.FusedTrainStep, "_capture", counted)

    def probe(step, s):
        seen["tables"].add(step.deferred._table.data_ptr())
    a_sd, a_m = _fused_run(True, 48, dropout=0.2, clock=True, lr_at=lr_at)
    b_sd, b_m = _fused_run(True, 48, dropout=0.2, graph=True, lr_at=lr_at, on_step=probe)
    assert len(seen["tables"]) >= 3, seen      # the table moved under the graph path
    assert seen["captures"] >= 3, seen         # ... which re-captured several times
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k


def test_fused_step_matches_dropin_path(f2):
    """FusedTrainStep (fused BCE, deferred Adam) vs the reference call pattern (nn.BCELoss +
    torch.optim.Adam through the hook) on the F2 golden batches."""
    from ncf_amd.trainer import FusedTrainStep
    g = f2
    U, I, D, Tt, H, B, M, steps = [int(x) for x in g["cfg"]]
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, Tt, [256, 128, 64], H, 0.0, M - 1)
    m.load_state_dict(T(sub(g, "init/")), strict=True)
    m = m.to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
    for s in range(steps):
        w = step(torch.from_numpy(g[f"step{s}/user_ids"]).to(DEV),
                 torch.from_numpy(g[f"step{s}/item_ids"]).to(DEV),
                 torch.from_numpy(g[f"step{s}/targets"]).to(DEV))
        assert abs(float(w.loss.item()) - float(g[f"step{s}/loss"])) < 2e-6
    sd = m.state_dict()
    lr, wd = 1e-3, 1e-5
    for k, v in sub(g, f"after{steps - 1}/param/").items():
        assert_params_close(k, sd[k].cpu().numpy(), v, zone_masks(g, k, steps), lr)


# ----------------------------------------------------------------------------- sharded (RCCL)
def _sharded_vs_fused(exchange, ahead, U=2000, I=300, Bg=64, steps=14, check_hot=False):
    """The row-sharded step at world size 1 against FusedTrainStep on the same batches: losses
    every step and every parameter bit for bit at the end."""
    import socket
    import torch.distributed as dist
    from ncf_amd.distributed import make_sharded_step
    from ncf_amd.trainer import FusedTrainStep
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        def factory(ru, ri):
            torch.manual_seed(5)
            return ncf.AdvancedNCF(ru, ri, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, 4).to(DEV).train()
        ms, sharded = make_sharded_step(factory, U, I, lr=1e-3, weight_decay=1e-5,
                                        exchange=exchange)
        assert type(sharded.x).__name__ == ("RcclExchange" if exchange == "rccl" else "ShardExchange")
        sharded.ahead = ahead          # next step's first all-to-all during this step, or not
        mf = factory(U, I)
        fused = FusedTrainStep(mf, lr=1e-3, weight_decay=1e-5)
        g = torch.Generator().manual_seed(6)
        batches = []
        for _ in range(steps):
            u = torch.randint(0, U, (Bg,), generator=g).repeat_interleave(5).to(DEV)
            i = (torch.rand(Bg * 5, generator=g) ** 3 * I).long().to(DEV)
            t = torch.zeros(Bg, 5)
            t[:, 0] = 1
            batches.append((u, i, t.reshape(-1, 1).to(DEV)))
        if check_hot:
            # hot items: segments of many 16-occurrence pieces (the multi-piece fix-up); ids past
            # 2^20 (the two-pass radix sort of the plan's keys)
            counts = torch.bincount(batches[0][1].cpu(), minlength=I)
            assert int(counts.max()) > 16 * 16 and int((counts > 16).sum()) >= 20
            assert int(batches[0][0].max()) >= 1 << 19 and U > 1 << 19
        for s_, (u, i, t) in enumerate(batches):
            # steps 1 .. steps-2 plan their successor ahead (pipelined); the first and the last
            # plan inline
            nxt = batches[s_ + 1][:2] if 1 <= s_ < len(batches) - 1 else None
            l1 = sharded(u, i, t, next=nxt)
            fused(u, i, t)
            assert abs(float(l1.item()) - float(fused.last_loss.item())) < 1e-6
        sharded.ops.check()
        a, b = ms.state_dict(), mf.state_dict()
        for k in a:
            assert torch.equal(a[k], b[k]), k
        if exchange == "rccl" and steps >= 14:
            # the later steps replayed their launch tapes (tapes.SegmentTapes)
            assert sharded.tapes.replays >= 8, sharded.tapes.replays
        if exchange == "rccl":
            sharded.x.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange,ahead", [("rccl", True), ("rccl", False), ("torch", True)])
def test_sharded_step_world1_bitwise_equals_fused(exchange, ahead):
    """The row-sharded DP step (owner bucketing, all-to-alls over RCCL, mini tables, owner-side
    sums, deferred Adam on the shard) at world size 1 reproduces FusedTrainStep bit for bit, with
    the C-ABI collectives (RcclExchange) and with torch.distributed's; the world > 1 protocol
    itself is covered by tests/test_dist_cpu.py (gloo, 2 ranks) and test_gpu_dist.py."""
    _sharded_vs_fused(exchange, ahead)


def test_sharded_step_c3_size_world1_bitwise_equals_fused():
    """C3's per-rank workload (BASELINE configs[2]: 1M users x 100K items, D = 64, 4096 groups of
    5 per rank; VERDICT r5 missing 2): the row-sharded step at world 1 — the plan's two-pass radix
    sort of 1M-row keys, hot items whose segments span many pieces, the received rows read in
    place — bit for bit the fused step over 6 steps (4 of them pipelined)."""
    _sharded_vs_fused("rccl", True, U=1_000_000, I=100_000, Bg=4096, steps=6, check_hot=True)


def test_comm_alltoallv_and_allreduce_single_rank():
    """ncf_comm_alltoallv / ncf_comm_allreduce_sum_f32 on a one-rank communicator: the
    all-to-all is a copy of the first send_rows rows (any row width, empty splits), the sum
    all-reduce is the identity."""
    import ctypes
    from ncf_amd import _lib
    assert _lib.query("ncf_comm_available") == 1
    uid = torch.zeros(128, dtype=torch.uint8)
    _lib.call("ncf_comm_unique_id", uid.data_ptr(), 128)
    comm = ctypes.c_void_p()
    _lib.call("ncf_comm_init", uid.data_ptr(), 128, 1, 0, ctypes.byref(comm))
    try:
        st = torch.cuda.current_stream().cuda_stream
        g = torch.Generator().manual_seed(3)
        for rows, width, dt in [(1000, 128, torch.float32), (37, 1, torch.int32), (0, 16, torch.int64),
                                (5, 3, torch.int64)]:
            src = (torch.randn(rows + 4, width, generator=g) * 100).to(dt).to(DEV)
            dst = torch.full((max(rows, 1), width), -7, dtype=dt, device=DEV)
            n = (ctypes.c_int64 * 1)(rows)
            _lib.call("ncf_comm_alltoallv", comm, src.data_ptr(), n, dst.data_ptr(), n,
                      width * src.element_size(), st)
            torch.cuda.synchronize()
            if rows:
                assert torch.equal(dst[:rows], src[:rows])
        x = torch.randn(4099, generator=g).to(DEV)
        y = x.clone()
        _lib.call("ncf_comm_allreduce_sum_f32", comm, y.data_ptr(), y.numel(), st)
        torch.cuda.synchronize()
        assert torch.equal(x, y)
        with pytest.raises(ValueError):   # negative split
            bad = (ctypes.c_int64 * 1)(-1)
            _lib.call("ncf_comm_alltoallv", comm, x.data_ptr(), bad, y.data_ptr(), bad, 4, st)
    finally:
        _lib.call("ncf_comm_destroy", comm)


@pytest.mark.parametrize("a_t,b_t", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("Mm,Nn,Kk", [(77, 130, 45), (20480, 64, 64), (256, 96, 1000), (1, 5, 3),
                                      (64, 256, 128)])
def test_gemm_direct_and_splitk_rowsum_vs_torch(a_t, b_t, Mm, Nn, Kk):
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(Mm * 7 + Nn + Kk)
    A = torch.randn(Mm, Kk, generator=g)
    Bm = torch.randn(Kk, Nn, generator=g) * torch.linspace(0.5, 2.0, Nn)  # asymmetric
    bias = torch.randn(Nn, generator=g)
    As = (A.t().contiguous() if a_t else A).to(DEV)
    Bs = (Bm.t().contiguous() if b_t else Bm).to(DEV)
    lda, ldb = (Mm if a_t else Kk), (Kk if b_t else Nn)
    C = torch.full((Mm, Nn), 3.0, device=DEV)
    _lib.call("ncf_gemm_direct", Mm, Nn, Kk, As.data_ptr(), lda, a_t, Bs.data_ptr(), ldb, b_t,
              C.data_ptr(), Nn, bias.to(DEV).data_ptr(), 1 | 2, _lib.stream_ptr(DEV))  # relu, accum
    ref = (torch.relu(A.double() @ Bm.double() + bias.double()) + 3.0).float()
    np.testing.assert_allclose(C.cpu().numpy(), ref.numpy(), atol=2e-5 * (Kk ** 0.5), rtol=1e-5)
    for splits in (1, 7):
        ws = torch.empty(_lib.query("ncf_gemm_splitk_workspace", Mm, Nn, splits), device=DEV)
        C2 = torch.empty(Mm, Nn, device=DEV)
        db = torch.empty(Mm, device=DEV)
        _lib.call("ncf_gemm_f32_splitk", Mm, Nn, Kk, As.data_ptr(), lda, a_t, Bs.data_ptr(), ldb,
                  b_t, C2.data_ptr(), Nn, 0, db.data_ptr(), splits, ws.data_ptr(), ws.numel(),
                  None, _lib.stream_ptr(DEV))
        np.testing.assert_allclose(C2.cpu().numpy(), (A.double() @ Bm.double()).float().numpy(),
                                   atol=2e-5 * (Kk ** 0.5), rtol=1e-5)
        np.testing.assert_allclose(db.cpu().numpy(), A.double().sum(1).float().numpy(),
                                   atol=2e-5 * (Kk ** 0.5), rtol=1e-5)

@pytest.fixture(params=["small", "radix"])
def dedup_form(request):
    """The one-launch small-batch dedup (<= 2048 ids per kind) and the multi-launch radix sort."""
    from ncf_amd import _lib
    prev = _lib.query("ncf_dedup_set_small_max", 2048 if request.param == "small" else 0)
    yield request.param
    _lib.query("ncf_dedup_set_small_max", prev)


@pytest.mark.parametrize("n0,n1", [(1, 1), (1023, 1025), (2048, 17), (5000, 3000),
                                   (70000, 20480), (0, 7)])
@pytest.mark.parametrize("rows0,rows1", [(1, 2000), (1 << 20, 100000), (1 << 23, 3)])
def test_dedup_ids_vs_numpy(n0, n1, rows0, rows1, dedup_form):
    """Onesweep radix dedup (1, 2 and 3 passes; ragged tiles; look-back over many tiles; a
    Zipf-hot id) and the one-launch form for batches <= 2048 ids: uniq ids == np.unique, counts,
    slot maps and the inverse map (which reads the sorted pairs and per-tile segment offsets)."""
    from ncf_amd import _lib
    rng = np.random.default_rng(n0 * 31 + n1 + rows0 % 97)
    ids = []
    for n, rows in ((n0, rows0), (n1, rows1)):
        x = (rng.zipf(1.2, n) - 1) % rows if n else np.zeros(0, np.int64)
        if n > 100:
            x[::7] = rows - 1
        ids.append(torch.from_numpy(x.astype(np.int64)))
    n = max(n0, n1)
    D = 64
    ws = torch.empty(_lib.query("ncf_embedding_bwd_workspace", n, D), dtype=torch.uint8, device=DEV)
    uq = [torch.full((max(1, n),), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
    slot = [torch.full((r,), -1, dtype=torch.int32, device=DEV) for r in (rows0, rows1)]
    inv = [torch.full((max(1, n),), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
    nu = torch.full((2,), 99, dtype=torch.int32, device=DEV)
    dv = [t.to(DEV) for t in ids]
    st = _lib.stream_ptr(DEV)
    _lib.call("ncf_dedup_ids2", dv[0].data_ptr(), n0, rows0, dv[1].data_ptr(), n1, rows1, D,
              uq[0].data_ptr(), uq[1].data_ptr(), slot[0].data_ptr(), slot[1].data_ptr(),
              nu.data_ptr(), ws.data_ptr(), ws.numel(), st)
    _lib.call("ncf_dedup_inverse", n0, n1, rows0, rows1, D, inv[0].data_ptr(), inv[1].data_ptr(),
              ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    for k, (x, nk) in enumerate(zip(ids, (n0, n1))):
        u, iv = np.unique(x.numpy(), return_inverse=True)
        assert int(nu[k]) == len(u)
        np.testing.assert_array_equal(uq[k][:len(u)].cpu().numpy(), u)
        np.testing.assert_array_equal(inv[k][:nk].cpu().numpy(), iv)
        s = slot[k].cpu().numpy()
        np.testing.assert_array_equal(s[u], np.arange(len(u)))
        assert (np.delete(s, u) == -1).all()


@pytest.mark.parametrize("n,D", [(1280, 64), (40, 16), (2048, 128), (17, 64)])
def test_dedup_small_form_bitwise_equals_radix(n, D):
    """The one-launch small-batch dedup leaves the segments / pieces the embedding backward reads
    exactly as the multi-launch radix sort does: the compact table gradients, the LayerNorm
    parameter gradients, uniq ids and counts bit for bit (1,280 ids = the reference's default
    batch, 256 groups x 5; hot ids spanning several pieces)."""
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(n + D)
    U, I = 1_000_000, 100_000
    uid = torch.randint(0, U, (n // 5 + 1,), generator=g).repeat_interleave(5)[:n]
    iid = (torch.rand(n, generator=g) ** 3 * I).long()
    tabs = [torch.randn(r, D, generator=g).to(DEV) for r in (U, U, I, I)]
    dys = [torch.randn(n, D, generator=g).to(DEV) for _ in range(4)]
    gm, gl = torch.randn(D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)
    ud, idd = uid.to(DEV), iid.to(DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    st = _lib.stream_ptr(DEV)
    res = []
    for small in (2048, 0):
        prev = _lib.query("ncf_dedup_set_small_max", small)
        try:
            ws = torch.full((_lib.query("ncf_embedding_bwd_workspace", n, D),), 0x5A,
                            dtype=torch.uint8, device=DEV)
            uq = [torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
            nu = torch.zeros(2, dtype=torch.int32, device=DEV)
            G = [torch.zeros(n, D, device=DEV) for _ in range(4)]
            pg = [torch.zeros(D, device=DEV) for _ in range(4)]
            _lib.call("ncf_dedup_ids", P(ud), P(idd), n, D, U, I, P(uq[0]), P(uq[1]), None, None,
                      P(nu), P(ws), ws.numel(), st)
            _lib.call("ncf_embedding_bwd_reduce", n, D, U, I, *[P(x) for x in dys],
                      *[P(x) for x in (tabs[0], tabs[1], tabs[2], tabs[3])], P(gm), P(gl), 1e-5,
                      *[P(x) for x in G], P(uq[0]), P(uq[1]), *[P(x) for x in pg], P(ws),
                      ws.numel(), None, st)
            torch.cuda.synchronize()
        finally:
            _lib.query("ncf_dedup_set_small_max", prev)
        res.append((nu.cpu(), [u.cpu() for u in uq], [x.cpu() for x in G], [x.cpu() for x in pg]))
    (n0, u0, g0, p0), (n1, u1, g1, p1) = res
    assert torch.equal(n0, n1)
    for a, b in zip(u0 + g0 + p0, u1 + g1 + p1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shapes", [
    [(64, 64), (64, 128), (128, 256), (256, 64)],      # C2: attention + MLP tower
    [(16, 16), (64, 16), (32, 64), (1, 32)],           # C1 dims + a 1-row output
])
@pytest.mark.parametrize("n", [20480, 999, 1])
def test_wgrad_grouped_vs_torch(shapes, n):
    """All weight gradients of a step in one grouped launch: dW = dYᵀX (+ bias = column sums of
    dY), strided inputs, accumulate; inline reduce and deferred reduce are bit-identical."""
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(n + len(shapes))
    st = _lib.stream_ptr(DEV)
    descs = (_lib.WgradDesc * len(shapes))()
    keep, refs = [], []
    for k, (mo, ki) in enumerate(shapes):
        dy = torch.randn(n, mo + 3, generator=g).to(DEV)       # ld = mo + 3 (strided)
        x = torch.randn(n, ki + 1, generator=g).to(DEV)
        dw = torch.randn(mo, ki + 2, generator=g).to(DEV)      # ldw = ki + 2
        db = torch.empty(mo, device=DEV)
        acc = k % 2
        ref_w = dy[:, :mo].double().t() @ x[:, :ki].double() + (dw[:, :ki].double() if acc else 0)
        refs.append((ref_w, dy[:, :mo].double().sum(0)))
        d = descs[k]
        d.dy, d.x, d.dw, d.dbias = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr()
        d.ldy, d.ldx, d.ldw = mo + 3, ki + 1, ki + 2
        d.m_out, d.k_in, d.n, d.slabs, d.accumulate = mo, ki, n, max(1, n // 160), acc
        keep.append((dy, x, dw, db, dw.clone()))
    ws = torch.empty(_lib.query("ncf_wgrad_grouped_workspace", ctypes.addressof(descs), len(shapes)),
                     device=DEV)
    _lib.call("ncf_wgrad_grouped", ctypes.addressof(descs), len(shapes), ws.data_ptr(), ws.numel(),
              None, st)
    torch.cuda.synchronize()
    outs = [(t[2].clone(), t[3].clone()) for t in keep]
    for (dw0, db0), (rw, rb), (mo, ki) in zip(outs, refs, shapes):
        tol = 2e-5 * max(1.0, n ** 0.5)
        np.testing.assert_allclose(dw0[:, :ki].cpu().double().numpy(), rw.cpu().numpy(), rtol=1e-5, atol=tol)
        np.testing.assert_allclose(db0.cpu().double().numpy(), rb.cpu().numpy(), rtol=1e-5, atol=tol)
    # deferred: restore the accumulate targets, run again through a reduce list
    for t in keep:
        t[2].copy_(t[4])
    lst = _lib.ReduceList()
    _lib.call("ncf_wgrad_grouped", ctypes.addressof(descs), len(shapes), ws.data_ptr(), ws.numel(),
              lst.address, st)
    scr = torch.empty(max(1, _lib.query("ncf_reduce_batch_scratch", lst.address)), device=DEV)
    _lib.call("ncf_reduce_batch", lst.address, scr.data_ptr(), scr.numel(), st)
    torch.cuda.synchronize()
    for (dw0, db0), t in zip(outs, keep):
        assert torch.equal(dw0, t[2]) and torch.equal(db0, t[3])


def test_f5_score_topk_matches_reference_top10(f5):
    """C5 scorer on the demo checkpoint: the reference's forward_simple + top-10 (golden F5)."""
    from ncf_amd.scoring import score_topk
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    s, it = score_topk(m, torch.arange(nu), k=10)
    got = it.cpu().numpy()
    ref_top = np.take_along_axis(f5["scores"], f5["top_items"], axis=1)
    # same ranking; positions may differ only between reference scores tied within 1e-6
    # (torch.topk's tie order is unspecified, ours is item id ascending)
    np.testing.assert_allclose(np.take_along_axis(f5["scores"], got, axis=1), ref_top, atol=1e-6)
    assert (np.sort(got, 1) == np.sort(f5["top_items"], 1)).mean() > 0.95
    np.testing.assert_allclose(s.cpu().numpy(), ref_top, atol=2e-6)


@pytest.mark.parametrize("k,cap", [(1, 8192), (10, 8192), (100, 8192), (100, 128)])
def test_score_topk_vs_oracle(k, cap):
    """Factorised scorer vs the oracle's score_factorised + a (score desc, id asc) sort: users
    not a multiple of the 256-user tile, items not a multiple of the 32-item tile; cap=128
    forces the overflow re-run path."""
    from oracle import ncf_oracle as O
    from ncf_amd.scoring import score_topk
    torch.manual_seed(3)
    U, I = 300, 20011
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randint(0, U, (37,))
    s, it = score_topk(m, users, k=k, cap=cap)
    p = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}
    ref = O.score_factorised(p, users, torch.arange(I), temporal_dim=32, n_layers=3).double()
    for r in range(len(users)):
        order = sorted(range(I), key=lambda j: (-ref[r, j].item(), j))[:k] if k <= 10 else \
            torch.argsort(-ref[r], stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        # identical ranking except where the oracle's own fp32 scores tie within 1e-6
        mism = [a for a, b in zip(got, order) if a != b]
        if mism:
            gs = ref[r, got].numpy()
            os_ = ref[r, order].numpy()
            np.testing.assert_allclose(gs, os_, atol=1e-6)
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, got].numpy(), atol=1e-6)


@pytest.mark.parametrize("D,H,hidden", [(16, 1, [64, 32]), (32, 2, [256, 128, 64])])
def test_score_topk_narrow_dims_vs_oracle(D, H, hidden):
    """The C5 scorer for a model narrower than 64 (C1: D = 16, one head, MLP [64, 32]; and D =
    32): query and item rows zero-padded to the scan's 64-deep rows (ncf_score_queries,
    ItemIndex), against the oracle's score_factorised: the same top-k (except between oracle
    scores tied within 1e-6) and scores within 1e-6."""
    from oracle import ncf_oracle as O
    from ncf_amd.scoring import score_topk
    torch.manual_seed(31)
    U, I, k = 943, 1682, 10
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, 32, hidden, H, 0.2, 4).to(DEV).eval()
    users = torch.randint(0, U, (61,))
    s, it = score_topk(m, users, k=k)
    p = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}
    ref = O.score_factorised(p, users, torch.arange(I), temporal_dim=32,
                             n_layers=len(hidden)).double()
    for r in range(len(users)):
        order = torch.argsort(-ref[r], stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        if got != order:
            np.testing.assert_allclose(ref[r, got].numpy(), ref[r, order].numpy(), atol=1e-6)
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, got].numpy(), atol=1e-6)


@pytest.mark.parametrize("k,cap", [(10, 8192), (100, 8192), (20, 64)])
def test_score_topk_d128_vs_oracle(k, cap):
    """The C5 scorer for a D = 128 model (the C4 width; VERDICT r5 missing 1): the fp32 threshold
    sample and the fp32 scan's 128-deep form (k_collect<128>), against the oracle's
    score_factorised over the whole catalogue — the same top-k (except between oracle scores tied
    within 1e-6) and scores within 1e-6; 300 users (two 256-user blocks, the second partial),
    20011 items (a partial last tile), cap = 64 at k = 20 forces the overflow re-run; the
    captured GraphedScorer gives the same result."""
    from oracle import ncf_oracle as O
    from ncf_amd.scoring import GraphedScorer, ItemIndex, score_topk
    torch.manual_seed(41)
    U, I = 2000, 20011
    m = ncf.AdvancedNCF(U, I, 5, 24, 128, 128, 32, [256, 128, 64], 4, 0.2, 4).to(DEV).eval()
    users = torch.randperm(U)[:300]
    idx = ItemIndex(m)
    assert idx.p.shape[1] == 128 and idx.p3 is None
    s, it = score_topk(m, users, k=k, index=idx, cap=cap)
    p = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}
    ref = O.score_factorised(p, users, torch.arange(I), temporal_dim=32, n_layers=3).double()
    for r in range(len(users)):
        order = torch.argsort(-ref[r], stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        if got != order:
            np.testing.assert_allclose(ref[r, got].numpy(), ref[r, order].numpy(), atol=1e-6)
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, got].numpy(), atol=1e-6)
    g = GraphedScorer(m, len(users), k, index=idx, cap=cap)
    gs, gi = g(users.to(DEV))
    assert torch.equal(gi.cpu(), it.cpu()) and torch.equal(gs.cpu(), s.cpu())


@pytest.mark.parametrize("k,cap", [(10, 8192), (100, 8192), (50, 256)])
def test_split_bf16_scan_equals_fp32_scan(k, cap):
    """The C5 candidate scan on bf16 matrix cores with 2-term operand splits (the default: margin-
    lowered thresholds, candidates re-scored in fp32) and with 3-term splits (k_collect3) against
    the fp32 MFMA scan (k_collect) on the same index: the same top-k items
    (except between scores equal within fp32 accumulation rounding) and scores within 1e-6.
    700 of 5000 users (three 256-user blocks, the last partial), 100003 items (a partial last
    tile); cap=256 at k=50 takes the overflow re-run through a user list."""
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(11)
    U, I = 5000, 100003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    assert idx.p3 is not None and idx.pmax is not None, "a re-scored split scan is the default"
    s2, i2 = score_topk(m, users, k=k, index=idx, cap=cap)
    idx.pmax = None                    # same index, three-term scan (logits from the scan)
    s3, i3 = score_topk(m, users, k=k, index=idx, cap=cap)
    idx.p3 = None                      # same index, fp32 MFMA scan
    s1, i1 = score_topk(m, users, k=k, index=idx, cap=cap)
    for s_, i_ in ((s3, i3), (s2, i2)):
        torch.testing.assert_close(s_, s1, rtol=0, atol=1e-6)
        diff = i_ != i1
        assert diff.float().mean().item() < 1e-3
        if diff.any():
            assert bool(((s_ - s1).abs()[diff] <= 1e-6).all())


@pytest.mark.parametrize("k,cap", [(10, 8192), (100, 8192), (50, 256)])
def test_one_term_scan_equals_two_term_scan(k, cap):
    """The one-product bf16 scan (thresholds lowered by its 2^-8 error bound, every candidate
    within 2E of the scan's K-th re-scored in fp32) against the default two-term scan on the same
    index: both select on the same fp32 re-scored keys, so the top-k items and scores are
    bit-identical; cap = 256 at k = 50 takes the overflow re-run."""
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(13)
    U, I = 5000, 100003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    assert idx.pmax is not None
    idx.terms = 2
    s2, i2 = score_topk(m, users, k=k, index=idx, cap=cap)
    idx.terms = 1
    s1, i1 = score_topk(m, users, k=k, index=idx, cap=cap)
    assert torch.equal(i1, i2)
    assert torch.equal(s1, s2)


@pytest.mark.parametrize("k,cap", [(10, 8192), (100, 8192), (50, 256)])
def test_fp16_threshold_sample_equals_fp32_sample(k, cap, monkeypatch):
    """The threshold sample on bf16 matrix cores with fp16 logits rounded down
    (ncf_score_sample_split16 + ncf_score_kth16, the k-th lowered by the two-term bound) against
    the fp32 sample GEMM + fp32 k-th: only the thresholds differ (both are valid lower bounds of
    the K-th largest logit), so the top-k items and scores are the same bits; cap = 256 at
    k = 50 takes the overflow re-run."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(17)
    U, I = 5000, 100003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    monkeypatch.setattr(scoring, "SAMPLE16", True)
    s16, i16 = score_topk(m, users, k=k, index=idx, cap=cap)
    monkeypatch.setattr(scoring, "SAMPLE16", False)
    s32, i32 = score_topk(m, users, k=k, index=idx, cap=cap)
    assert torch.equal(i16, i32)
    assert torch.equal(s16, s32)


def test_fp16_sample_with_overflowing_bias_equals_fp32_sample(monkeypatch):
    """item biases far outside the fp16 range.  A third of the items get -1e6 (their
    fp16 sample logits round down to -inf) and a few get +1e5 (they saturate at 65504): the k-th
    select's bin range covers the finite sample values only (k_kth_lds fin_lo / fin_hi), so the
    fp16-sample pipeline still returns the fp32-sample pipeline's top-k bits, and the boosted items
    lead every user's list."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(19)
    U, I = 4000, 60013
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:300]
    idx = ItemIndex(m)
    idx.bias[::3] = -1e6
    boost = torch.tensor([5, 7001, 33333], device=DEV)
    idx.bias[boost] = 1e5
    out = []
    for s16 in (True, False):
        monkeypatch.setattr(scoring, "SAMPLE16", s16)
        out.append(score_topk(m, users, k=10, index=idx))
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][0], out[1][0])
    top3 = out[0][1][:, :3].sort(dim=1).values
    assert torch.equal(top3, boost.sort().values.expand_as(top3))


def test_sample_group_maxima_bitwise_equal_max_of_sample():
    """ncf_score_sample_split16 with group 8 stores, per user, the largest fp16 value of every 8
    consecutive sample items: bit for bit the max over the group of the group-1 sample (ragged
    last group, users not a multiple of the 128-user tile)."""
    from ncf_amd import _lib
    from ncf_amd.scoring import ItemIndex
    torch.manual_seed(29)
    U, I, n, S, stride = 500, 30011, 300, 3003, 7
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    idx = ItemIndex(m)
    assert idx.p3 is not None
    q = torch.randn(n, 64, device=DEV)
    sb = torch.randn(S, device=DEV)
    full = torch.empty(n, S, dtype=torch.int16, device=DEV)
    Sg = -(-S // 8)
    grp = torch.empty(n, Sg, dtype=torch.int16, device=DEV)
    st = _lib.stream_ptr(DEV)
    for g, out in ((1, full), (8, grp)):
        _lib.call("ncf_score_sample_split16", q.data_ptr(), n, idx.p3.data_ptr(), I, 64, stride,
                  sb.data_ptr(), S, g, out.data_ptr(), st)
    torch.cuda.synchronize()
    f = full.view(torch.float16).float().cpu()
    pad = torch.full((n, Sg * 8 - S), float("-inf"))
    want = torch.cat([f, pad], 1).view(n, Sg, 8).amax(2)
    assert torch.equal(grp.view(torch.float16).float().cpu(), want)


@pytest.mark.parametrize("k", [10, 100])
def test_sample_group_maxima_same_topk(k, monkeypatch):
    """The C5 pipeline with the threshold sample's group maxima (SAMPLE_GROUP 8) against every
    sample logit (1): the same top-k items and score bits (only the threshold may differ)."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(31)
    U, I = 5000, 100003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    assert scoring._TopKRun(idx, 700, k, 8192).G == 8
    s8, i8 = score_topk(m, users, k=k, index=idx, cap=8192)
    monkeypatch.setattr(scoring, "SAMPLE_GROUP", 1)
    assert scoring._TopKRun(idx, 700, k, 8192).G == 1
    s1, i1 = score_topk(m, users, k=k, index=idx, cap=8192)
    assert torch.equal(i8, i1)
    assert torch.equal(s8, s1)


@pytest.mark.parametrize("k,cap", [(100, 8192), (40, 8192), (100, 4096)])
def test_rank_j_threshold_equals_kth_threshold(k, cap, monkeypatch):
    """Rank-j thresholds (the sample's 16th largest logit over a sample ~k/16 times smaller,
    the selection verified per user by the re-scoring select's thr_check) against the
    sample's k-th: the same top-k items and score bits.  The sample floor is lowered so the
    rank-j plan applies at 100003 items (it does from ~0.8M items at k = 100 by default)."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(19)
    U, I = 5000, 100003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    monkeypatch.setattr(scoring, "SAMPLE_MIN", 256)
    monkeypatch.setattr(scoring, "RANK_J", 16)
    plan = scoring._TopKRun(idx, 700, k, cap)
    assert plan.s16 and plan.j == 16 and plan.thr_chk is not None, "the rank-j plan applies"
    sj, ij = score_topk(m, users, k=k, index=idx, cap=cap)
    monkeypatch.setattr(scoring, "RANK_J", 0)
    assert scoring._TopKRun(idx, 700, k, cap).j == k
    sk, ik = score_topk(m, users, k=k, index=idx, cap=cap)
    assert torch.equal(ij, ik)
    assert torch.equal(sj, sk)


def test_rank_j_shortfall_reruns_from_kth(monkeypatch):
    """A catalogue where the strided threshold sample holds the best items (their bias raised):
    the sample's 16th logit then has fewer than k items at or above it, every user's check in the
    select fails (flag 2), and the re-run from the sample's k-th gives the exact top k: the same
    bits as the k-th-threshold pipeline on the same index."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(23)
    U, I, k = 2000, 100003, 100
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:300]
    idx = ItemIndex(m)
    monkeypatch.setattr(scoring, "SAMPLE_MIN", 256)
    monkeypatch.setattr(scoring, "RANK_J", 16)
    plan = scoring._TopKRun(idx, 300, k, 8192)
    assert plan.j == 16
    idx.bias[:plan.S * plan.stride:plan.stride] += 5.0
    calls = []
    safe = scoring._TopKRun.safe_thresholds

    def counted(self, redo, st):
        calls.append(int(redo.numel()))
        return safe(self, redo, st)
    monkeypatch.setattr(scoring._TopKRun, "safe_thresholds", counted)
    sj, ij = score_topk(m, users, k=k, index=idx)
    assert calls and calls[0] == 300, f"every user re-run from the k-th ({calls})"
    monkeypatch.setattr(scoring, "RANK_J", 0)
    sk, ik = score_topk(m, users, k=k, index=idx)
    assert torch.equal(ij, ik)
    assert torch.equal(sj, sk)
    # and those are the top k of the modified catalogue: the boosted sample items lead
    assert bool((ik % plan.stride == 0).float().mean() > 0.9)


@pytest.mark.parametrize("k,terms", [(10, 2), (100, 2), (100, 3), (10, 1)])
def test_split_scan_item_split_sizing_is_invisible(k, terms, monkeypatch):
    """The split scan's item split raised from the expected candidates per user (k x I / S, the
    `expected_per_user` argument of ncf_score_collect_split: fewer per-wave LDS slice overflows)
    against the default split (expected 0): the same top-k items and the same score bits."""
    from ncf_amd import scoring
    from ncf_amd.scoring import ItemIndex, score_topk
    torch.manual_seed(12)
    U, I = 5000, 200003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randperm(U)[:700]
    idx = ItemIndex(m)
    if terms == 3:
        idx.pmax = None
    else:
        idx.terms = terms
    s_sized, i_sized = score_topk(m, users, k=k, index=idx)
    seen = []
    collect = scoring._collect

    def unsized(*a, expected=0, **kw):
        seen.append(expected)
        return collect(*a, expected=0, **kw)
    monkeypatch.setattr(scoring, "_collect", unsized)
    s0, i0 = score_topk(m, users, k=k, index=idx)
    assert seen and max(seen) > 0, "the launch passes the expected candidates per user"
    assert torch.equal(i_sized, i0)
    assert torch.equal(s_sized, s0)


@pytest.mark.parametrize("U,I,k,cap", [(40, 1003, 10, 8192), (40, 1003, 1, 8192), (20, 64, 64, 8192),
                                       (33, 4099, 37, 8192), (24, 50000, 100, 256)])
def test_score_topk_small_catalogues(U, I, k, cap):
    """Small and odd catalogues: a threshold sample of S = I (not a multiple of 4: the k-th
    kernel's scalar tail), k = I (every item a candidate: the select's take-all path), k = 1;
    k = 100 with cap = 256 needs a sample of 39168 > the LDS-resident 38912 logits (the streaming
    radix k-th kernel)."""
    from oracle import ncf_oracle as O
    from ncf_amd.scoring import score_topk
    torch.manual_seed(31)
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.arange(U)
    s, it = score_topk(m, users, k=k, cap=cap)
    p = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}
    ref = O.score_factorised(p, users, torch.arange(I), temporal_dim=32, n_layers=3).double()
    for r in range(U):
        order = torch.argsort(-ref[r], stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        assert sorted(got) == sorted(order) or np.allclose(
            np.sort(ref[r, got].numpy()), np.sort(ref[r, order].numpy()), atol=1e-6)
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, got].numpy(), atol=1e-6)
        assert bool((s[r][:-1] >= s[r][1:]).all())


@pytest.mark.parametrize("k,cap,distinct", [(100, 8192, 10), (10, 8192, 10), (5, 4096, 10),
                                            (10, 8192, 0)])
def test_score_topk_exact_ties_by_item_id(k, cap, distinct):
    """Select with a tie group straddling the k-th place: all but the last `distinct` items share
    one item row (identical logits for every user), so the k best are the larger of the distinct
    items and then the tied items in ascending id order — the select's second radix pass over
    ids (distinct = 0: every logit equal, min = max in the threshold and select kernels).  Checked against the oracle's scores sorted by (score desc, id asc).  (A cap below the
    tie group's size overflows for good: score_topk raises, as documented.)"""
    from oracle import ncf_oracle as O
    from ncf_amd.scoring import score_topk
    torch.manual_seed(21)
    U, I = 60, 3000
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    with torch.no_grad():
        for t in m.parameters():
            if t.dim() == 2 and t.shape[0] == I:     # the item tables
                t[:I - distinct] = t[0]
    users = torch.arange(0, U, 3)
    s, it = score_topk(m, users, k=k, cap=cap)
    p = {kk: v.detach().cpu() for kk, v in m.state_dict().items()}
    ref = O.score_factorised(p, users, torch.arange(I), temporal_dim=32, n_layers=3)
    for r in range(len(users)):
        tie = ref[r, 0].item()
        others = [(ref[r, j].item(), j) for j in range(I - distinct, I)]
        assert all(abs(v - tie) > 1e-5 for v, _ in others)   # (no near-tie with the group)
        above = [j for v, j in sorted(others, reverse=True) if v > tie]
        want = (above + list(range(k)))[:k]     # then the tied items, ascending ids
        assert it[r].cpu().tolist() == want
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, want].numpy(), atol=1e-6)


@pytest.mark.parametrize("W,strided", [(3, False), (4, True), (1, False)])
@pytest.mark.parametrize("k", [10, 100])
def test_item_sharded_scoring_equals_single(W, strided, k):
    """SURVEY 8e item-sharded C5 scoring, all W shards emulated in one process: per-shard
    top-k (ItemIndex over the shard's global ids) + ncf_score_merge == the one-GPU top-k."""
    from ncf_amd.scoring import ItemIndex, merge_topk, score_topk, shard_items
    torch.manual_seed(5)
    U, I = 200, 5003
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    users = torch.randint(0, U, (45,))
    ref_s, ref_i = score_topk(m, users, k=k)
    ls, li = [], []
    for r in range(W):
        ids = torch.arange(r, I, W) if strided else shard_items(I, W, r)
        s, i = score_topk(m, users, k=k, index=ItemIndex(m, items=ids))
        assert bool(((i % W == r) if strided else ((i >= ids[0]) & (i <= ids[-1]))).all())
        ls.append(s)
        li.append(i)
    gs, gi = merge_topk(torch.cat(ls, 1), torch.cat(li, 1), k)
    torch.testing.assert_close(gs, ref_s, rtol=0, atol=0)
    # identical ids except between exactly tied probabilities
    diff = gi != ref_i
    if diff.any():
        assert bool((gs[diff] == ref_s[diff]).all())


@pytest.mark.parametrize("k,cap,shard", [(10, 8192, False), (100, 128, False), (10, 8192, True)])
def test_graphed_scorer_equals_eager(k, cap, shard):
    """C5 as a captured hipGraph (GraphedScorer, BASELINE configs[4]) == the eager score_topk
    bit for bit, over several replays with different users; cap=128 takes the eager overflow
    re-run after the replay; an item shard maps to global ids inside the graph; a parameter
    change rebuilds the index and re-captures."""
    from ncf_amd.scoring import GraphedScorer, ItemIndex, score_topk, shard_items
    torch.manual_seed(9)
    U, I = 300, 20011
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    m.eval()
    idx = ItemIndex(m, items=shard_items(I, 3, 1)) if shard else None
    sc = GraphedScorer(m, 37, k=k, index=idx, cap=cap)
    for rep in range(3):
        users = torch.randint(0, U, (37,), device=DEV)
        gs, gi = sc(users)
        es, ei = score_topk(m, users, k=k, index=idx, cap=cap)
        assert torch.equal(gs, es) and torch.equal(gi, ei), rep
    with pytest.raises(ValueError):
        sc(torch.zeros(5, dtype=torch.int64, device=DEV))
    with torch.no_grad():
        m.final[0].bias.add_(0.25)
    users = torch.randint(0, U, (37,), device=DEV)
    gs, gi = sc(users)
    es, ei = score_topk(m, users, k=k, index=None if not shard else
                        ItemIndex(m, items=shard_items(I, 3, 1)), cap=cap)
    assert torch.equal(gs, es) and torch.equal(gi, ei)
    with pytest.raises(IndexError):
        sc(torch.full((37,), U, dtype=torch.int64, device=DEV))


def test_merge_topk_empty_slots_and_ties():
    from ncf_amd.scoring import merge_topk
    s = torch.tensor([[0.5, 0.9, 0.5, 0.0, 0.7], [0.1, 0.0, 0.0, 0.0, 0.0]], device=DEV)
    i = torch.tensor([[7, 3, 2, -1, 11], [4, -1, -1, -1, -1]], device=DEV)
    gs, gi = merge_topk(s, i, 4)
    assert gi.cpu().tolist() == [[3, 11, 2, 7], [4, -1, -1, -1]]
    assert gs.cpu().tolist()[0] == pytest.approx([0.9, 0.7, 0.5, 0.5])
    assert gs.cpu().tolist()[1] == [pytest.approx(0.1), 0.0, 0.0, 0.0]


def test_item_index_tracks_fused_updates():
    """An ItemIndex built before a FusedTrainStep is stale afterwards (the HIP Adam writes the
    tables behind torch's _version); score_topk must rebuild it."""
    from ncf_amd.scoring import ItemIndex, score_topk
    from ncf_amd.trainer import FusedTrainStep
    torch.manual_seed(6)
    U, I, B, Mm = 50, 300, 16, 5
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV)
    idx = ItemIndex(m)
    step = FusedTrainStep(m, lr=5e-2)
    u = torch.randint(0, U, (B,), device=DEV).repeat_interleave(Mm)
    it = torch.randint(0, I, (B * Mm,), device=DEV)
    t = torch.zeros(B, Mm, device=DEV)
    t[:, 0] = 1
    m.train()
    for _ in range(3):
        step(u, it, t.reshape(-1, 1))
    step.sync()
    m.eval()
    assert not idx.valid_for(m)
    users = torch.arange(U)
    s_old, i_old = score_topk(m, users, 10, idx)
    s_new, i_new = score_topk(m, users, 10, ItemIndex(m))
    torch.testing.assert_close(s_old, s_new, rtol=0, atol=0)


def test_f6_forward_simple_hour(f5, f6):
    """forward_simple(hour=h) vs the reference (F6: its per-call projection reproduced by seed),
    and the drop-in call that draws its own projection like the reference does."""
    from ncf_amd.ops import forward_simple_hour
    from oracle import ncf_oracle as O
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    items = torch.arange(366, device=DEV)
    with torch.no_grad():
        for c in range(len(f6["hours"])):
            u = torch.full_like(items, int(f6["user_pos"][c]))
            h = torch.full_like(items, int(f6["hours"][c]))
            s = forward_simple_hour(m, u, items, h, projection=(
                torch.from_numpy(f6["proj_w"][c]), torch.from_numpy(f6["proj_b"][c])))
            np.testing.assert_allclose(s.cpu().numpy(), f6["scores"][c], atol=2e-6)
        # the module call draws nn.Linear(T, D) on the model's device from torch's RNG
        torch.manual_seed(77)
        got = m.forward_simple(torch.zeros_like(items), items, torch.full_like(items, 5))
        torch.manual_seed(77)
        lin = torch.nn.Linear(32, 64, device=DEV)
    p = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.forward_simple_hour(p, torch.zeros(366, dtype=torch.int64), torch.arange(366),
                                torch.full((366,), 5), lin.weight.detach().cpu(),
                                lin.bias.detach().cpu(), num_heads=4, n_layers=3)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=2e-6)


def test_forward_simple_hour_train_mode_vs_oracle(f5):
    """forward_simple(hour=h) in training mode (the reference's dropouts active, architecture.py:
    458-473; the drop-in used to refuse it): under torch.no_grad() against the oracle with the
    kernels' own keep-scales (the attention's single-key weight per (row, head); the tower's per
    element after each LayerNorm), recovered from ncf_dropout_rows on the same dropout stream;
    fresh masks per call; with gradients enabled it refuses (no backward on this path)."""
    from ncf_amd import _lib
    from ncf_amd.ops import forward_simple_hour
    from oracle import ncf_oracle as O
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24, dropout=0.25).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.train()
    n, H, D, hid = 366, 4, 64, [256, 128, 64]
    items = torch.arange(n, device=DEV)
    u, h = torch.full_like(items, 2), torch.full_like(items, 7)
    g = torch.Generator().manual_seed(4)
    pw, pb = torch.randn(D, 32, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    seed = 12345

    def keep(cols, group, sd_):
        s_ = torch.empty(n, cols // group, device=DEV)
        o_ = torch.empty(n, cols, device=DEV)
        x_ = torch.ones(n, cols, device=DEV)
        _lib.call("ncf_dropout_rows", x_.data_ptr(), n, cols, group, 0.25, sd_, o_.data_ptr(),
                  s_.data_ptr(), _lib.stream_ptr(DEV))
        return s_.cpu()
    with torch.no_grad():
        got = forward_simple_hour(m, u, items, h, projection=(pw, pb), seed=seed)
        again = forward_simple_hour(m, u, items, h, projection=(pw, pb), seed=seed)
        other = forward_simple_hour(m, u, items, h, projection=(pw, pb), seed=seed + 1)
        sa = keep(D, D // H, seed).view(n, H, 1, 1)
        ms = [keep(w_, 1, (seed + 0x9E37 * (l + 1)) & (2 ** 63 - 1)) for l, w_ in enumerate(hid)]
        with pytest.raises(NotImplementedError):
            with torch.enable_grad():
                m.forward_simple(u, items, h)
        fresh = m.forward_simple(u, items, h)
    assert torch.equal(got, again) and not torch.equal(got, other) and not torch.equal(got, fresh)
    p = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.forward_simple_hour(p, u.cpu(), items.cpu(), h.cpu(), pw, pb, num_heads=H, n_layers=3,
                                attn_drop=sa, mlp_masks=ms)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=2e-6)
    assert ((sa == 0).float().mean() - 0.25).abs() < 0.06


# ----------------------------------------------------------------------------- 8f: negatives
def _sampler_case():
    """40 products; users with histories of 0..5 items, one with 38 of 40 (the fallback path is
    frequent), one with all 40 (the 'bought everything' branch)."""
    I = 40
    hist = {0: [3], 1: [0, 1, 2, 3, 4], 2: [7, 30], 3: list(range(38)), 4: list(range(40))}
    users, prods = [], []
    for u, h in hist.items():
        for p in h:
            users.append(u)
            prods.append(p)
    users += [5] * 30                 # extra interactions skew popularity
    prods += [9] * 30
    return I, hist, torch.tensor(users), torch.tensor(prods)


def test_negative_sampler_distribution_matches_reference():
    """Per user, the empirical distribution of 200K device negatives vs the exact distribution
    of the reference's _sample_negative (oracle.negative_distribution: inverse-popularity draws
    with rejection of positive + history, 10 attempts, uniform fallback) — 6 sigma."""
    from oracle import ncf_oracle as O
    from ncf_amd.data import DeviceNegativeSampler
    I, hist, users, prods = _sampler_case()
    s = DeviceNegativeSampler(users, prods, 6, I, negative_samples=4, device=DEV)
    w = O.inverse_popularity_weights(prods.tolist(), I)
    np.testing.assert_allclose(s.weights, w, rtol=1e-12)
    for u, h in hist.items():
        pos = h[0]
        idx = [k for k in range(len(users)) if users[k] == u and prods[k] == pos][0]
        reps = 50_000
        kjt, tgt = s.batch(torch.full((reps,), idx), seed=100 + u)
        vals = kjt.values().view(2, reps, 5)
        assert bool((vals[0] == u).all())
        assert bool((vals[1][:, 0] == pos).all())
        neg = vals[1][:, 1:].reshape(-1).cpu().numpy()
        emp = np.bincount(neg, minlength=I) / neg.size
        exp = O.negative_distribution(w, h, pos)
        sig = np.sqrt(np.maximum(exp * (1 - exp), 1e-12) / neg.size)
        assert np.all(np.abs(emp - exp) <= 6 * sig + 1e-9), (u, np.max(np.abs(emp - exp) / (sig + 1e-12)))
        assert tgt.shape == (reps * 5, 1)
        assert bool((tgt.view(reps, 5)[:, 0] == 1).all()) and bool((tgt.view(reps, 5)[:, 1:] == 0).all())


def test_negative_sampler_epoch_layout_and_determinism():
    """epoch(): every interaction exactly once, KJT layout (values [users || items], lengths 1),
    identical batches for the same seed, different negatives for another seed; batches run
    through the model's own forward."""
    from ncf_amd.data import DeviceNegativeSampler
    g = torch.Generator().manual_seed(5)
    U, I, P = 50, 300, 1000
    users = torch.randint(0, U, (P,), generator=g)
    prods = torch.randint(0, I, (P,), generator=g)
    s = DeviceNegativeSampler(users, prods, U, I, negative_samples=4, device=DEV)
    seen, b1 = [], []
    for kjt, t in s.epoch(batch_size=128, seed=7, pad_last=False):
        n = kjt.values().numel() // 2
        assert n % 5 == 0 and t.shape == (n, 1)
        assert bool((kjt.lengths() == 1).all()) and kjt.keys() == ["user_id", "product_id"]
        v = kjt.values().view(2, n // 5, 5)
        seen.append(torch.stack([v[0][:, 0], v[1][:, 0]], 1).cpu())
        b1.append(v.cpu())
        # negatives are never the user's positives (histories here are tiny: no fallback)
        for uu, row in zip(v[0][:, 0].tolist(), v[1][:, 1:].tolist()):
            hist = set(prods[users == uu].tolist())
            assert not (set(row) & hist)
    pairs = torch.cat(seen)
    ref = torch.stack([users, prods], 1)
    assert sorted(map(tuple, pairs.tolist())) == sorted(map(tuple, ref.tolist()))
    b2 = [kjt.values().view(2, -1, 5).cpu() for kjt, _ in s.epoch(batch_size=128, seed=7)]
    # train mode pads the short last batch (1000 = 7 x 128 + 104) with its own first 24 groups
    # (ConsistentBatchSampler, data_prep.py:433-438); the groups before the padding are the same
    assert len(b2) == len(b1) and b2[-1].shape[1] == 128 and b1[-1].shape[1] == 104
    assert all(torch.equal(a, b) for a, b in zip(b1[:-1], b2[:-1]))
    assert torch.equal(b2[-1][:, :104, 0], b1[-1][:, :, 0])
    assert torch.equal(b2[-1][:, 104:, 0], b1[-1][:, :24, 0])
    b3 = [kjt.values().view(2, -1, 5).cpu() for kjt, _ in s.epoch(batch_size=128, seed=8)]
    assert not all(torch.equal(a, b) for a, b in zip(b1, b3))
    m = ncf.AdvancedNCF(U, I, 5, 24).to(DEV).train()
    kjt, t = next(s.epoch(batch_size=64, seed=1))
    out = m(kjt)
    assert out.shape == t.shape
    val = DeviceNegativeSampler(users, prods, U, I, mode="val", device=DEV)
    kjt, t = val.batch(torch.arange(10), seed=0)
    assert kjt.values().numel() == 20 and bool((t == 1).all())


# ----------------------------------------------------------------------------- 8f: ANN export
def test_product_embedding_export_vs_reference(f5):
    """L2-normalised "mlp" product vectors (generate_embeddings.py:206-211) on the demo
    checkpoint: the reference's get_product_embeddings rows (F5) normalised, and the oracle."""
    import io
    import json
    from oracle import ncf_oracle as O
    from ncf_amd.export import export_product_embeddings, product_embeddings
    sd = T(sub(f5, "sd/"))
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    pid = torch.from_numpy(f5["emb_pids"])
    got = product_embeddings(m, pid).cpu().numpy()
    ref = f5["emb_item_mlp"] / np.linalg.norm(f5["emb_item_mlp"], axis=1, keepdims=True)
    np.testing.assert_allclose(got, ref, atol=2e-6)
    p = {k: v.cpu() for k, v in sd.items()}
    ln = O.layer_norm(p[O.K_MLP_I][torch.arange(366)], p["mlp_norm.weight"], p["mlp_norm.bias"])
    ln = ln / ln.norm(dim=1, keepdim=True)
    rows = [{"product_id": f"P{i:X}"} for i in range(400)] + [{"product_id": "P5"}]
    buf = io.StringIO()
    assert export_product_embeddings(m, rows, buf) == 400
    recs = [json.loads(x) for x in buf.getvalue().splitlines()]
    assert [r["id"] for r in recs] == [f"P{i:X}" for i in range(400)]
    emb = np.array([r["embedding"] for r in recs])
    np.testing.assert_allclose(emb, ln.numpy()[np.arange(400) % 366], atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6)


# ----------------------------------------------------------------------------- 8f: checkpoints
def test_checkpoint_resume_is_exact(tmp_path):
    """save_checkpoint mid-run (trainer.py:548-585 format, FusedTrainStep moments in torch Adam
    state_dict form), load_checkpoint into a fresh model + step, continue: identical parameters
    to the uninterrupted run (dropout 0, deferred schedule restarted fully synced)."""
    from ncf_amd.checkpoint import load_checkpoint, save_checkpoint
    from ncf_amd.trainer import FusedTrainStep
    U, I, B = 300, 120, 32
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(8):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(5).to(DEV)
        i = torch.randint(0, I, (B * 5,), generator=g).to(DEV)
        t = torch.zeros(B, 5)
        t[:, 0] = 1
        batches.append((u, i, t.reshape(-1, 1).to(DEV)))

    def fresh():
        torch.manual_seed(9)
        m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, 4).to(DEV)
        return m, FusedTrainStep(m, lr=1e-2, weight_decay=1e-5)
    m1, s1 = fresh()
    for b in batches[:4]:
        s1(*b)
    path = str(tmp_path / "ckpt.pt")
    save_checkpoint(path, m1, s1, epoch=2, metrics={"loss": 0.5}, config={"learning_rate": 1e-2})
    for b in batches[4:]:
        s1(*b)
    ref = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    m2, s2 = fresh()
    assert load_checkpoint(path, m2, s2) == 3
    for b in batches[4:]:
        s2(*b)
    got = m2.state_dict()
    for k in ref:
        assert torch.equal(got[k].cpu(), ref[k]), k
    ck = torch.load(path, weights_only=True, map_location="cpu")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config",
                       "model_config"}
    assert ck["model_config"] == {"num_users": U, "num_products": I, "embedding_dim": 64}


# ----------------------------------------------------------------------------- 8f: metrics
@pytest.mark.parametrize("B,M,ties", [(300, 5, False), (257, 5, True), (40, 12, False)])
def test_calculate_metrics_vs_reference_loops(B, M, ties):
    """ncf_amd.metrics.calculate_metrics vs the oracle restatement of src/utils/metrics.py (the
    reference's per-row loops) and sklearn's roc_auc_score; ties exercise AUC's one-half rule
    (both sides rank ties column-ascending)."""
    from sklearn.metrics import roc_auc_score
    from oracle import ncf_oracle as O
    from ncf_amd.metrics import calculate_metrics
    g = torch.Generator().manual_seed(B + M)
    p = torch.rand(B, M, generator=g)
    if ties:
        p = (p * 10).round() / 10
    t = torch.zeros(B, M)
    t[:, 0] = 1
    t[torch.rand(B, M, generator=g) < 0.1] = 1        # some groups with several positives
    got = calculate_metrics(p.reshape(-1, 1).to(DEV), t.reshape(-1, 1).to(DEV), [1, 5, 10],
                            batch_size=B, negative_samples=M - 1)
    ref = O.ranking_metrics(p.tolist(), t.tolist(), [1, 5, 10])
    assert list(got) == list(ref)
    for k in ref:
        assert abs(got[k] - ref[k]) < 1e-9, (k, got[k], ref[k])
    assert abs(got["auc"] - roc_auc_score(t.reshape(-1).numpy(), p.reshape(-1).numpy())) < 1e-12


def test_calculate_metrics_errors_like_reference():
    from ncf_amd.metrics import calculate_metrics
    p = torch.rand(20, device=DEV)
    t = torch.ones(20, device=DEV)
    with pytest.raises(ValueError, match="batch_size and negative_samples"):
        calculate_metrics(p, t)
    with pytest.raises(ValueError, match="Size mismatch"):
        calculate_metrics(p, t, batch_size=3, negative_samples=4)
    # validate(): M = 1, all positives -> scikit-learn 1.6 (requirements.txt:16) gives nan
    with pytest.warns(RuntimeWarning, match="Only one class"):
        got = calculate_metrics(p, t, batch_size=20, negative_samples=0)
    assert np.isnan(got["auc"]) and got["hit_rate@1"] == 1.0


def test_f7_metrics_match_reference(f7):
    from ncf_amd.metrics import calculate_metrics
    for c in ("a", "b"):
        B, M = f7[f"{c}_shape"].tolist()
        got = calculate_metrics(torch.from_numpy(f7[f"{c}_pred"]).to(DEV),
                                torch.from_numpy(f7[f"{c}_targ"]).to(DEV), [1, 5, 10],
                                batch_size=B, negative_samples=M - 1)
        keys = [str(k) for k in f7[f"{c}_keys"]]
        assert list(got) == keys
        np.testing.assert_allclose([got[k] for k in keys], f7[f"{c}_vals"], atol=1e-6)


def test_f8_device_sampler_matches_reference_draws(f8):
    """Device negatives vs the reference's own _sample_negative draws (F8), per (user, positive):
    same weights; per-item frequencies agree within 6 sigma of a two-sample difference."""
    from ncf_amd.data import DeviceNegativeSampler
    inter = torch.from_numpy(f8["interactions"])
    U, I = int(f8["num_users"]), int(f8["num_products"])
    s = DeviceNegativeSampler(inter[:, 0], inter[:, 1], U, I, negative_samples=4, device=DEV)
    np.testing.assert_allclose(s.weights, f8["product_weights"], rtol=1e-12)
    for (u, pos), cnt in zip(f8["pairs"], f8["counts"]):
        idx = int(((inter[:, 0] == int(u)) & (inter[:, 1] == int(pos))).nonzero()[0])
        kjt, _ = s.batch(torch.full((20_000,), idx), seed=int(u))
        neg = kjt.values().view(2, -1, 5)[1][:, 1:].reshape(-1).cpu().numpy()
        a = np.bincount(neg, minlength=I) / neg.size
        n2 = cnt.sum()
        b = cnt / n2
        pool = (a * neg.size + cnt) / (neg.size + n2)
        sig = np.sqrt(np.maximum(pool * (1 - pool), 1e-12) * (1 / neg.size + 1 / n2))
        assert np.all(np.abs(a - b) <= 6 * sig + 1e-9), (u, np.max(np.abs(a - b) / (sig + 1e-12)))


@pytest.mark.parametrize("W,D,U,I", [(3, 64, 1000, 300), (2, 16, 1000, 300), (8, 32, 1000, 300),
                                     (8, 128, 1000, 300), (8, 128, 50_000_000, 5_000_000)])
def test_shard_exchange_kernels_emulated_ranks(W, D, U, I):
    """The row-sharded step's exchange kernels (exchange.hip) for W ranks emulated on one GPU:
    plan (owner-ordered keys, counts, destination-major send layout, spos, inverse), the
    all-to-all emulated by slicing, owner-side sort-free dedup (unique rows, pos table), owner
    gather, rank-ordered gradient sums (bitwise vs a sequential fp32 sum), rows in/out.
    The last case is C4's 8-GPU split (BASELINE configs[3]: 50M x 5M, D = 128): global ids
    above 2^31 / D, 6.25M-row user shards (3.2 GB per emulated shard table)."""
    from ncf_amd import _lib
    n = 60
    Ru, Ri = -(-U // W), -(-I // W)
    g = torch.Generator().manual_seed(W * 100 + D)
    i64 = dict(dtype=torch.int64, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    err = torch.zeros(1, **i32)
    plans = []
    for r in range(W):
        uid = torch.randint(0, U, (n,), generator=g)
        iid = (torch.rand(n, generator=g) ** 2 * I).long()
        bufs = dict(keys=[torch.empty(n, **i64) for _ in range(2)],
                    uniq=[torch.empty(n, **i64) for _ in range(2)],
                    nu=torch.zeros(2, **i32), inv=[torch.empty(n, **i64) for _ in range(2)],
                    counts=torch.zeros(W, 2, **i64), send=torch.empty(2 * n, **i32),
                    spos=[torch.empty(n, **i32) for _ in range(2)],
                    bounds=torch.empty(3 * (W + 1), **i32),
                    ws=torch.empty(_lib.query("ncf_embedding_bwd_workspace", n, D),
                                   dtype=torch.uint8, device=DEV))
        o = _lib.ShardPlanOut()
        o.keys0, o.keys1 = bufs["keys"][0].data_ptr(), bufs["keys"][1].data_ptr()
        o.uniq0, o.uniq1 = bufs["uniq"][0].data_ptr(), bufs["uniq"][1].data_ptr()
        o.num_unique = bufs["nu"].data_ptr()
        o.inv0, o.inv1 = bufs["inv"][0].data_ptr(), bufs["inv"][1].data_ptr()
        o.counts, o.send = bufs["counts"].data_ptr(), bufs["send"].data_ptr()
        o.spos0, o.spos1 = bufs["spos"][0].data_ptr(), bufs["spos"][1].data_ptr()
        o.bounds = bufs["bounds"].data_ptr()
        ud, idv = uid.to(DEV), iid.to(DEV)      # kept alive until the kernels ran
        _lib.call("ncf_shard_plan", ud.data_ptr(), idv.data_ptr(), n, W, U, I, D,
                  ctypes.addressof(o), bufs["ws"].data_ptr(), bufs["ws"].numel(),
                  err.data_ptr(), None)
        torch.cuda.synchronize()
        # reference plan
        counts = bufs["counts"].cpu()
        send = bufs["send"].cpu()
        layout_off = [0]
        for d in range(W):
            layout_off.append(layout_off[-1] + int(counts[d].sum()))
        for k, (ids, R) in enumerate(((uid, Ru), (iid, Ri))):
            keys = (ids % W) * R + ids // W
            uq, inv = torch.unique(keys, return_inverse=True)
            c = int(bufs["nu"][k])
            assert c == len(uq)
            assert torch.equal(bufs["uniq"][k][:c].cpu(), uq)
            assert torch.equal(bufs["inv"][k].cpu(), inv)
            own = uq // R
            assert counts[:, k].tolist() == torch.bincount(own, minlength=W).tolist()
            sp = bufs["spos"][k][:c].cpu().long()
            assert torch.equal(send[sp], (uq % R).int())
            for d in range(W):                      # destination-major, users before items
                sel = sp[own == d]
                base = layout_off[d] + (0 if k == 0 else int(counts[d][0]))
                assert torch.equal(sel, torch.arange(base, base + len(sel)))
        plans.append(dict(bufs=bufs, counts=counts, send=send, off=layout_off, uid=uid, iid=iid))
    assert int(err) == 0
    # owners: emulated all-to-all + sort-free dedup + gather + gradient sums
    gd = torch.Generator(device=DEV).manual_seed(W * 100 + D + 1)
    tables = [torch.randn(R_, D, generator=gd, device=DEV) for R_ in (Ru, Ru, Ri, Ri)]
    mark = [torch.zeros(Ru, **i32), torch.zeros(Ri, **i32)]
    uidx = [torch.zeros(Ru, **i32), torch.zeros(Ri, **i32)]
    for token, o_ in enumerate(range(W), start=1):
        parts, L = [], _lib.ShardRecv()
        L.world, off = W, 0
        for s in range(W):
            p = plans[s]
            parts.append(p["send"][p["off"][o_]:p["off"][o_ + 1]])
            L.start[s], L.n0[s] = off, int(p["counts"][o_][0])
            off += len(parts[-1])
        L.start[W] = off
        recv = torch.cat(parts).to(DEV)
        tot = off
        uq = [torch.empty(max(tot, 1), **i64) for _ in range(2)]
        pos = [torch.empty(max(tot, 1) * W, **i32) for _ in range(2)]
        cnt = torch.zeros(2, **i32)
        _lib.call("ncf_shard_owner_prepare", recv.data_ptr(), ctypes.addressof(L), token,
                  mark[0].data_ptr(), mark[1].data_ptr(), uidx[0].data_ptr(), uidx[1].data_ptr(),
                  Ru, Ri, uq[0].data_ptr(), uq[1].data_ptr(), cnt.data_ptr(), pos[0].data_ptr(),
                  pos[1].data_ptr(), err.data_ptr(), None)
        rows = torch.empty(max(tot, 1), 2 * D, device=DEV)
        _lib.call("ncf_shard_owner_gather", recv.data_ptr(), ctypes.addressof(L),
                  tables[0].data_ptr(), tables[1].data_ptr(), Ru, tables[2].data_ptr(),
                  tables[3].data_ptr(), Ri, D, rows.data_ptr(), None)
        got = torch.randn(max(tot, 1), 2 * D, generator=g).to(DEV)
        G = [torch.empty(max(tot, 1), D, device=DEV) for _ in range(4)]
        _lib.call("ncf_shard_owner_gradsum", got.data_ptr(), pos[0].data_ptr(), pos[1].data_ptr(),
                  cnt.data_ptr(), tot, W, D, G[0].data_ptr(), G[1].data_ptr(), G[2].data_ptr(),
                  G[3].data_ptr(), None)
        torch.cuda.synchronize()
        rc, gc = recv.cpu().long(), got.cpu()
        kind = torch.zeros(tot, dtype=torch.long)
        src = torch.zeros(tot, dtype=torch.long)
        for s in range(W):
            kind[L.start[s] + L.n0[s]:L.start[s + 1]] = 1
            src[L.start[s]:L.start[s + 1]] = s
        for k in (0, 1):
            sel = (kind == k).nonzero().reshape(-1)
            c = int(cnt[k])
            urows = uq[k][:c].cpu()
            assert sorted(urows.tolist()) == sorted(set(rc[sel].tolist()))
            P = pos[k][:c * W].cpu().view(c, W)
            for u, row in enumerate(urows.tolist()):
                for s in range(W):
                    hit = sel[(rc[sel] == row) & (src[sel] == s)]
                    assert P[u, s] == (int(hit[0]) if len(hit) else -1)
                acc = torch.zeros(2 * D)
                for s in range(W):                   # rank order, sequential fp32
                    if P[u, s] >= 0:
                        acc = acc + gc[int(P[u, s])]
                assert torch.equal(G[2 * k][u].cpu(), acc[:D])
                assert torch.equal(G[2 * k + 1][u].cpu(), acc[D:])
            ix = rc[sel].to(DEV)
            assert torch.equal(rows[sel.to(DEV)], torch.cat([tables[2 * k][ix], tables[2 * k + 1][ix]], 1))
    assert int(err) == 0
    # requester rows in / gradients out
    p = plans[0]
    b = p["bufs"]
    nmax = n
    back = torch.randn(2 * n, 2 * D, generator=g).to(DEV)
    mini = [torch.zeros(n, D, device=DEV) for _ in range(4)]
    _lib.call("ncf_shard_rows", back.data_ptr(), b["spos"][0].data_ptr(), b["spos"][1].data_ptr(),
              b["nu"].data_ptr(), nmax, D, *[m_.data_ptr() for m_ in mini], 0, None)
    out = torch.zeros(2 * n, 2 * D, device=DEV)
    _lib.call("ncf_shard_rows", out.data_ptr(), b["spos"][0].data_ptr(), b["spos"][1].data_ptr(),
              b["nu"].data_ptr(), nmax, D, *[m_.data_ptr() for m_ in mini], 1, None)
    torch.cuda.synchronize()
    for k in (0, 1):
        c = int(b["nu"][k])
        sp = b["spos"][k][:c].long()
        assert torch.equal(mini[2 * k][:c], back[sp, :D])
        assert torch.equal(mini[2 * k + 1][:c], back[sp, D:])
        assert torch.equal(out[sp], back[sp])


def test_adam_flat_clock_close_equals_two_launches():
    """ncf_adam_flat_clock_close (flat Adam + step-clock advance in one launch, the last block
    closing the step) == ncf_adam_flat_clock followed by ncf_step_clock_advance, bit for bit, over
    several steps; the block counter is re-armed (0) after every launch."""
    import numpy as np
    from ncf_amd import _lib
    g = torch.Generator().manual_seed(11)
    n = 300_001                       # > one block, not a multiple of 256
    lr, b1, b2, eps, wd, seed = 1e-3, 0.9, 0.999, 1e-8, 1e-5, 12345
    host = np.zeros(4 * 9, dtype=np.float32)      # step scalars of steps 1..8 at index 4s..4s+3
    _lib.call("ncf_adam_step_scalars", lr, b1, b2, eps, 1, 8, host[4:].ctypes.data)
    table = torch.from_numpy(host).to(DEV)
    ps = [torch.randn(n, generator=g).to(DEV) for _ in range(2)]
    ps[1].copy_(ps[0])
    ms = [torch.zeros(n, device=DEV) for _ in range(2)]
    vs = [torch.zeros(n, device=DEV) for _ in range(2)]
    clocks = [torch.tensor([0, seed], dtype=torch.int64, device=DEV) for _ in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(4):
        grad = torch.randn(n, generator=g).to(DEV)
        _lib.call("ncf_adam_flat_clock", ps[0].data_ptr(), grad.data_ptr(), ms[0].data_ptr(),
                  vs[0].data_ptr(), n, table.data_ptr(), 1, clocks[0].data_ptr(), b1, b2, eps, wd, st)
        _lib.call("ncf_step_clock_advance", clocks[0].data_ptr(), seed, st)
        _lib.call("ncf_adam_flat_clock_close", ps[1].data_ptr(), grad.data_ptr(), ms[1].data_ptr(),
                  vs[1].data_ptr(), n, table.data_ptr(), 1, clocks[1].data_ptr(), b1, b2, eps, wd,
                  seed, st)
    torch.cuda.synchronize()
    for a, b in ((ps[0], ps[1]), (ms[0], ms[1]), (vs[0], vs[1]), (clocks[0], clocks[1])):
        assert torch.equal(a, b)
    assert int(clocks[1][0].item()) == 4          # t = 4, reserved (high word) = 0


def test_side_streams_run_beside_the_step():
    """the deferred schedule's side stream (the overlapped sweep, the next
    batch's sort, the late catch-up) runs beside the step's stream whichever streams the process
    took from torch's pool before the step was built (GPU_MAX_HW_QUEUES = 4: a pool stream can
    share the step's hardware queue; _lib.side_stream probes and skips those), and the probe
    itself tells a shared queue apart (a stream with itself serialises)."""
    from ncf_amd import _lib
    from ncf_amd.trainer import FusedTrainStep
    main = torch.cuda.current_stream(DEV)
    assert not _lib.streams_overlap(main, main)          # one queue: two spans, not one
    for k in range(8):
        held = [torch.cuda.Stream(DEV) for _ in range(k)]
        torch.manual_seed(5)
        m = ncf.AdvancedNCF(300, 200, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
        step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5)
        assert step.deferred is not None and step.deferred.overlap
        assert _lib.streams_overlap(step.deferred._side, main), k
        del step, m, held
