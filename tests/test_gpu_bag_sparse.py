"""Sparse table gradients of the pooled bags and ``ncf_amd.SparseAdam`` on a real MI355X (marker
``gpu``): ``pool_rows(sparse=True)`` (``ncf_bag_pool_bwd`` with ``NCF_BAG_COMPACT``),
``EmbeddingBagCollection(sparse=True)`` and the row-wise step on ``ncf_adam_rows_apply``.

The sparse gradient is held to the dense path bit for bit (``to_dense()`` against ``table.grad``
of the same inputs), and the dense path to tests/bag_pool_ref.py's derived bound, so no tolerance
is introduced for it.  The collection's two-feature sum: one fp32 rounding of the exact sum on each
side, ``|sparse - dense| <= 2^-23 |dense|`` element-wise.  SparseAdam: the float64 restatement of
tests/sparse_adam_ref.py (held to ``torch.optim.SparseAdam`` by tests/test_bag_sparse_cpu.py), with
4 x the float32 restatement's own distance from it as the bound (p absolute, m and v relative),
derived at run time from the case's inputs, never from the kernel's output.  On the MI355X the
kernel used at most 0.34 of it (p 0.25, m 0.25, v 0.34)."""
import copy
import functools

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import bag_pool_ref as R
from tests import sparse_adam_ref as S

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import _lib, sparse  # noqa: E402
from ncf_amd.sparse import pool_rows  # noqa: E402

DEV = torch.device("cuda:0")
KJT = ncf.KeyedJaggedTensor
HOT = 2 * sparse.BAG_BWD_CHUNK + 3      # crosses a piece boundary: reaches the combine kernel
MODES = [("sum", False), ("mean", False), ("sum", True)]


@functools.lru_cache(maxsize=None)
def case(dim):
    c = R.make_case(dim, HOT)
    d = {k: torch.from_numpy(c[k]).to(DEV) for k in ("table", "ids", "offsets", "weights", "C")}
    return c, d


def bits(x):
    return x.contiguous().view(torch.int32)


def backward(table, ids, offsets, C, weights=None, mode="sum", check=True, sparse=False):
    """(table.grad, weights.grad) of loss = (pool_rows(...) * C).sum() on fresh leaves."""
    t = table.clone().requires_grad_(True)
    w = None if weights is None else weights.clone().requires_grad_(True)
    out = pool_rows(t, ids, offsets, w, mode, check=check, sparse=sparse)
    (out * C).sum().backward()
    return t.grad, None if w is None else w.grad


def check_sparse(g, shape):
    """The structure every sparse gradient has; returns (indices [U], values [U, dim])."""
    assert g.is_sparse and g.layout == torch.sparse_coo and g.is_coalesced()
    assert tuple(g.shape) == tuple(shape) and g.dtype == torch.float32
    idx, vals = g._indices(), g._values()
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == 1
    assert tuple(vals.shape) == (idx.shape[1], shape[1])
    i = idx[0]
    if i.numel():
        assert int(i.min()) >= 0 and int(i.max()) < shape[0]
        assert bool((i[1:] > i[:-1]).all()), "indices must ascend strictly"
    # truly coalesced: torch's own coalesce of the same entries changes nothing
    again = torch.sparse_coo_tensor(idx, vals, shape).coalesce()
    assert torch.equal(again._indices(), idx) and torch.equal(bits(again._values()), bits(vals))
    return i, vals


def same_as_dense(table, ids, offsets, C, weights=None, mode="sum", check=True):
    """Runs both paths; the sparse gradient's to_dense() is the dense gradient's bits."""
    gd, wd = backward(table, ids, offsets, C, weights, mode, check, sparse=False)
    gs, wsp = backward(table, ids, offsets, C, weights, mode, check, sparse=True)
    assert not gd.is_sparse
    i, vals = check_sparse(gs, table.shape)
    assert torch.equal(bits(gs.to_dense()), bits(gd))
    assert torch.equal(bits(vals), bits(gd[i]))
    if weights is not None:
        assert torch.equal(bits(wsp), bits(wd))
    return gs, gd


@pytest.mark.parametrize("dim", (16, 64, 256))
@pytest.mark.parametrize("mode,weighted", MODES)
def test_sparse_gradient_is_the_dense_gradient_bitwise(dim, mode, weighted):
    c, d = case(dim)
    w = d["weights"] if weighted else None
    gs, gd = same_as_dense(d["table"], d["ids"], d["offsets"], d["C"], w, mode)
    wn = c["weights"] if weighted else None
    ref, bound, count = R.grad_table(R.ROWS, c["ids"], c["offsets"], c["C"], wn, mode)
    over, ratio = R.within(gd.cpu().numpy(), ref, bound)
    print(f"dense grad_table dim={dim} {mode} weighted={weighted}: worst err/bound {ratio:.3f}")
    assert over <= 0
    assert gs._nnz() == int((count > 0).sum())
    assert np.array_equal(gs._indices()[0].cpu().numpy(), np.nonzero(count > 0)[0])


@pytest.mark.parametrize("dim", (16, 64, 256))
def test_second_backward_accumulates_exactly_twice(dim):
    c, d = case(dim)
    t = d["table"].clone().requires_grad_(True)
    for k in range(2):
        out = pool_rows(t, d["ids"], d["offsets"], d["weights"], "sum", sparse=True)
        (out * d["C"]).sum().backward()
        if k == 0:
            first = t.grad.clone()
    i0, v0 = check_sparse(first, t.shape)
    both = t.grad.coalesce()
    assert torch.equal(both._indices()[0], i0)
    assert torch.equal(bits(both._values()), bits(v0 * 2))


def test_radix_sort_path_gives_the_same_sparse_gradient():
    """The case fits the dedup's one-launch sort; forced onto the radix passes it must list the
    same ids (the count comes from another kernel there) with the same bits."""
    c, d = case(64)
    want, _ = backward(d["table"], d["ids"], d["offsets"], d["C"], d["weights"], sparse=True)
    prev = _lib.query("ncf_dedup_set_small_max", 0)
    try:
        got, _ = same_as_dense(d["table"], d["ids"], d["offsets"], d["C"], d["weights"])
    finally:
        _lib.query("ncf_dedup_set_small_max", prev)
    assert torch.equal(got._indices(), want._indices())
    assert torch.equal(bits(got._values()), bits(want._values()))


def _bags(n, per):
    return torch.arange(0, n + 1, per, device=DEV)


def test_edges_one_id_every_id_distinct_and_a_full_table():
    c, d = case(64)
    table = d["table"]
    g = torch.Generator().manual_seed(11)
    # every id equal: U = 1, 200 positions = 13 pieces
    ids = torch.full((200,), 5, dtype=torch.int64, device=DEV)
    C = torch.randn(20, 64, generator=g).to(DEV)
    gs, _ = same_as_dense(table, ids, _bags(200, 10), C)
    assert gs._indices().tolist() == [[5]]
    # every id distinct: U = n_ids
    ids = torch.randperm(R.ROWS, generator=g)[:300].to(DEV)
    C = torch.randn(30, 64, generator=g).to(DEV)
    gs, _ = same_as_dense(table, ids, _bags(300, 10), C, mode="mean")
    assert gs._nnz() == 300
    # every row of the table once: U = n_ids = rows, the compact buffer exactly full
    ids = torch.randperm(R.ROWS, generator=g).to(DEV)
    C = torch.randn(100, 64, generator=g).to(DEV)
    gs, _ = same_as_dense(table, ids, _bags(R.ROWS, 10), C)
    assert gs._nnz() == R.ROWS
    # more ids than rows: U = rows < n_ids
    ids = torch.cat([ids, ids[:500]])
    C = torch.randn(150, 64, generator=g).to(DEV)
    gs, _ = same_as_dense(table, ids, _bags(1500, 10), C)
    assert gs._nnz() == R.ROWS


def test_edges_no_ids_and_empty_bags():
    c, d = case(16)
    table = d["table"]
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    for offsets, bags in ((torch.zeros(4, dtype=torch.int64, device=DEV), 3),
                          (torch.zeros(1, dtype=torch.int64, device=DEV), 0)):
        C = torch.ones(bags, 16, device=DEV)
        gs, gd = same_as_dense(table, none, offsets, C)
        assert gs._nnz() == 0 and tuple(gs._values().shape) == (0, 16) and not gd.any()
    # ids that no bag holds (every bag empty, and offsets that stop short): listed, rows of +0.0
    ids = torch.tensor([9, 3, 9, 700, 3, 12], device=DEV)
    for offsets in (torch.zeros(4, dtype=torch.int64, device=DEV),
                    torch.tensor([0, 0, 2], device=DEV)):
        C = torch.ones(offsets.numel() - 1, 16, device=DEV)
        gs, gd = same_as_dense(table, ids, offsets, C)
        assert gs._indices()[0].tolist() == [3, 9, 12, 700]
        held = ids[:int(offsets[-1])].tolist()
        for r, row in zip(gs._indices()[0].tolist(), gs._values()):
            assert (row == float(held.count(r))).all(), r
            if r not in held:
                assert torch.equal(bits(row), torch.zeros(16, dtype=torch.int32, device=DEV)), r


def test_edges_out_of_range_ids_are_not_listed():
    c, d = case(16)
    table = d["table"]
    ids = torch.tensor([40, R.ROWS, 41, -1, 40, R.ROWS + 5, 999, 2 ** 40], device=DEV)
    offsets = torch.tensor([0, 3, 8], device=DEV)
    C = torch.ones(2, 16, device=DEV)
    with pytest.raises(IndexError):
        pool_rows(table.clone().requires_grad_(True), ids, offsets, sparse=True)
    gs, gd = same_as_dense(table, ids, offsets, C, check=False)
    # the ids out of range are listed nowhere; their positions fall to row 0 (the sort's clamp),
    # which is listed with an exact zero row because no position names row 0
    assert gs._indices()[0].tolist() == [0, 40, 41, 999]
    assert torch.equal(bits(gs._values()[0]), torch.zeros(16, dtype=torch.int32, device=DEV))
    assert (gs._values()[1] == 2.0).all() and (gs._values()[2:] == 1.0).all()
    # with row 0 named by real positions the row holds exactly their terms
    ids2 = torch.tensor([0, R.ROWS, 0, -7], device=DEV)
    gs, gd = same_as_dense(table, ids2, torch.tensor([0, 2, 4], device=DEV), C, check=False)
    assert gs._indices()[0].tolist() == [0] and (gs._values() == 2.0).all()


def _raw_bwd(mode, n_ids, rows, grad_table, ws, ids=None, offsets=None, bags=0, g=None, dim=16):
    _lib.call("ncf_bag_pool_bwd", _lib.ptr(ids), n_ids, _lib.ptr(offsets), bags, None, None,
              _lib.ptr(g), rows, dim, mode, _lib.ptr(grad_table), None, _lib.ptr(ws),
              0 if ws is None else ws.numel(), _lib.stream_ptr(DEV))


def test_c_level_flag_bits_and_the_output_block():
    ids = torch.tensor([7, 2, 7, 5], device=DEV)
    offsets = torch.tensor([0, 4], device=DEV)
    g = torch.ones(1, 16, device=DEV)
    ws = torch.full((_lib.query("ncf_bag_pool_bwd_workspace", 4, 1, 16),), 0xAB, dtype=torch.uint8,
                    device=DEV)
    gt = torch.full((4, 16), -9.0, device=DEV)
    for bad in (2, 3, 0x200, 0x100 | 2, 0x100 | 0x400, -1):
        with pytest.raises(_lib.NCFArgumentError, match="mode"):
            _raw_bwd(bad, 4, 10, gt, ws, ids, offsets, 1, g)
    out = torch.empty(1, 16, device=DEV)
    for bad in (_lib.BAG_COMPACT, _lib.BAG_COMPACT | 1):
        with pytest.raises(_lib.NCFArgumentError, match="mode"):
            _lib.call("ncf_bag_pool_fwd", _lib.ptr(ids), 4, _lib.ptr(offsets), 1, None,
                      _lib.ptr(torch.zeros(10, 16, device=DEV)), 10, 16, bad, _lib.ptr(out), None,
                      _lib.stream_ptr(DEV))
    with pytest.raises(_lib.NCFArgumentError, match="COMPACT"):      # the flag needs grad_table
        _lib.call("ncf_bag_pool_bwd", _lib.ptr(ids), 4, _lib.ptr(offsets), 1, None,
                  _lib.ptr(torch.zeros(10, 16, device=DEV)), _lib.ptr(g), 10, 16, _lib.BAG_COMPACT,
                  None, _lib.ptr(torch.empty(4, device=DEV)), _lib.ptr(ws), ws.numel(),
                  _lib.stream_ptr(DEV))
    assert (gt == -9.0).all()                            # nothing ran
    # the block: U at byte 0, the ids from byte 256; rows >= U untouched (not zero-filled)
    _raw_bwd(_lib.BAG_COMPACT | 1, 4, 10, gt, ws, ids, offsets, 1, g)
    c0, i0 = _lib.BAG_WS_COUNT_OFFSET, _lib.BAG_WS_IDS_OFFSET
    assert int(ws[c0:c0 + 4].view(torch.int32).item()) == 3
    assert ws[i0:i0 + 24].view(torch.int64).tolist() == [2, 5, 7]
    assert gt[:3, 0].tolist() == [0.25, 0.25, 0.5] and (gt[3] == -9.0).all()
    # n_ids == 0, and rows == 0: count 0, nothing else written
    for n_ids, rows in ((0, 10), (4, 0)):
        ws.fill_(0xAB)
        gt.fill_(-9.0)
        _raw_bwd(_lib.BAG_COMPACT, n_ids, rows, gt, ws, ids, offsets, 1, g)
        assert int(ws[c0:c0 + 4].view(torch.int32).item()) == 0
        assert (ws[8:] == 0xAB).all() and (gt == -9.0).all()
    with pytest.raises(RuntimeError, match="workspace"):
        _raw_bwd(_lib.BAG_COMPACT, 0, 10, gt, ws[:128])
    torch.cuda.synchronize()


def test_backward_memory_is_proportional_to_the_ids_not_the_table():
    rows, dim, n, per = 1 << 22, 16, 4096, 16
    table_bytes = rows * dim * 4
    table = torch.zeros(rows, dim, device=DEV, requires_grad=True)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, rows, (n,), generator=g)
    ids[0], ids[1], ids[2] = rows - 1, 0, rows - 1
    ids = ids.to(DEV)
    offsets = _bags(n, per)

    def peak_of_backward(sparse_flag):
        table.grad = None
        out = pool_rows(table, ids, offsets, sparse=sparse_flag)
        loss = out.sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.memory_allocated(DEV)
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(DEV) - before

    extra = peak_of_backward(True)
    gs = table.grad
    i, vals = check_sparse(gs, table.shape)
    uniq, counts = torch.unique(ids, return_counts=True)
    assert torch.equal(i, uniq) and torch.equal(vals[:, 0], counts.float())
    assert int(i[-1]) == rows - 1 and int(i[0]) == 0
    print(f"sparse backward: {extra / 2 ** 20:.2f} MiB beyond the table's {table_bytes >> 20} MiB")
    assert extra < table_bytes // 64                     # 4 MiB: the workspace and U rows
    del gs, vals, i
    dense = peak_of_backward(False)                      # the yardstick measures what it claims
    assert dense >= table_bytes
    table.grad = None


def _cfg(name, rows, dim, feats, pooling=None):
    return ncf.EmbeddingBagConfig(num_embeddings=rows, embedding_dim=dim, name=name,
                                  feature_names=feats, pooling=pooling or ncf.PoolingType.SUM)


def test_collection_two_features_on_one_table():
    torch.manual_seed(5)
    tables = [_cfg("hist", 50, 32, ["user_hist", "cart"]),
              _cfg("tags", 40, 64, ["product_tags"], ncf.PoolingType.MEAN)]
    dense = ncf.EmbeddingBagCollection(tables, device=DEV)
    sp = ncf.EmbeddingBagCollection(tables, device=DEV, sparse=True)
    sp.load_state_dict(dense.state_dict())
    lengths = [2, 0, 3,   1, 4, 0,   0, 2, 2]
    values = [1, 49, 3, 3, 0,   7, 8, 9, 10, 11,   39, 0, 5, 5]
    k = KJT.from_lengths_sync(keys=["user_hist", "product_tags", "cart"],
                              values=torch.tensor(values), lengths=torch.tensor(lengths),
                              stride=3).to(DEV)
    g = torch.Generator().manual_seed(6)
    Cs = {f: torch.randn(3, dm, generator=g).to(DEV)
          for f, dm in (("user_hist", 32), ("cart", 32), ("product_tags", 64))}
    for ebc in (dense, sp):
        out = ebc(k)
        sum((out[f] * Cs[f]).sum() for f in Cs).backward()
    for name in ("hist", "tags"):
        gd = dense.embedding_bags[name].raw_weight().grad
        gs = sp.embedding_bags[name].raw_weight().grad
        assert gs.is_sparse and not gd.is_sparse and tuple(gs.shape) == tuple(gd.shape)
        got = gs.to_dense()
        # each side rounds the exact sum of the two features' rows once
        assert bool(((got - gd).abs() <= 2.0 ** -23 * gd.abs()).all()), name
        print(f"{name}: bitwise equal to the dense sum: {torch.equal(bits(got), bits(gd))}")
    tags = sp.embedding_bags["tags"].raw_weight().grad        # one feature: coalesced, same bits
    check_sparse(tags, (40, 64))
    assert torch.equal(bits(tags.to_dense()), bits(dense.embedding_bags["tags"].raw_weight().grad))
    rows = sp.embedding_bags["hist"].raw_weight().grad.coalesce()._indices()[0].tolist()
    assert rows == sorted(set(values[0:5] + values[10:14]))
    # the single-id layout is still the plain gather, without grad_fn
    one = KJT.from_lengths_sync(keys=["user_hist"], values=torch.tensor([3, 5]),
                                lengths=torch.tensor([1, 1])).to(DEV)
    assert sp(one)["user_hist"].grad_fn is None


def test_model_owned_collection_ignores_the_flag():
    m = ncf.AdvancedNCF(300, 50, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, 4).to(DEV)
    ebc = m.mlp_embedding_collection
    ebc._sparse = True
    k = KJT.from_lengths_sync(keys=["product_id"], values=torch.tensor([1, 2, 3, 4]),
                              lengths=torch.tensor([3, 0, 1])).to(DEV)
    out = ebc(k)["product_id"]
    assert out.grad_fn is None and not out.requires_grad


# ----------------------------------------------------------------------------- SparseAdam
def _grad(ids, vals, shape, split=False):
    i, v = torch.from_numpy(ids).to(DEV), torch.from_numpy(vals).to(DEV)
    if split:       # the same rows in two halves, not coalesced: v/2 + v/2 == v exactly
        return torch.sparse_coo_tensor(torch.cat([i, i.flip(0)])[None],
                                       torch.cat([v * 0.5, v.flip(0) * 0.5]), shape)
    return torch.sparse_coo_tensor(i[None], v, shape, is_coalesced=True)


def _run_ours(case_, steps, p0=None, state_dict=None, cls=None, check_rows=True):
    """The steps on the kernel path; returns (p, optimizer).  Rows a step does not name keep
    parameter and both moments bitwise (checked after every step)."""
    p = torch.nn.Parameter(torch.from_numpy(case_["p"]).to(DEV) if p0 is None else p0.clone())
    opt = (cls or ncf.SparseAdam)([p], lr=S.LRS[0], betas=S.BETAS, eps=S.EPS)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    for s, (ids, vals, lr) in enumerate(steps):
        opt.param_groups[0]["lr"] = lr
        st = opt.state.get(p, {})
        before = [p.detach().clone()] + [st[k].clone() if k in st else torch.zeros_like(p)
                                         for k in ("exp_avg", "exp_avg_sq")]
        p.grad = _grad(ids, vals, p.shape, split=s == 2)
        opt.step()
        if check_rows:
            keep = torch.ones(p.shape[0], dtype=torch.bool, device=DEV)
            keep[torch.from_numpy(ids).to(DEV)] = False
            st = opt.state[p]
            for a, b in zip(before, (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
                assert torch.equal(bits(a[keep]), bits(b[keep])), "a row without a gradient changed"
                assert not torch.equal(bits(a[~keep]), bits(b[~keep]))
    return p, opt


@pytest.mark.parametrize("dim", (16, 64, 256))
def test_sparse_adam_against_float64(dim):
    c = S.make_case(dim)
    ref = S.run(c, S.F64)
    bound, fp = S.bounds(c, ref)
    p, opt = _run_ours(c, c["steps"])
    st = opt.state[p]
    assert st["step"] == len(c["steps"]) and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    got = [x.detach().cpu().numpy() for x in (p, st["exp_avg"], st["exp_avg_sq"])]
    d = S.distance(got, ref, c["touched"])
    ratio = {q: d[q] / bound[q] for q in "pmv"}
    print(f"SparseAdam dim={dim}: fp32 restatement {fp}; kernel / bound "
          + " ".join(f"{q} {ratio[q]:.3f}" for q in "pmv"))
    assert all(ratio[q] < 1.0 for q in "pmv"), ratio
    never = ~c["touched"]
    assert np.array_equal(got[0][never].view(np.int32), c["p"][never].view(np.int32))
    assert not got[1][never].any() and not got[2][never].any()
    assert len(opt._tables) == len(set(S.LRS))          # lr is read every step: a table per lr


def test_sparse_adam_state_dict_moves_to_torch_and_back():
    c = S.make_case(64)
    whole, opt_w = _run_ours(c, c["steps"], check_rows=False)
    half, opt_h = _run_ours(c, c["steps"][:2], check_rows=False)
    sd = copy.deepcopy(opt_h.state_dict())     # (load_state_dict keeps the tensors it is given)
    # into a stock torch.optim.SparseAdam ...
    q = torch.nn.Parameter(half.detach().clone())
    stock = torch.optim.SparseAdam([q], lr=1.0)
    stock.load_state_dict(sd)
    assert stock.state[q]["step"] == 2 and stock.param_groups[0]["lr"] == S.LRS[1]
    assert torch.equal(bits(stock.state[q]["exp_avg"]), bits(opt_h.state[half]["exp_avg"]))
    # ... and back: the remaining steps end on the uninterrupted run's bits
    r = torch.nn.Parameter(half.detach().clone())
    back = ncf.SparseAdam([r], lr=1.0)
    back.load_state_dict(copy.deepcopy(stock.state_dict()))
    for s, (ids, vals, lr) in enumerate(c["steps"][2:], start=2):
        back.param_groups[0]["lr"] = lr
        r.grad = _grad(ids, vals, r.shape, split=s == 2)
        back.step()
    assert back.state[r]["step"] == 5
    assert torch.equal(bits(r.detach()), bits(whole.detach()))
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(back.state[r][k]), bits(opt_w.state[whole][k]))
    # the stock optimizer takes the loaded state on: one step of its own lands on the same
    # float64 reference as ours within the bound
    ids, vals, lr = c["steps"][2]
    stock.param_groups[0]["lr"] = lr
    q.grad = _grad(ids, vals, q.shape)
    stock.step()
    ref3 = S.run(c, S.F64, steps=c["steps"][:3])
    bound, _ = S.bounds(c)
    rows = np.zeros(S.ROWS, bool)
    rows[ids] = True
    d = S.distance([q.detach().cpu().numpy(), stock.state[q]["exp_avg"].cpu().numpy(),
                    stock.state[q]["exp_avg_sq"].cpu().numpy()], ref3, rows)
    assert all(d[x] < bound[x] for x in "pmv"), d


def test_sparse_adam_trains_pool_rows_end_to_end():
    """pool_rows(sparse=True) -> ncf_amd.SparseAdam, three steps, against the dense path's
    gradients fed to the float64 restatement (the rows the dense gradient leaves at zero but the
    sparse one lists cannot differ: every listed row here has positions in a bag)."""
    c, d = case(64)
    t = torch.nn.Parameter(d["table"].clone())
    opt = ncf.SparseAdam([t], lr=1e-2)
    p, m, v = c["table"].astype(S.F64), np.zeros((R.ROWS, 64)), np.zeros((R.ROWS, 64))
    p32 = [x.astype(S.F32) for x in (p, m, v)]
    ids = np.unique(c["ids"])
    for step in (1, 2, 3):
        opt.zero_grad()
        out = pool_rows(t, d["ids"], d["offsets"], d["weights"], sparse=True)
        (out * d["C"]).sum().backward()
        g = t.grad._values().cpu().numpy()
        assert np.array_equal(t.grad._indices()[0].cpu().numpy(), ids)
        opt.step()
        S.sparse_adam_step(p, m, v, ids, g, 1e-2, step)
        S.sparse_adam_step(*p32, ids, g, 1e-2, step, dtype=S.F32)
    rows = np.zeros(R.ROWS, bool)
    rows[ids] = True
    err = np.abs(t.detach().cpu().numpy().astype(S.F64) - p)[rows].max()
    fp = np.abs(p32[0].astype(S.F64) - p)[rows].max()
    print(f"end to end: |p - float64| {err:.3g}, fp32 restatement {fp:.3g}")
    assert err < S.MARGIN * fp
    assert np.array_equal(t.detach().cpu().numpy()[~rows].view(np.int32),
                          c["table"][~rows].view(np.int32))
