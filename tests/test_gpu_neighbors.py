"""Exact nearest-product search (``ncf_amd.neighbors.ProductSearch``: ncf_nn_scan + the slab
merge) on a real MI355X (marker ``gpu``).

Reference: the float64 restatement of tests/neighbors_ref.py over the index's own fp32 rows read
back from the device (that those rows equal the reference's vectors is pinned by
test_product_embedding_export_vs_reference).  Tolerance ``atol = (D + 8) 2^-24``: ids equal except
where the reference similarities of the differing entries lie within 2 atol of each other,
similarities within atol, filter membership and skip exact."""
import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import neighbors_ref as R

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd.neighbors import ProductSearch, plan  # noqa: E402

DEV = torch.device("cuda:0")
U, I, D = 300, 20011, 64       # a prime catalogue: the last tile and the last slab are ragged
DUP = [5, 6, 40, 10000, 20010]
MAX_ERR = []


def _kjt(users):
    n = users.numel()
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([users, torch.zeros_like(users)]),
        lengths=torch.ones(2 * n, dtype=torch.long)).to(DEV)


class _Ctx:
    def __init__(self):
        torch.manual_seed(11)
        self.model = ncf.AdvancedNCF(U, I, 5, 24).to(DEV).eval()
        self.index = ProductSearch(self.model)
        self.V = self.index.vectors.cpu().numpy()          # the index's own rows (never written)
        g = torch.Generator().manual_seed(12)
        self.q = (torch.randn(37, D, generator=g) * 3.0).to(DEV)
        self.cat = torch.randint(0, 24, (I,), generator=g)
        self.cat[[7, 9000, 20010]] = 24                     # a category of exactly 3 items
        self.cat_index = ProductSearch(self.model, categories=self.cat)
        v = torch.randn(I, D, generator=g)
        v[DUP] = v[DUP[0]].clone()
        self.dup_rows = v
        self.dup = ProductSearch.from_vectors(v.to(DEV))


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


def _check(index, V, q, k, out, cat=None, qcat=None, skip=None):
    sim, mask, ids = R.restate(V, q.cpu().numpy(), k, cat, qcat, skip)
    R.check(out[0].cpu().numpy(), out[1].cpu().numpy(), sim, mask, ids, k, R.atol(V.shape[1]),
            MAX_ERR)


def _same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


@pytest.mark.parametrize("k", [1, 10, 100, 128])
@pytest.mark.parametrize("n", [1, 33, 37])
def test_against_float64(ctx, n, k):
    out = ctx.index.find_neighbors(ctx.q[:n], k)
    assert out[0].shape == out[1].shape == (n, k)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int64
    _check(ctx.index, ctx.V, ctx.q[:n], k, out)
    if n == 1:     # a [D] query is a batch of one
        assert _same(ctx.index.find_neighbors(ctx.q[0], k), out)


@pytest.mark.parametrize("k", [10, 100, 128])
def test_slab_plans_agree_bitwise(ctx, k):
    """One slab, the default plan, 313 slabs (two merge levels at k = 100, slabs smaller than k)
    and 607 slabs of 33: the same ids and the same similarity bits."""
    assert plan(I, 100, 64).g1 > 1 and plan(I, k).n_slabs > 1
    outs = [ctx.index.find_neighbors(ctx.q, k, slab_items=s) for s in (I, None, 64, 33)]
    _check(ctx.index, ctx.V, ctx.q, k, outs[0])
    for o in outs[1:]:
        assert _same(o, outs[0])


def test_run_twice_bitwise(ctx):
    a = ctx.cat_index.find_neighbors(ctx.q, 100, category_filter=3)
    b = ctx.cat_index.find_neighbors(ctx.q, 100, category_filter=3)
    assert _same(a, b)


@pytest.mark.parametrize("slab", [None, 64, I])
def test_ties_lowest_id_first(ctx, slab):
    """Five identical rows across a tile and a slab boundary, the query equal to them."""
    q = ctx.dup_rows[DUP[0]].to(DEV)
    sim, ids = ctx.dup.find_neighbors(q, 5, slab_items=slab)
    assert ids[0].tolist() == DUP
    assert len(set(sim[0].view(torch.int32).tolist())) == 1 and abs(float(sim[0, 0]) - 1) < 1e-5
    sim, ids = ctx.dup.find_neighbors(q, 3, slab_items=slab)
    assert ids[0].tolist() == DUP[:3]


@pytest.mark.parametrize("rising", [True, False])
def test_compaction_stress(rising):
    """Similarity to query 0 rising with the position: every item beats the running K-th key, so
    every step appends a full tile per wave and compacts (and falling: none after the first K)."""
    s = torch.linspace(-0.9, 0.9, I, dtype=torch.float64)
    if not rising:
        s = s.flip(0)
    v = torch.zeros(I, D, dtype=torch.float64)
    v[:, 0], v[:, 1] = s, (1 - s * s).sqrt()
    index = ProductSearch.from_vectors(v.float().to(DEV))
    V = index.vectors.cpu().numpy()
    q = torch.zeros(3, D)
    q[0, 0], q[1, 1] = 2.0, 1.0
    q[2] = torch.randn(D, generator=torch.Generator().manual_seed(5))
    q = q.to(DEV)
    outs = [index.find_neighbors(q, 128, slab_items=sl) for sl in (I, None)]
    _check(index, V, q, 128, outs[0])
    assert _same(outs[0], outs[1])
    want = torch.arange(I - 1, I - 129, -1) if rising else torch.arange(128)
    assert outs[0][1][0].cpu().tolist() == want.tolist()


def test_category_filter(ctx):
    g = torch.Generator().manual_seed(13)
    qcat = torch.randint(0, 24, (37,), generator=g)
    qcat[[0, 5, 33]] = -1          # no filter
    qcat[[1, 34]] = 24             # the category of 3 items
    qcat[[2, 36]] = 99             # a category no item has
    sim, ids = out = ctx.cat_index.find_neighbors(ctx.q, 10, category_filter=qcat.to(DEV))
    _check(ctx.cat_index, ctx.V, ctx.q, 10, out, ctx.cat.numpy(), qcat.numpy())
    for r in (1, 34):
        assert sorted(ids[r, :3].tolist()) == [7, 9000, 20010]
        assert ids[r, 3:].tolist() == [-1] * 7 and sim[r, 3:].tolist() == [0.0] * 7
    for r in (2, 36):
        assert ids[r].tolist() == [-1] * 10 and sim[r].tolist() == [0.0] * 10
    got = ids.cpu()
    inside = (got < 0) | (qcat[:, None] < 0) | (ctx.cat[got.clamp_min(0)] == qcat[:, None])
    assert bool(inside.all())
    # one int for every query; a negative int is no filter
    out = ctx.cat_index.find_neighbors(ctx.q[:5], 10, category_filter=24)
    _check(ctx.cat_index, ctx.V, ctx.q[:5], 10, out, ctx.cat.numpy(), np.full(5, 24))
    assert _same(ctx.cat_index.find_neighbors(ctx.q[:5], 10, category_filter=-1),
                 ctx.index.find_neighbors(ctx.q[:5], 10))


def test_similar_products(ctx):
    pid = torch.tensor([0, 17, 9000, 20010])
    out = ctx.index.similar_products(pid.to(DEV), 10)
    assert not bool((out[1].cpu() == pid[:, None]).any())
    _check(ctx.index, ctx.V, ctx.index.vectors[pid.to(DEV)], 10, out, skip=pid.numpy())
    # the duplicated rows: the nearest product of one is another (the lowest id of them)
    sim, ids = ctx.dup.similar_products(torch.tensor([5, 6, 20010], device=DEV), 1)
    assert ids[:, 0].tolist() == [6, 5, 5]
    with pytest.raises(IndexError):
        ctx.index.similar_products(torch.tensor([I], device=DEV), 3)


def test_find_neighbors_of_users(ctx):
    users = torch.randint(0, U, (33,), generator=torch.Generator().manual_seed(14))
    with torch.no_grad():
        ue = ctx.model.get_user_embeddings({"user_features": _kjt(users)})["mlp"]
    a = ctx.index.find_neighbors_of_users(users.to(DEV), 10)
    assert _same(a, ctx.index.find_neighbors(ue, 10))
    _check(ctx.index, ctx.V, ue, 10, a)
    with pytest.raises(IndexError):
        ctx.index.find_neighbors_of_users(torch.tensor([0, U], device=DEV), 10)


def test_small_catalogues():
    g = torch.Generator().manual_seed(15)
    q = torch.randn(3, D, generator=g).to(DEV)
    for n_items in (7, 1):
        index = ProductSearch.from_vectors(torch.randn(n_items, D, generator=g).to(DEV))
        out = index.find_neighbors(q, 10)
        _check(index, index.vectors.cpu().numpy(), q, 10, out)
        assert out[1][:, n_items:].eq(-1).all() and out[1][:, :n_items].ge(0).all()


def test_zero_and_nan_queries(ctx):
    q = ctx.q[:33].clone()
    q[4] = 0
    clean = ctx.index.find_neighbors(q, 10)
    assert clean[1][4].tolist() == list(range(10)) and clean[0][4].tolist() == [0.0] * 10
    q[3, 17] = float("nan")
    sim, ids = ctx.index.find_neighbors(q, 10)
    assert ids[3].tolist() == [-1] * 10 and sim[3].tolist() == [0.0] * 10
    keep = [r for r in range(33) if r != 3]      # its neighbours in the block are unaffected
    assert _same((sim[keep], ids[keep]), (clean[0][keep], clean[1][keep]))


@pytest.mark.parametrize("dim", [16, 32, 128])
def test_other_widths(dim):
    g = torch.Generator().manual_seed(16 + dim)
    index = ProductSearch.from_vectors(torch.randn(3001, dim, generator=g).to(DEV))
    q = torch.randn(5, dim, generator=g).to(DEV)
    out = index.find_neighbors(q, 10)
    _check(index, index.vectors.cpu().numpy(), q, 10, out)
    assert _same(out, index.find_neighbors(q, 10, slab_items=100))


def test_from_vectors_normalises_and_refuses_non_finite():
    g = torch.Generator().manual_seed(17)
    v = torch.randn(40, D, generator=g) * 7
    v[9] = 0
    index = ProductSearch.from_vectors(v.to(DEV), ids=torch.arange(40) * 2 + 1)
    nrm = index.vectors.double().norm(dim=1).cpu()
    assert bool((nrm[torch.arange(40) != 9] - 1).abs().max() < 1e-6) and float(nrm[9]) == 0.0
    sim, ids = index.find_neighbors(v[3].to(DEV), 2)
    assert ids[0, 0].item() == 7 and bool((ids % 2 == 1).all())          # global ids come back
    assert index.similar_products(torch.tensor([7], device=DEV), 1)[1].item() != 7
    v[2, 2] = float("inf")
    with pytest.raises(ValueError):
        ProductSearch.from_vectors(v.to(DEV))


def test_items_subset_and_validity():
    torch.manual_seed(18)
    model = ncf.AdvancedNCF(20, 3001, 5, 24).to(DEV).eval()
    items = torch.arange(0, 3001, 3)
    index = ProductSearch(model, items=items)
    full = ProductSearch(model)
    assert torch.equal(index.vectors, full.vectors[items.to(DEV)])
    q = torch.randn(5, D, generator=torch.Generator().manual_seed(19)).to(DEV)
    sim, ids = index.find_neighbors(q, 10)
    assert bool((ids % 3 == 0).all())
    _check(index, index.vectors.cpu().numpy(), q, 10, (sim, ids // 3))
    out = index.similar_products(torch.tensor([3, 2997], device=DEV), 4)
    assert bool((out[1] % 3 == 0).all()) and 3 not in out[1][0].tolist()
    with pytest.raises(IndexError):
        index.similar_products(torch.tensor([4], device=DEV), 4)        # outside the subset
    with pytest.raises(IndexError):
        ProductSearch(model, items=torch.tensor([3001]))
    assert index.valid_for(model) and not index.valid_for(ncf.AdvancedNCF(20, 3001, 5, 24))
    with torch.no_grad():
        model.mlp_norm.weight.mul_(1.5)
    assert not index.valid_for(model)


def test_reported_errors():
    """The largest |similarity - float64| of the module's comparisons (bound: atol(128))."""
    worst = max(MAX_ERR, default=0.0)
    print("max |sim - ref|:", worst, "atol(64) =", R.atol(64))
    assert worst <= R.atol(128)
