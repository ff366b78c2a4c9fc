"""Pooled bags on a real MI355X (marker ``gpu``): ``ncf_amd.sparse.pool_rows`` (ncf_bag_pool_fwd /
ncf_bag_pool_bwd) and the pooled path of ``EmbeddingBagCollection``.

Reference: the float64 restatement of tests/bag_pool_ref.py (pinned to
``torch.nn.functional.embedding_bag`` by test_bag_pool_cpu.py) over the same fp32 tables, with the
element-wise bounds derived there: forward ``(L_b + 4) 2^-24 scale_b sum|w x|``, table gradient
``(c_r + 4) 2^-24 sum|terms|``, weight gradient ``(dim + 4) 2^-24 sum|g x|``.  The bounds hold for
fp32 summation in any order; they are fixed, not measured.  Bitwise: a bag of one id is
``gather_rows``, runs repeat, bags permute, a second backward doubles."""
import functools

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import bag_pool_ref as R

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import sparse  # noqa: E402
from ncf_amd.sparse import gather_rows, pool_rows  # noqa: E402

DEV = torch.device("cuda:0")
KJT = ncf.KeyedJaggedTensor
HOT = 1500 if sparse.BAG_BWD_CHUNK is None else 2 * sparse.BAG_BWD_CHUNK + 3
MODES = [("sum", False), ("mean", False), ("sum", True)]


@functools.lru_cache(maxsize=None)
def case(dim):
    """The case of this width (numpy, never written) and its device tensors."""
    c = R.make_case(dim, HOT)
    d = {k: torch.from_numpy(c[k]).to(DEV) for k in ("table", "ids", "offsets", "weights", "C")}
    return c, d


def run(dim, mode, weighted):
    """One forward + backward of loss = (out * C).sum(): (out, table.grad, weights.grad)."""
    c, d = case(dim)
    table = d["table"].clone().requires_grad_(True)
    w = d["weights"].clone().requires_grad_(True) if weighted else None
    out = pool_rows(table, d["ids"], d["offsets"], w, mode)
    (out * d["C"]).sum().backward()
    return out.detach(), table, w


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("mode,weighted", MODES)
def test_forward_and_gradients_within_the_bounds(dim, mode, weighted):
    c, d = case(dim)
    out, table, w = run(dim, mode, weighted)
    wn = c["weights"] if weighted else None
    ref, bound = R.forward(c["table"], c["ids"], c["offsets"], wn, mode)
    over, ratio = R.within(out.cpu().numpy(), ref, bound)
    print(f"forward dim={dim} {mode} weighted={weighted}: worst err/bound {ratio:.3f}")
    assert over <= 0
    assert (out[torch.from_numpy(c["lengths"] == 0).to(DEV)] == 0).all()
    gt, gbound, count = R.grad_table(R.ROWS, c["ids"], c["offsets"], c["C"], wn, mode)
    got = table.grad.cpu().numpy()
    over, ratio = R.within(got, gt, gbound)
    print(f"grad_table: worst err/bound {ratio:.3f}")
    assert over <= 0
    assert (got[count == 0] == 0).all()
    if weighted:
        gw, wbound = R.grad_weights(c["table"], c["ids"], c["offsets"], c["C"])
        over, ratio = R.within(w.grad.cpu().numpy(), gw, wbound)
        print(f"grad_weights: worst err/bound {ratio:.3f}")
        assert over <= 0
    # a second backward accumulates: exactly twice the first
    first = table.grad.clone()
    wfirst = w.grad.clone() if weighted else None
    out2 = pool_rows(table, d["ids"], d["offsets"], w, mode)
    (out2 * d["C"]).sum().backward()
    assert torch.equal(table.grad, first * 2)
    if weighted:
        assert torch.equal(w.grad, wfirst * 2)


@pytest.mark.parametrize("dim", R.DIMS)
def test_single_id_bags_are_gather_rows_bitwise(dim):
    c, d = case(dim)
    ids = d["ids"]
    off = torch.arange(ids.numel() + 1, device=DEV)
    want = gather_rows(d["table"], ids)
    for mode in ("sum", "mean"):
        assert torch.equal(pool_rows(d["table"], ids, off, mode=mode), want), mode


@pytest.mark.parametrize("dim", (16, 64, 256))
@pytest.mark.parametrize("mode,weighted", MODES)
def test_runs_repeat_bitwise(dim, mode, weighted):
    a, b = run(dim, mode, weighted), run(dim, mode, weighted)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].grad, b[1].grad)
    if weighted:
        assert torch.equal(a[2].grad, b[2].grad)


def test_multi_launch_sort_gives_the_same_gradient_bits():
    """The case's ids fit the dedup's one-launch sort; the radix sort (larger inputs) leaves the
    same segments, so the gradient is the same bits."""
    from ncf_amd import _lib
    want = run(64, "sum", True)
    prev = _lib.query("ncf_dedup_set_small_max", 0)
    try:
        got = run(64, "sum", True)
    finally:
        _lib.query("ncf_dedup_set_small_max", prev)
    assert torch.equal(got[1].grad, want[1].grad) and torch.equal(got[2].grad, want[2].grad)


@pytest.mark.parametrize("dim", (32, 128))
@pytest.mark.parametrize("mode,weighted", MODES)
def test_permuting_the_bags_permutes_the_rows_bitwise(dim, mode, weighted):
    c, d = case(dim)
    perm = np.random.RandomState(3).permutation(R.BAGS)
    off, ids = c["offsets"], c["ids"]
    pieces = [np.arange(off[b], off[b + 1]) for b in perm]
    take = np.concatenate(pieces).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum(c["lengths"][perm])]).astype(np.int64)
    w = d["weights"] if weighted else None
    base = pool_rows(d["table"], d["ids"], d["offsets"], w, mode)
    take_t = torch.from_numpy(take).to(DEV)
    got = pool_rows(d["table"], d["ids"][take_t], torch.from_numpy(poff).to(DEV),
                    None if w is None else w[take_t], mode)
    assert torch.equal(got, base[torch.from_numpy(perm).to(DEV)])


def test_only_what_needs_a_gradient_is_computed():
    c, d = case(64)
    w = d["weights"].clone().requires_grad_(True)
    out = pool_rows(d["table"], d["ids"], d["offsets"], w, "sum")      # table: no grad
    (out * d["C"]).sum().backward()
    gw, wbound = R.grad_weights(c["table"], c["ids"], c["offsets"], c["C"])
    assert R.within(w.grad.cpu().numpy(), gw, wbound)[0] <= 0
    assert pool_rows(d["table"], d["ids"], d["offsets"]).grad_fn is None
    # a grad_out that is not contiguous
    table = d["table"].clone().requires_grad_(True)
    out = pool_rows(table, d["ids"], d["offsets"])
    out.backward(d["C"].t().contiguous().t())
    gt, gbound, _ = R.grad_table(R.ROWS, c["ids"], c["offsets"], c["C"])
    assert R.within(table.grad.cpu().numpy(), gt, gbound)[0] <= 0


def _cfg(name, rows, dim, feats, pooling=None):
    return ncf.EmbeddingBagConfig(num_embeddings=rows, embedding_dim=dim, name=name,
                                  feature_names=feats,
                                  pooling=pooling or ncf.PoolingType.SUM)


def _pooled(bag, values, lengths, weights=None, mode="sum"):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return R.forward(bag.weight.detach().cpu().numpy(), np.asarray(values, dtype=np.int64), off,
                     weights, mode)


def _close(got, ref_bound):
    return R.within(got.detach().cpu().numpy(), *ref_bound)[0] <= 0


def test_collection_two_keys_two_tables_and_a_shared_table():
    torch.manual_seed(5)
    ebc = ncf.EmbeddingBagCollection([
        _cfg("hist", 50, 32, ["user_hist", "cart"]),                       # two features, one table
        _cfg("tags", 40, 64, ["product_tags"], ncf.PoolingType.MEAN)], device=DEV)
    lengths = [2, 0, 3,   1, 4, 0,   0, 2, 2]
    values = [1, 49, 3, 3, 0,   7, 8, 9, 10, 11,   39, 0, 5, 5]
    k = KJT.from_lengths_sync(keys=["user_hist", "product_tags", "cart"],
                              values=torch.tensor(values), lengths=torch.tensor(lengths),
                              stride=3).to(DEV)
    out = ebc(k)
    assert set(out) == {"user_hist", "product_tags", "cart"}
    hist, tags = ebc.embedding_bags["hist"], ebc.embedding_bags["tags"]
    assert tuple(out["user_hist"].shape) == (3, 32) and tuple(out["product_tags"].shape) == (3, 64)
    assert _close(out["user_hist"], _pooled(hist, values[0:5], lengths[0:3]))
    assert _close(out["product_tags"], _pooled(tags, values[5:10], lengths[3:6], mode="mean"))
    assert _close(out["cart"], _pooled(hist, values[10:14], lengths[6:9]))
    assert (out["user_hist"][1] == 0).all() and (out["cart"][0] == 0).all()
    # free-standing: differentiable, both features' gradients land in the shared table
    (out["user_hist"].sum() + out["cart"].sum()).backward()
    g = hist.raw_weight().grad
    count = np.bincount(values[0:5] + values[10:14], minlength=50)
    assert torch.equal(g[:, 0].cpu(), torch.from_numpy(count).float())
    assert tags.raw_weight().grad is None
    # a KJT built with offsets= gives the same rows
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]))
    k2 = KJT(keys=["user_hist", "product_tags", "cart"], values=torch.tensor(values),
             offsets=off).to(DEV)
    out2 = ebc(k2)
    for f in out:
        assert torch.equal(out[f], out2[f]), f


def test_equal_counts_on_the_device_are_pooled_not_gathered():
    torch.manual_seed(6)
    ebc = ncf.EmbeddingBagCollection([_cfg("u", 10, 16, ["user_id"]),
                                      _cfg("p", 10, 16, ["product_id"])], device=DEV)
    k = KJT.from_lengths_sync(keys=["user_id", "product_id"],
                              values=torch.tensor([1, 2, 3, 4], device=DEV),
                              lengths=torch.tensor([2, 0, 1, 1], device=DEV))
    out = ebc(k)
    assert _close(out["user_id"], _pooled(ebc.embedding_bags["u"], [1, 2], [2, 0]))
    assert _close(out["product_id"], _pooled(ebc.embedding_bags["p"], [3, 4], [1, 1]))
    # the single-id layout is still the plain gather
    one = KJT.from_lengths_sync(keys=["user_id", "product_id"],
                                values=torch.tensor([1, 2, 3, 4], device=DEV),
                                lengths=torch.ones(4, dtype=torch.long, device=DEV))
    got = ebc(one)
    assert torch.equal(got["user_id"], ebc.embedding_bags["u"].weight.detach()[[1, 2]])
    assert got["user_id"].grad_fn is None


def test_weighted_collection_and_unweighted_ignores_weights():
    torch.manual_seed(7)
    cfg = _cfg("hist", 30, 16, ["user_hist"])
    lengths, values = [3, 1, 0, 2], [4, 4, 9, 29, 0, 1]
    wts = np.asarray([0.5, -1.0, 0.0, 2.0, 1.5, -0.25], dtype=np.float32)
    k = KJT.from_lengths_sync(keys=["user_hist"], values=torch.tensor(values),
                              lengths=torch.tensor(lengths), weights=torch.from_numpy(wts)).to(DEV)
    weighted = ncf.EmbeddingBagCollection([cfg], device=DEV, is_weighted=True)
    plain = ncf.EmbeddingBagCollection([cfg], device=DEV)
    bag = weighted.embedding_bags["hist"]
    with torch.no_grad():
        plain.embedding_bags["hist"].raw_weight().copy_(bag.raw_weight())
    assert _close(weighted(k)["user_hist"], _pooled(bag, values, lengths, wts))
    assert _close(plain(k)["user_hist"], _pooled(bag, values, lengths))
    one = KJT.from_lengths_sync(keys=["user_hist"], values=torch.tensor([3, 5]),
                                lengths=torch.tensor([1, 1]),
                                weights=torch.tensor([2.0, -1.0])).to(DEV)
    rows = bag.weight.detach()[[3, 5]]
    assert torch.equal(weighted(one)["user_hist"], rows * torch.tensor([[2.0], [-1.0]], device=DEV))
    assert torch.equal(plain(one)["user_hist"], rows)


def test_zero_bags_and_zero_ids():
    ebc = ncf.EmbeddingBagCollection([_cfg("hist", 30, 16, ["user_hist"])], device=DEV)
    none = KJT.from_lengths_sync(keys=["user_hist"], values=torch.zeros(0, dtype=torch.long),
                                 lengths=torch.zeros(0, dtype=torch.long)).to(DEV)
    assert tuple(ebc(none)["user_hist"].shape) == (0, 16)
    empty = KJT.from_lengths_sync(keys=["user_hist"], values=torch.zeros(0, dtype=torch.long),
                                  lengths=torch.zeros(3, dtype=torch.long)).to(DEV)
    out = ebc(empty)["user_hist"]
    assert tuple(out.shape) == (3, 16) and (out == 0).all()
    out.sum().backward()
    assert (ebc.embedding_bags["hist"].raw_weight().grad == 0).all()


def test_model_owned_collection_pools_current_rows_without_grad_fn():
    """After FusedTrainSteps on the deferred schedule the pooled forward of the model's own
    collection reads the current rows (through ``bag.weight``) and returns no ``grad_fn``."""
    from ncf_amd.trainer import FusedTrainStep
    U, I, B, M = 3000, 500, 64, 5
    torch.manual_seed(23)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, M - 1).to(DEV)
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, deferred=True)
    g = torch.Generator().manual_seed(24)
    seen = []
    for _ in range(3):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M).to(DEV)
        i = torch.randint(0, I, (B * M,), generator=g).to(DEV)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        step(u, i, t.reshape(-1, 1).to(DEV))
        seen.append(i[:40].cpu())
    lengths = [3, 0, 50, 1, 26]
    values = torch.cat(seen)[:sum(lengths)]                 # rows the steps have just written
    k = KJT.from_lengths_sync(keys=["product_id"], values=values,
                              lengths=torch.tensor(lengths)).to(DEV)
    assert m.engine.lagging()                               # rows are held behind the step count
    out = m.mlp_embedding_collection(k)["product_id"]
    assert out.grad_fn is None and not out.requires_grad
    assert not m.engine.lagging()
    bag = m.mlp_embedding_collection.embedding_bags["product_id"]
    assert _close(out, _pooled(bag, values.numpy(), lengths))
    with pytest.raises(NotImplementedError):                # the model's own forward still refuses
        m(k)


def test_bad_ids_and_offsets_raise_and_are_clamped():
    c, d = case(16)
    ids = d["ids"].clone()
    ids[5] = R.ROWS
    ids[9] = -1
    with pytest.raises(IndexError):
        pool_rows(d["table"], ids, d["offsets"])
    out = pool_rows(d["table"], ids, d["offsets"], check=False)      # they contribute nothing
    keep = np.ones(c["ids"].size, dtype=bool)
    keep[[5, 9]] = False
    w = keep.astype(np.float32)
    safe = np.where(keep, c["ids"], 0)
    assert _close(out, R.forward(c["table"], safe, c["offsets"], w))
    off = torch.tensor([0, 4, 2, 6], device=DEV)                      # decreasing
    with pytest.raises(ValueError):
        pool_rows(d["table"], d["ids"][:6], off)
    with pytest.raises(ValueError):                                   # past the end
        pool_rows(d["table"], d["ids"][:6], torch.tensor([0, 3, 9], device=DEV))
    out = pool_rows(d["table"], d["ids"][:6], torch.tensor([0, 3, 9], device=DEV), check=False)
    assert _close(out, R.forward(c["table"], c["ids"][:6], np.asarray([0, 3, 6])))
    torch.cuda.synchronize()
