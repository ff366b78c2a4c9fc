"""CPU-only checks of the nearest-product search's host side (``ncf_amd.neighbors``): the
declared entry point and its argument refusals, the slab / merge plan, the validation before any
launch, the JSONL round trip, and the tests' own float64 restatement against a brute force.  The
kernel is tested in test_gpu_neighbors.py."""
import io
import itertools

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import neighbors_ref as R

ncf = _ncf_pkg.load()
from ncf_amd import _lib, export  # noqa: E402
from ncf_amd.neighbors import ProductSearch, plan  # noqa: E402


def test_entry_point_is_declared():
    assert "ncf_nn_scan" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ncf_nn_scan"][1]) == 15
    assert ncf.ProductSearch is ProductSearch


def test_entry_point_refuses_bad_arguments():
    """NCF_CHECK_ARG runs before any launch, so the refusals need no GPU."""
    ok = dict(queries=16, n=1, norm=1, vectors=16, items=100, dim=64, item_cat=None,
              query_cat=None, skip=None, slab=128, slabs=1, K=10, ps=16, pi=16, st=None)
    for change in (dict(K=0), dict(K=129), dict(dim=48), dict(dim=256), dict(slab=0),
                   dict(query_cat=16), dict(slabs=0), dict(items=2 ** 31), dict(queries=8)):
        with pytest.raises(_lib.NCFArgumentError):
            _lib.call("ncf_nn_scan", *{**ok, **change}.values())


@pytest.mark.parametrize("n_items,k", itertools.product(
    [1, 7, 1023, 1025, 20011, 100000, 10 ** 6, 5 * 10 ** 6], [1, 10, 100, 128]))
def test_plan_invariants(n_items, k):
    for blocks in (1, 8):
        p = plan(n_items, k, query_blocks=blocks)
        assert p.g1 * k <= 8192 and p.g2 * k <= 8192          # every merge level
        assert p.g1 * p.g2 >= p.n_slabs >= 1
        # the slabs cover the catalogue exactly once: contiguous, the last one non-empty
        assert (p.n_slabs - 1) * p.slab_items < n_items <= p.n_slabs * p.slab_items
        assert p.slab_items >= 1024
        if n_items >= 512 * 1024:
            assert p.n_slabs * blocks >= 2 * 256                  # two workgroups per CU
    assert plan(n_items, k).g1 == 1 or plan(n_items, k).n_slabs * k > 8192


def test_plan_forced_slabs():
    p = plan(20011, 100, slab_items=64)
    assert (p.slab_items, p.n_slabs) == (64, 313) and p.g1 > 1       # two levels
    assert p.g1 * 100 <= 8192 and p.g2 * 100 <= 8192 and p.g1 * p.g2 >= 313
    assert plan(20011, 10, slab_items=20011) == (20011, 1, 1, 1)
    assert plan(20011, 128, slab_items=33).n_slabs == 607
    with pytest.raises(ValueError):
        plan(5 * 10 ** 6, 128, slab_items=1)       # more slabs than two levels merge
    with pytest.raises(ValueError):
        plan(100, 10, slab_items=0)
    with pytest.raises(ValueError):
        plan(0, 10)


def _cpu_index(I=50, D=16, categories=None):
    """An index object over CPU rows: enough to reach every check that precedes a launch."""
    idx = ProductSearch.__new__(ProductSearch)
    idx._set(torch.nn.functional.normalize(torch.randn(I, D), dim=1), None, categories)
    return idx


def test_validation_before_any_launch():
    idx = _cpu_index(categories=torch.arange(50) % 3)
    q = torch.randn(4, 16)
    for k in (0, 129, -1):
        with pytest.raises(ValueError):
            idx.find_neighbors(q, k)
    for k in (1.5, True, None):
        with pytest.raises(TypeError):
            idx.find_neighbors(q, k)
    with pytest.raises(ValueError):
        idx.find_neighbors(torch.randn(4, 32), 5)                       # another width
    with pytest.raises(TypeError):
        idx.find_neighbors(q.long(), 5)
    with pytest.raises(ValueError):
        idx.find_neighbors(q, 5, category_filter=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        idx.find_neighbors(q, 5, category_filter=torch.zeros(4))
    with pytest.raises(TypeError):
        idx.find_neighbors(q, 5, category_filter=1.0)
    with pytest.raises(ValueError):
        idx.find_neighbors(q, 5, skip=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(TypeError):
        idx.find_neighbors(q, 5, skip=torch.zeros(4))
    with pytest.raises(TypeError):
        idx.find_neighbors(q, 5, skip=[0, 1, 2, 3])
    with pytest.raises(ValueError):                                     # no categories=
        _cpu_index().find_neighbors(q, 5, category_filter=1)
    with pytest.raises(TypeError):
        idx.similar_products(torch.zeros(2), 5)
    # categories of the wrong length or sign, a width the kernel does not take, non-float rows
    with pytest.raises(ValueError):
        ProductSearch.from_vectors(torch.randn(5, 64), categories=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ProductSearch.from_vectors(torch.randn(5, 64), categories=-torch.ones(5, dtype=torch.int64))
    with pytest.raises(TypeError):
        ProductSearch.from_vectors(torch.randn(5, 64), categories=torch.zeros(5))
    for D in (8, 48, 256):
        with pytest.raises(ValueError):
            ProductSearch.from_vectors(torch.randn(5, D))
    with pytest.raises(ValueError):
        ProductSearch.from_vectors(torch.randn(64))
    with pytest.raises(TypeError):
        ProductSearch.from_vectors(torch.zeros(5, 64, dtype=torch.int64))
    with pytest.raises(ValueError):
        ProductSearch.from_vectors(torch.randn(5, 64), ids=torch.arange(4))


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ProductSearch.from_vectors(torch.randn(5, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cpu_index().find_neighbors(torch.randn(4, 16), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ProductSearch(ncf.AdvancedNCF(10, 20, 5, 24))


def test_embeddings_jsonl_round_trip(tmp_path):
    torch.manual_seed(3)
    emb = torch.nn.functional.normalize(torch.randn(9, 64), dim=1)
    emb[2, 5] = 1e-30
    emb[3, 0] = -0.0
    ids = [f"P{i:04X}" for i in range(9)]
    path = str(tmp_path / "e.jsonl")
    assert export.write_embeddings_jsonl(path, ids, emb) == 9
    ids2, emb2 = export.read_embeddings_jsonl(path)
    assert ids2 == ids and emb2.dtype == torch.float32 and emb2.shape == (9, 64)
    assert torch.equal(emb2.view(torch.int32), emb.view(torch.int32))          # the same bits
    buf = io.StringIO()
    export.write_embeddings_jsonl(buf, ids, emb)
    ids3, emb3 = export.read_embeddings_jsonl(io.StringIO(buf.getvalue() + "\n"))
    assert ids3 == ids and torch.equal(emb3, emb2)
    assert export.read_embeddings_jsonl(io.StringIO(""))[1].shape == (0, 0)
    with pytest.raises(ValueError):
        export.read_embeddings_jsonl(io.StringIO(
            '{"id": "a", "embedding": [1.0, 2.0]}\n{"id": "b", "embedding": [1.0]}\n'))


def test_restatement_against_brute_force():
    """50 x 8 with hand-placed ties: rows 3, 4, 20 and 49 identical and nearest to query 0, rows
    10 and 11 identical; a category filter, a skip and a zero query."""
    rng = np.random.default_rng(0)
    V = rng.standard_normal((50, 8)).astype(np.float32)
    V[[4, 20, 49]] = V[3]
    V[11] = V[10]
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    q = rng.standard_normal((4, 8)).astype(np.float32)
    q[0] = 5 * V[3]
    q[3] = 0
    cat = np.arange(50) % 4
    qcat, skip = np.array([-1, 2, -1, 1]), np.array([4, -1, 10, -1])
    sim, mask, ids = R.restate(V, q, 6, cat, qcat, skip)
    for r in range(4):
        # the brute force: every allowed item, best first, the lower position first among equals
        s = [float(np.dot(V[i].astype(np.float64), q[r].astype(np.float64)) /
                   (np.linalg.norm(q[r].astype(np.float64)) or 1.0)) for i in range(50)]
        ok = [i for i in range(50) if (qcat[r] < 0 or cat[i] == qcat[r]) and i != skip[r]]
        want = sorted(ok, key=lambda i: (-s[i], i))[:6]
        assert ids[r].tolist() == want, r
        assert np.allclose(sim[r], s, rtol=0, atol=1e-15)
    assert ids[0].tolist()[:3] == [3, 20, 49]                   # (4 is skipped)
    assert ids[3].tolist() == [1, 5, 9, 13, 17, 21]             # zero query: first matches
    assert ids[2].tolist().count(10) == 0
    # check() accepts the restatement's own answer and refuses a wrong one
    got_i = np.stack([np.pad(x, (0, 6 - len(x)), constant_values=-1) for x in ids])
    got_s = np.stack([np.pad(sim[r][x], (0, 6 - len(x))) for r, x in enumerate(ids)]).astype(
        np.float32)
    R.check(got_s, got_i, sim, mask, ids, 6, R.atol(8))
    bad = got_i.copy()
    bad[1, 0] = [i for i in range(50) if cat[i] != 2][0]
    with pytest.raises(AssertionError):
        R.check(got_s, bad, sim, mask, ids, 6, R.atol(8))
    bad = got_i.copy()
    bad[2, [0, 5]] = bad[2, [5, 0]]
    with pytest.raises(AssertionError):
        R.check(got_s, bad, sim, mask, ids, 6, R.atol(8))
    assert R.atol(64) == 72 * 2.0 ** -24
