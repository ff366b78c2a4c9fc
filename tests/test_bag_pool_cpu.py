"""Pooled bags, the part that needs no GPU: the float64 restatement (tests/bag_pool_ref.py) is
``torch.nn.functional.embedding_bag`` (the semantic the reference's torchrec EBC maps to:
src/model/architecture.py:153-190, PoolingType.SUM; torchrec pools any bag length), the
KeyedJaggedTensor surface for jagged features, the C-ABI table, and the errors raised before any
device work."""
import os
import re

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import bag_pool_ref as R
from tests.conftest import ROOT

ncf = _ncf_pkg.load()
from ncf_amd import _lib, sparse  # noqa: E402

KJT = ncf.KeyedJaggedTensor


def _hot():
    return 1500 if sparse.BAG_BWD_CHUNK is None else 2 * sparse.BAG_BWD_CHUNK + 3


@pytest.mark.parametrize("dim", R.DIMS)
@pytest.mark.parametrize("mode,weighted", [("sum", False), ("mean", False), ("sum", True)])
def test_restatement_is_embedding_bag_float64(dim, mode, weighted):
    c = R.make_case(dim, _hot())
    table = torch.tensor(c["table"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(c["weights"], dtype=torch.float64, requires_grad=True) if weighted else None
    out = torch.nn.functional.embedding_bag(
        torch.tensor(c["ids"]), table, torch.tensor(c["offsets"]), mode=mode,
        per_sample_weights=w, include_last_offset=True)
    (out * torch.tensor(c["C"], dtype=torch.float64)).sum().backward()
    wn = c["weights"] if weighted else None
    ref, _ = R.forward(c["table"], c["ids"], c["offsets"], wn, mode)
    assert np.abs(out.detach().numpy() - ref).max() <= 1e-12
    assert (ref[c["lengths"] == 0] == 0).all()
    gt, _, count = R.grad_table(R.ROWS, c["ids"], c["offsets"], c["C"], wn, mode)
    assert np.abs(table.grad.numpy() - gt).max() <= 1e-12
    assert (gt[count == 0] == 0).all()
    if weighted:
        gw, _ = R.grad_weights(c["table"], c["ids"], c["offsets"], c["C"])
        assert np.abs(w.grad.numpy() - gw).max() <= 1e-12


def test_case_list_covers_the_edges():
    c = R.make_case(64, _hot())
    L = c["lengths"].tolist()
    assert L[0] == 0 and L[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(L, L[1:]))
    assert {1, 2, 3, 4, 5, 63, 64, 65, 200} <= set(L) and len(L) == 67
    ids = c["ids"]
    assert ids.min() == 0 and ids.max() == R.ROWS - 1 and ids.size < 8192
    assert int((ids == c["hot"]).sum()) == _hot()
    b5 = ids[c["offsets"][5]:c["offsets"][6]]
    assert len(b5) == 5 and len(set(b5.tolist())) < 5
    assert (c["weights"] == 0).sum() >= 3 and (c["weights"] < 0).any()


def _jagged():
    #            user_hist: [1, 2] [] [3]   product_tags: [4] [5, 6, 7] []
    return KJT.from_lengths_sync(keys=["user_hist", "product_tags"],
                                 values=torch.tensor([1, 2, 3, 4, 5, 6, 7]),
                                 lengths=torch.tensor([2, 0, 1, 1, 3, 0]),
                                 weights=torch.arange(7, dtype=torch.float32))


def test_kjt_jagged_surface():
    k = _jagged()
    assert k.stride() == 3
    assert k.length_per_key() == [3, 4] and k.offset_per_key() == [0, 3, 7]
    assert k.length_per_key() is k.length_per_key()          # computed once
    td = k.to_dict()
    assert td["user_hist"].values().tolist() == [1, 2, 3]
    assert td["user_hist"].lengths().tolist() == [2, 0, 1]
    assert td["product_tags"].values().tolist() == [4, 5, 6, 7]
    assert td["product_tags"].offsets().tolist() == [0, 1, 4, 4]
    with pytest.raises(NotImplementedError):
        k.single_id_split()
    assert k.weights().tolist() == list(range(7))
    moved = k.to("cpu")
    assert moved.weights_or_none() is not None and moved.weights().tolist() == list(range(7))
    assert moved.length_per_key() == [3, 4]
    plain = KJT.from_lengths_sync(keys=["a"], values=torch.tensor([1]), lengths=torch.tensor([1]))
    assert plain.weights_or_none() is None and plain.to("cpu").weights_or_none() is None
    with pytest.raises(Exception):
        plain.weights()
    # the equal-count trap: 4 values, 4 lengths, not single-id
    trap = KJT.from_lengths_sync(keys=["user_id", "product_id"], values=torch.tensor([1, 2, 3, 4]),
                                 lengths=torch.tensor([2, 0, 1, 1]))
    assert trap.length_per_key() == [2, 2] and trap.offset_per_key() == [0, 2, 4]
    empty = KJT.from_lengths_sync(keys=["a", "b"], values=torch.zeros(0, dtype=torch.long),
                                  lengths=torch.zeros(0, dtype=torch.long))
    assert empty.length_per_key() == [0, 0] and empty.offset_per_key() == [0, 0, 0]


def test_new_entry_points_are_in_the_table_with_the_header_counts():
    for name, count in (("ncf_bag_pool_fwd", 12), ("ncf_bag_pool_bwd_workspace", 3),
                        ("ncf_bag_pool_bwd", 15)):
        assert len(_lib.SIGNATURES[name][1]) == count, name
    assert _lib.query("ncf_bag_pool_bwd_workspace", 8000, 67, 64) > 0
    assert _lib.query("ncf_bag_pool_bwd_workspace", 0, 0, 64) > 0


def test_chunk_length_is_the_dedup_piece():
    """BAG_BWD_CHUNK is the piece length the backward's partial sums are cut at."""
    seg = open(os.path.join(ROOT, "neural-collaborative-filtering-demo_amd", "csrc",
                            "segments.h")).read()
    assert int(re.search(r"#define NCF_PIECE (\d+)", seg).group(1)) == sparse.BAG_BWD_CHUNK


def test_errors_come_before_any_device_work():
    table = torch.zeros(10, 16)
    ids, off = torch.tensor([1, 2, 3]), torch.tensor([0, 2, 3])
    with pytest.raises(ValueError, match="SUM pooling only"):
        sparse.pool_rows(table, ids, off, weights=torch.ones(3), mode="mean")
    with pytest.raises(ValueError, match="mode"):
        sparse.pool_rows(table, ids, off, mode="max")
    cfg = ncf.EmbeddingBagConfig(num_embeddings=10, embedding_dim=16, name="t",
                                 feature_names=["user_hist"])
    ebc = ncf.EmbeddingBagCollection([cfg], is_weighted=True)
    k = KJT.from_lengths_sync(keys=["user_hist"], values=ids, lengths=torch.tensor([2, 1]))
    with pytest.raises(ValueError, match="weights"):
        ebc(k)
    mean = ncf.EmbeddingBagConfig(num_embeddings=10, embedding_dim=16, name="t",
                                  feature_names=["user_hist"], pooling=ncf.PoolingType.MEAN)
    kw = KJT.from_lengths_sync(keys=["user_hist"], values=ids, lengths=torch.tensor([2, 1]),
                               weights=torch.ones(3))
    with pytest.raises(ValueError, match="SUM pooling only"):
        ncf.EmbeddingBagCollection([mean], is_weighted=True)(kw)


def test_no_cpu_fallback():
    table = torch.zeros(10, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse.pool_rows(table, torch.tensor([1, 2, 3]), torch.tensor([0, 2, 3]))
    cfg = ncf.EmbeddingBagConfig(num_embeddings=10, embedding_dim=16, name="t",
                                 feature_names=["user_hist"])
    k = KJT.from_lengths_sync(keys=["user_hist"], values=torch.tensor([1, 2, 3]),
                              lengths=torch.tensor([2, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncf.EmbeddingBagCollection([cfg])(k)
    assert ncf.pool_rows is sparse.pool_rows
