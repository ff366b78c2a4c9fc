"""Sparse table gradients and ``ncf_amd.SparseAdam``, the part that needs no GPU: the header's
flag and workspace offsets (and that no entry point or struct came with them), the new keyword
arguments and their defaults, the refusals raised before any device work, the step-table entries
the optimizer hands ``ncf_adam_rows_apply``, and the premise of tests/test_gpu_bag_sparse.py: the
float64 restatement (tests/sparse_adam_ref.py) is ``torch.optim.SparseAdam`` on the CPU, its
float32 form sits inside its own bound with room, and a step count off by one does not."""
import inspect
import os

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import sparse_adam_ref as S
from tests.conftest import ROOT

ncf = _ncf_pkg.load()
from ncf_amd import _abi, _lib, optim, sparse  # noqa: E402


def test_header_defines_the_flag_and_adds_no_entry_point():
    functions, structs, defines = _abi.parse_header(os.path.join(ROOT, "include", "ncf_hip.h"))
    assert len(functions) == 148 and len(structs) == 11
    assert defines["NCF_BAG_COMPACT"] == 0x100 == _lib.BAG_COMPACT
    assert (defines["NCF_BAG_WS_COUNT_OFFSET"], defines["NCF_BAG_WS_IDS_OFFSET"]) == (0, 256)
    assert (_lib.BAG_WS_COUNT_OFFSET, _lib.BAG_WS_IDS_OFFSET) == (0, 256)
    assert defines["NCF_BAG_COMPACT"] & 1 == 0          # (the flag leaves the mode bit alone)
    for name, count in (("ncf_bag_pool_fwd", 12), ("ncf_bag_pool_bwd_workspace", 3),
                        ("ncf_bag_pool_bwd", 15), ("ncf_adam_rows_apply", 21)):
        assert len(_lib.SIGNATURES[name][1]) == count, name
    # one workspace size for both forms, and the ids' block fits before the scratch
    for n in (0, 1, 35, 8000):
        assert _lib.query("ncf_bag_pool_bwd_workspace", n, 67, 64) >= 256 + 8 * n


def test_new_keyword_arguments_default_to_the_old_behaviour():
    p = inspect.signature(sparse.pool_rows).parameters
    assert list(p) == ["table", "ids", "offsets", "weights", "mode", "check", "sparse"]
    assert p["sparse"].default is False
    e = inspect.signature(sparse.EmbeddingBagCollection.__init__).parameters
    assert list(e) == ["self", "tables", "device", "is_weighted", "sparse"]
    assert e["sparse"].default is False
    cfg = ncf.EmbeddingBagConfig(num_embeddings=10, embedding_dim=16, name="t",
                                 feature_names=["user_hist"])
    assert ncf.EmbeddingBagCollection([cfg])._sparse is False
    assert ncf.EmbeddingBagCollection([cfg], sparse=True)._sparse is True
    assert ncf.SparseAdam is optim.SparseAdam and issubclass(ncf.SparseAdam, torch.optim.Optimizer)
    # the old refusals come first with sparse=True too
    table = torch.zeros(10, 16)
    ids, off = torch.tensor([1, 2, 3]), torch.tensor([0, 2, 3])
    with pytest.raises(ValueError, match="mode"):
        sparse.pool_rows(table, ids, off, mode="max", sparse=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sparse.pool_rows(table, ids, off, sparse=True)
    for doc in (sparse.__doc__, sparse.pool_rows.__doc__, sparse.EmbeddingBagCollection.__doc__):
        assert "sparse=True" in doc and "sparse (COO) gradients, bf16" not in doc


def test_sparse_adam_refusals_that_need_no_device():
    ok = torch.nn.Parameter(torch.zeros(10, 16))
    with pytest.raises(ValueError, match="maximize"):
        ncf.SparseAdam([ok], maximize=True)
    for bad in (torch.zeros(10, 24), torch.zeros(10), torch.zeros(2, 5, 16),
                torch.zeros(10, 16, dtype=torch.float64), torch.zeros(10, 16, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="width"):
            ncf.SparseAdam([torch.nn.Parameter(bad)])
    with pytest.raises(ValueError, match="learning rate"):
        ncf.SparseAdam([ok], lr=0.0)
    with pytest.raises(ValueError, match="beta"):
        ncf.SparseAdam([ok], betas=(0.9, 1.0))
    opt = ncf.SparseAdam([ok], lr=1e-3)
    assert opt.defaults == torch.optim.SparseAdam([torch.nn.Parameter(torch.zeros(2, 2))],
                                                  lr=1e-3).defaults
    assert opt.step() is None                            # no gradient: nothing to do
    ok.grad = torch.zeros(10, 16)
    with pytest.raises(RuntimeError, match="dense gradients"):
        opt.step()
    ok.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]]), torch.ones(2, 16), (10, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        opt.step()


def test_step_table_entries_are_sparse_adams_step_size():
    lr, betas, eps = 3e-4, (0.9, 0.999), 1e-8
    tab = optim.sparse_step_scalars(lr, betas, eps, 7, 300)
    assert tab.dtype == np.float32 and tab.shape == (300, 4)
    for i in (0, 1, 150, 299):
        ns = -S.step_size(lr, betas, 7 + i)
        assert tab[i, 0] == np.float32(ns) and tab[i, 1] == 1.0
        assert tab[i, 2] == np.float32(1.0 / ns) and tab[i, 3] == np.float32(eps / ns)
    opt = ncf.SparseAdam([torch.nn.Parameter(torch.zeros(10, 16))])
    dev = torch.device("cpu")
    t0, at = opt._table_entry(dev, lr, betas, eps, 7)
    assert at == 1 and np.array_equal(t0[1].numpy(), tab[0])
    t1, at = opt._table_entry(dev, lr, betas, eps, 7 + 255)          # the same window
    assert t1 is t0 and at == 256 and np.array_equal(t1[256].numpy(), tab[255])
    t2, at = opt._table_entry(dev, lr, betas, eps, 7 + 256)          # the next one
    assert t2 is not t0 and at == 1 and np.array_equal(t2[1].numpy(), tab[256])
    assert tuple(t0.shape) == tuple(t2.shape) == (257, 4)
    # an lr seen for the first time while another is in use: that one step's scalars only; if
    # it stays, its full window; the first lr's table is still there
    t3, at = opt._table_entry(dev, 2 * lr, betas, eps, 8)
    assert tuple(t3.shape) == (2, 4) and at == 1
    assert t3[1, 0] == np.float32(-S.step_size(2 * lr, betas, 8))
    t4, at = opt._table_entry(dev, 2 * lr, betas, eps, 9)
    assert tuple(t4.shape) == (257, 4) and at == 1
    assert t4[1, 0] == np.float32(-S.step_size(2 * lr, betas, 9))
    assert opt._table_entry(dev, 2 * lr, betas, eps, 200)[0] is t4
    assert opt._table_entry(dev, lr, betas, eps, 7 + 300)[0] is t2
    # a scheduler's lr per step: one small table each, at most 8 kept, the oldest dropped
    for s in range(20):
        t, at = opt._table_entry(dev, lr * (3 + s), betas, eps, 10 + s)
        assert at == 1 and tuple(t.shape) == (2, 4)
        assert t[1, 0] == np.float32(-S.step_size(lr * (3 + s), betas, 10 + s))
    assert len(opt._tables) == 8 and (dev, lr * 22, betas, eps) in opt._tables


def _torch_sparse_adam(case, dtype, stock_steps=None):
    p = torch.nn.Parameter(torch.tensor(case["p"], dtype=dtype))
    opt = torch.optim.SparseAdam([p], lr=S.LRS[0], betas=S.BETAS, eps=S.EPS)
    for ids, vals, lr in case["steps"]:
        opt.param_groups[0]["lr"] = lr
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None], torch.tensor(vals, dtype=dtype),
                                         p.shape)
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("dim", (16, 64))
def test_float64_restatement_is_torch_sparse_adam(dim):
    case = S.make_case(dim)
    ref = S.run(case, S.F64)
    got = _torch_sparse_adam(case, torch.float64)
    d = S.distance(got, ref, case["touched"])
    print(f"restatement vs torch.optim.SparseAdam (float64) dim={dim}: {d}")
    assert d["p"] <= 1e-15 and d["m"] <= 1e-14 and d["v"] <= 1e-14
    for a, b0 in zip(got, (case["p"].astype(S.F64), 0.0, 0.0)):     # rows never named
        assert (a[~case["touched"]] == (b0[~case["touched"]] if np.ndim(b0) else b0)).all()
    # the bound: the float32 restatement uses a quarter of it by construction, torch's own
    # float32 SparseAdam (another order of the same operations) stays inside it, and a step
    # count off by one (the bias corrections of the wrong step) does not
    bound, fp = S.bounds(case, ref)
    print(f"float32 restatement's distance: {fp}")
    assert all(0 < fp[q] < 1e-5 for q in "pmv")
    t32 = S.distance(_torch_sparse_adam(case, torch.float32), ref, case["touched"])
    print(f"torch float32 / bound: { {q: t32[q] / bound[q] for q in 'pmv'} }")
    assert all(t32[q] < bound[q] for q in "pmv")
    off = S.distance(S.run(case, S.F64, step_shift=1), ref, case["touched"])
    assert off["p"] > 20 * bound["p"]
