"""The CPU oracle's MultiHeadAttention against F10 (the reference's module with a key/value length
that differs from the query length, masked and not): O.mha restates ``.view(B, -1, H, hd)``, so it
already covers these shapes.  tests/test_gpu_xattn.py compares the HIP path with it where the
fixture holds no recorded call (dropout on, a fully masked row).  Tolerances:
test_oracle_golden.test_f4_mha's."""
import numpy as np
import pytest
import torch

from oracle import ncf_oracle as O
from tests import xattn_cases as X
from tests.conftest import sub


def test_fixture_holds_every_case():
    f = X.f10()
    assert sorted({k.split("/")[0] for k in f}) == sorted(X.ALL)
    shapes = {t: tuple(int(x) for x in f[f"{t}/shape"]) for t in X.BASE}
    assert shapes == {"x1_50": (4, 1, 50, 64, 4), "x3_7": (5, 3, 7, 64, 4),
                      "x64_33": (2, 64, 33, 128, 8), "x7_64_h1": (3, 7, 64, 16, 1),
                      "x2_9_hd64": (3, 2, 9, 64, 1), "x5_12_hd8": (3, 5, 12, 32, 4),
                      "x4_40_hd32": (2, 4, 40, 64, 2)}
    for t in X.MASKED:
        Bn, Lq, Lk, D, H = shapes[t]
        pad, ph = f[f"{t}@padding/mask"], f[f"{t}@per_head/mask"]
        assert pad.shape == (Bn, 1, 1, Lk) and ph.shape == (Bn, H, Lq, Lk)
        assert ph[..., 0].all() and pad[..., 0].all() and not ph.all()
    assert f["x1_50@q2d/q"].shape == (4, 64)


@pytest.mark.parametrize("tag", X.ALL)
def test_f10_mha(tag):
    c = X.case(tag)
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    w = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sub(c, "w/").items()}
    q, k, v = [torch.from_numpy(c[n]).requires_grad_(True) for n in "qkv"]
    assert k.shape == (Bn, Lk, D) and v.shape == (Bn, Lk, D)
    mask = torch.from_numpy(c["mask"]) if "mask" in c else None
    # (a 2-D query is a length-1 sequence: the oracle takes it 3-D)
    y = O.mha(w, "", q if q.dim() == 3 else q.unsqueeze(1), k, v, H, mask=mask)
    assert tuple(y.shape) == (Bn, Lq, D) == c["y"].shape
    np.testing.assert_allclose(y.detach().numpy(), c["y"], atol=1e-5, rtol=1e-5)
    y.backward(torch.from_numpy(c["gy"]))
    for n, t in zip("qkv", (q, k, v)):
        np.testing.assert_allclose(t.grad.numpy(), c[f"g{n}"], atol=1e-5, rtol=1e-4)
    for n, t in w.items():
        np.testing.assert_allclose(t.grad.numpy(), c[f"gw/{n}"], atol=1e-5, rtol=1e-4)
