"""The gradients of forward_simple(user_ids, product_ids, hour) on the CPU: the float64 oracle
(autograd through oracle.forward_simple_hour) against F11, the reference's own gradients
(tests/golden/make_golden_hour_bwd.py), and the host-side pieces of the opt-in backward.

Bounds: output atol 1e-5 / rtol 1e-5; every gradient |d| <= 1e-6 + 1e-4 |ref| (1e-6 is the
gradient abs tolerance of tests/parity.py, the rtol test_f10's).  Measured on the three cases: the
worst abs difference 5.2e-8, the worst relative to a tensor's max 8.9e-7."""
import os
import re

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import hour_cases as C

ncf = _ncf_pkg.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(c):
    sd = C.T_(C.sub(c, "sd/"))
    proj = (torch.from_numpy(c["proj_w"]), torch.from_numpy(c["proj_b"])) if "proj_w" in c else None
    t = C.T_({k: c[k] for k in ("u", "p", "hour", "targets")})
    return C.oracle_grads(sd, t["u"], t["p"], t["hour"], t["targets"], proj, c["H"], len(c["hid"]))


@pytest.mark.parametrize("tag", C.CASES)
def test_oracle_float64_vs_f11(tag):
    c = C.case(tag)
    out, grads = _ref(c)
    np.testing.assert_allclose(out.numpy(), c["out"], atol=1e-5, rtol=1e-5)
    ref = C.sub(c, "g/")
    assert 31 <= len(ref) <= 35
    for name, g in ref.items():
        assert grads[name] is not None, name
        C.assert_grad_close(name, grads[name].numpy(), g)
    for name in c["nograd_names"]:
        assert grads[name] is None, name


@pytest.mark.parametrize("tag", C.CASES)
def test_f11_reference_gradient_facts(tag):
    """What the reference's own gradients look like: the temporal columns of mlp.0.weight train,
    hour_embed gets exactly the batch's 5 hours, q_proj / k_proj get zero TENSORS, and the
    modules forward_simple never calls get nothing."""
    c = C.case(tag)
    g = C.sub(c, "g/")
    D = c["D"]
    assert np.abs(g["mlp.0.weight"][:, D:]).max() > 1e-4
    gh = g[C.HOUR_W]
    assert gh.shape == (24, c["T"])
    rows = np.flatnonzero(np.abs(gh).sum(1))
    assert sorted(rows.tolist()) == sorted(set(c["hour"].tolist())) and len(rows) == 5
    for nm in ("q_proj", "k_proj"):
        for t in ("weight", "bias"):
            assert not g[f"user_product_attention.{nm}.{t}"].any()
    assert len(c["nograd_names"]) == 26
    for name in c["nograd_names"]:
        assert name.startswith(C.UNTOUCHED), name
    listed = [k for k in C.sub(c, "sd/") if k.startswith(C.UNTOUCHED) and not k.endswith(".pe")]
    assert sorted(listed) == sorted(c["nograd_names"])


def test_hour_grad_chunk_mirrors_the_kernel():
    """ops.HOUR_GRAD_CHUNK is the piece length ncf_hour_grad's ordered reduction is cut at."""
    from ncf_amd import ops
    src = open(os.path.join(ROOT, "neural-collaborative-filtering-demo_amd", "csrc",
                            "hour_bwd.hip")).read()
    assert int(re.search(r"#define NCF_HOUR_CHUNK (\d+)", src).group(1)) == ops.HOUR_GRAD_CHUNK


def test_switch_is_a_plain_attribute_and_the_refusal_names_it():
    """model.hour_backward is no parameter or buffer (no state_dict key); without it a
    training-mode call with gradients enabled is refused, and the message names the switch."""
    m = ncf.AdvancedNCF(6, 5, 5, 24, 16, 16, 8, [32, 16], 2, 0.0, 4)
    keys = list(m.state_dict().keys())
    m.train()
    u = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="hour_backward"):
        m.forward_simple(u, u, u)
    m.hour_backward = True
    assert list(m.state_dict().keys()) == keys
    assert "hour_backward" not in dict(m.named_parameters()) and \
        "hour_backward" not in dict(m.named_buffers())
