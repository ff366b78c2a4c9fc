"""The F11 fixture (tests/golden/make_golden_hour_bwd.py: the reference's own gradients of
forward_simple(user_ids, product_ids, hour)) as per-case dicts, and the float64 reference of the
hour path's gradients (autograd through oracle.forward_simple_hour) — TEST INFRASTRUCTURE ONLY.
"""
import functools

import numpy as np
import torch

from oracle import ncf_oracle as O
from tests.conftest import load_npz, sub

CASES = ["h16_8", "h64_32", "h32_32"]
HOUR_W = "temporal_encoding.hour_embed.weight"
# what forward_simple(hour) leaves without a gradient in the reference
UNTOUCHED = ("temporal_encoding.day_embed.", "temporal_encoding.month_embed.",
             "category_hierarchy.", "sequence_attention.", "feature_combination.")
ATOL, RTOL = 1e-6, 1e-4       # gradients: tests/parity.py's abs tolerance, test_f10's rtol


@functools.lru_cache(maxsize=None)
def f11():
    return load_npz("f11_hour_bwd.npz")


def case(tag):
    c = dict(sub(f11(), tag + "/"))
    U, I, D, T, H, n = [int(x) for x in c["shape"]]
    c.update(U=U, I=I, D=D, T=T, H=H, n=n, hid=[int(x) for x in c["hidden"]],
             nograd_names=bytes(c["nograd"]).decode().split("\n"))
    return c


def T_(d, dtype=None):
    out = {}
    for k, v in d.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        out[k] = t.to(dtype) if dtype is not None and t.is_floating_point() else t
    return out


def oracle_grads(sd, u, p, hour, targets, proj, H, n_layers, attn_drop=None, mlp_masks=None,
                 grad_out=None):
    """Float64 autograd through O.forward_simple_hour.  ``sd``: {state_dict key: tensor};
    ``proj``: (weight, bias) or None (T == D).  The loss is BCE(out, targets) (mean), or
    sum(out * grad_out) when ``grad_out`` is given.  Returns (out, {name: grad or None}) with the
    projection's gradients under "proj_w" / "proj_b"."""
    f64 = lambda t: t.detach().cpu().to(torch.float64)  # noqa: E731
    leaves = {k: (f64(v).requires_grad_(True) if v.is_floating_point() and not k.endswith(".pe")
                  else v.detach().cpu()) for k, v in sd.items()}
    pw = pb = None
    if proj is not None:
        pw, pb = (f64(t).requires_grad_(True) for t in proj)
    sc = lambda t: None if t is None else f64(t)  # noqa: E731
    out = O.forward_simple_hour(leaves, u.cpu(), p.cpu(), hour.cpu(), pw, pb, num_heads=H,
                                n_layers=n_layers, attn_drop=sc(attn_drop),
                                mlp_masks=None if mlp_masks is None else [f64(t) for t in mlp_masks])
    if grad_out is None:
        loss = O.bce_loss(out, f64(targets))
    else:
        loss = (out * f64(grad_out)).sum()
    names = [k for k, v in leaves.items() if v.requires_grad]
    ins = [leaves[k] for k in names] + ([pw, pb] if proj is not None else [])
    gs = torch.autograd.grad(loss, ins, allow_unused=True)
    grads = dict(zip(names + (["proj_w", "proj_b"] if proj is not None else []), gs))
    return out.detach(), grads


def assert_grad_close(name, got, ref, atol=ATOL, rtol=RTOL):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite gradient"
    d = np.abs(got - ref)
    bad = d > atol + rtol * np.abs(ref)
    assert not bad.any(), (f"{name}: {bad.sum()} of {d.size} elements differ, max |d| "
                           f"{d.max():.3e} (|ref| max {np.abs(ref).max():.3e})")
