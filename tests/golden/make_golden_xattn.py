#!/usr/bin/env python3
"""Generate the golden fixture F10 from the REFERENCE implementation: MultiHeadAttention with a
key/value length that differs from the query length.

    python tests/golden/make_golden_xattn.py --reference <checkout of the reference>

Imports the reference's own ``src/model/architecture.py`` the way make_goldens.py does (the
offline torchrec stand-in first on sys.path) and runs its MultiHeadAttention (dropout 0) forward
and backward on seeded inputs.  The module reshapes q, k and v each with
``.view(batch, -1, H, hd)`` (architecture.py:40-42), so the key length is free of the query
length; ``sequence_attention`` (:210-214) is the instance meant for one query over a user's item
history (config/config.yaml:202 max_sequence_length: 50).

F10 f10_xattn*.npz, in F4's key scheme (arrays only):
  <tag>/q, k, v, y, gy, gq, gk, gv, w/<param>, gw/<param>, shape = (B, L_q, L_k, D, H)
and for a variant of a case (same module, same k, v and gy; the keys it does not hold are the
base case's):
  <tag>@padding/mask [B, 1, 1, L_k]   key-padding mask, lengths drawn in 1..L_k
  <tag>@per_head/mask [B, H, L_q, L_k] random mask, keep 0.6, key 0 always kept
  <tag>@q2d/q [B, D]                  the base query given 2-D (a length-1 sequence)
each with its own y, gq, gk, gv, gw/<param>.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import import_reference, savez_parts  # noqa: E402

# tag: (B, L_q, L_k, D, H), seed, variants
CASES = {
    "x1_50": ((4, 1, 50, 64, 4), 1050, ("padding", "per_head", "q2d")),   # sequence_attention
    "x3_7": ((5, 3, 7, 64, 4), 1037, ("padding", "per_head")),            # both lengths small
    "x64_33": ((2, 64, 33, 128, 8), 6433, ()),                            # L_q > L_k, D = 128
    "x7_64_h1": ((3, 7, 64, 16, 1), 7641, ("padding", "per_head")),       # L_k at its limit
    "x2_9_hd64": ((3, 2, 9, 64, 1), 2964, ()),                            # head dim 64
    "x5_12_hd8": ((3, 5, 12, 32, 4), 5128, ()),                           # head dim 8
    "x4_40_hd32": ((2, 4, 40, 64, 2), 4432, ()),                          # head dim 32
}


def run(m, q, k, v, gy, mask):
    """One forward + backward of the reference module: y and every gradient, as numpy."""
    m.zero_grad()
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    y = m(q, k, v) if mask is None else m(q, k, v, mask)
    y.backward(gy)
    out = {"y": y.detach().numpy(), "gq": q.grad.numpy(), "gk": k.grad.numpy(),
           "gv": v.grad.numpy()}
    for n, p in m.named_parameters():
        out["gw/" + n] = p.grad.numpy().copy()
    return out


def make_f10(MultiHeadAttention):
    out = {}
    for tag, ((Bn, Lq, Lk, D, H), seed, variants) in CASES.items():
        torch.manual_seed(seed)
        m = MultiHeadAttention(D, H, dropout=0.0)
        q = torch.randn(Bn, Lq, D)
        k = torch.randn(Bn, Lk, D)
        v = torch.randn(Bn, Lk, D)
        gy = torch.randn(Bn, Lq, D)
        g = torch.Generator().manual_seed(seed + 1)
        out[f"{tag}/shape"] = np.array([Bn, Lq, Lk, D, H], np.int64)
        out[f"{tag}/q"], out[f"{tag}/k"], out[f"{tag}/v"] = q.numpy(), k.numpy(), v.numpy()
        out[f"{tag}/gy"] = gy.numpy()
        for n, p in m.named_parameters():
            out[f"{tag}/w/{n}"] = p.detach().numpy().copy()
        for n, a in run(m, q, k, v, gy, None).items():
            out[f"{tag}/{n}"] = a
        for var in variants:
            qv, mask = q, None
            if var == "padding":
                lens = torch.randint(1, Lk + 1, (Bn,), generator=g)
                mask = (torch.arange(Lk)[None, :] < lens[:, None]).view(Bn, 1, 1, Lk)
            elif var == "per_head":
                mask = torch.rand(Bn, H, Lq, Lk, generator=g) < 0.6
                mask[..., 0] = True
            else:
                assert var == "q2d" and Lq == 1
                qv = q[:, 0]
                out[f"{tag}@{var}/q"] = qv.numpy().copy()
            if mask is not None:
                out[f"{tag}@{var}/mask"] = mask.numpy().astype(np.uint8)
            for n, a in run(m, qv, k, v, gy, mask).items():
                out[f"{tag}@{var}/{n}"] = a
            assert np.isfinite(out[f"{tag}@{var}/y"]).all()
    out = {k_: np.ascontiguousarray(v_) for k_, v_ in out.items()}
    savez_parts("f10_xattn.npz", out)
    print("F10 written:", sum(v_.nbytes for v_ in out.values()), "bytes of arrays")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    a = ap.parse_args()
    torch.set_num_threads(8)
    _, MHA, _, _ = import_reference(a.reference)
    make_f10(MHA)


if __name__ == "__main__":
    main()
