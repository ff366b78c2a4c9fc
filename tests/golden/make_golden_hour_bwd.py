#!/usr/bin/env python3
"""Generate the golden fixture F11 from the REFERENCE implementation: the gradients of
``AdvancedNCF.forward_simple(user_ids, product_ids, hour)`` (src/model/architecture.py:409-485).

    python tests/golden/make_golden_hour_bwd.py --reference <checkout of the reference>

Imports the reference's own ``src/model/architecture.py`` the way make_goldens.py does (the
offline torchrec stand-in first on sys.path), builds its AdvancedNCF with dropout 0 in train()
mode, runs ``forward_simple(u, p, hour)`` and ``BCELoss(out, targets).backward()``.

When temporal_dim != mf_embedding_dim the reference draws a fresh ``nn.Linear(T, D)`` inside the
call (:436-442).  ``torch.manual_seed(s)`` directly before the call pins it: the same seed directly
before a stand-alone ``nn.Linear(T, D)`` reproduces its weights, which is how they are recorded.

F11 f11_hour_bwd*.npz (arrays only), per case <tag>:
  <tag>/shape = (U, I, D, T, H, n), <tag>/hidden, <tag>/sd/<state_dict key>, <tag>/u, p, hour,
  targets, <tag>/proj_w, proj_b (T != D only), <tag>/out, <tag>/loss,
  <tag>/g/<parameter name> for every parameter whose .grad is not None,
  <tag>/nograd = the names of the parameters left without a gradient, '\n'-joined bytes.
Hours are drawn from 5 distinct values, so repeats are heavy and 19 hour rows stay absent.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import import_reference, savez_parts  # noqa: E402

# tag: (U, I, D, T, hidden, H, n), seed
CASES = {
    "h16_8": ((11, 7, 16, 8, [32, 16], 2, 37), 1608),
    "h64_32": ((13, 9, 64, 32, [256, 128, 64], 4, 70), 6432),
    "h32_32": ((13, 9, 32, 32, [64, 32], 4, 33), 3232),       # T == D: no projection
}
HOURS = (0, 5, 11, 17, 23)
PROJ_SEED = 777


def make_f11(AdvancedNCF):
    out = {}
    for tag, ((U, I, D, T, hidden, H, n), seed) in CASES.items():
        torch.manual_seed(seed)
        m = AdvancedNCF(U, I, 5, 24, D, D, T, hidden, H, 0.0, 4)
        m.train()
        g = torch.Generator().manual_seed(seed + 1)
        u = torch.randint(0, U, (n,), generator=g)
        p = torch.randint(0, I, (n,), generator=g)
        hour = torch.tensor(HOURS)[torch.randint(0, len(HOURS), (n,), generator=g)]
        assert len(set(hour.tolist())) == len(HOURS)
        targets = (torch.rand(n, generator=g) < 0.4).float()
        out[f"{tag}/shape"] = np.array([U, I, D, T, H, n], np.int64)
        out[f"{tag}/hidden"] = np.array(hidden, np.int64)
        for k, v in m.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.detach().numpy().astype(np.float32).copy()
        out[f"{tag}/u"], out[f"{tag}/p"] = u.numpy(), p.numpy()
        out[f"{tag}/hour"], out[f"{tag}/targets"] = hour.numpy(), targets.numpy()
        if T != D:
            torch.manual_seed(PROJ_SEED + seed)
            lin = torch.nn.Linear(T, D)
            out[f"{tag}/proj_w"] = lin.weight.detach().numpy().copy()
            out[f"{tag}/proj_b"] = lin.bias.detach().numpy().copy()
        torch.manual_seed(PROJ_SEED + seed)
        y = m.forward_simple(u, p, hour)
        loss = torch.nn.BCELoss()(y, targets)
        loss.backward()
        out[f"{tag}/out"] = y.detach().numpy().copy()
        out[f"{tag}/loss"] = np.array(loss.item(), np.float64)
        nograd = []
        for name, prm in m.named_parameters():
            if prm.grad is None:
                nograd.append(name)
            else:
                out[f"{tag}/g/{name}"] = prm.grad.numpy().astype(np.float32).copy()
        out[f"{tag}/nograd"] = np.frombuffer("\n".join(nograd).encode(), np.uint8).copy()
        print(tag, "gradients:", sum(1 for k in out if k.startswith(f"{tag}/g/")),
              "none:", len(nograd))
    out = {k_: np.ascontiguousarray(v_) for k_, v_ in out.items()}
    savez_parts("f11_hour_bwd.npz", out)
    print("F11 written:", sum(v_.nbytes for v_ in out.values()), "bytes of arrays")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    a = ap.parse_args()
    torch.set_num_threads(8)
    AdvancedNCF = import_reference(a.reference)[0]
    make_f11(AdvancedNCF)


if __name__ == "__main__":
    main()
