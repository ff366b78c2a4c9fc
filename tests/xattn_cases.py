"""The F10 fixture (tests/golden/make_golden_xattn.py: the reference's MultiHeadAttention with a
key/value length that differs from the query length) as per-case dicts — TEST INFRASTRUCTURE ONLY.

A base case holds q, k, v, y, gy, gq, gk, gv, w/<param>, gw/<param>, shape = (B, L_q, L_k, D, H).
A variant ``<tag>@padding`` / ``@per_head`` (a mask) / ``@q2d`` (the query given 2-D) holds what
differs from its base (mask or q, and y and the gradients); ``case`` fills in the rest.
"""
import functools

import numpy as np
import torch

from tests.conftest import load_npz, sub

BASE = ["x1_50", "x3_7", "x64_33", "x7_64_h1", "x2_9_hd64", "x5_12_hd8", "x4_40_hd32"]
MASKED = ["x1_50", "x3_7", "x7_64_h1"]
ALL = BASE + [f"{t}@{k}" for t in MASKED for k in ("padding", "per_head")] + ["x1_50@q2d"]


@functools.lru_cache(maxsize=None)
def f10():
    return load_npz("f10_xattn.npz")


def case(tag):
    f = f10()
    d = dict(sub(f, tag.split("@")[0] + "/"))
    if "@" in tag:
        d.update(sub(f, tag + "/"))
    return d


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
