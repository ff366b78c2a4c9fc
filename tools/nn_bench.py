"""Timing of the exact nearest-product search against what a user would otherwise write,
``torch.topk(q @ V.T, k)`` on the same device and tensors (GPU only).

    python tools/nn_bench.py [--items 100000,1000000] [--queries 1,32,256] [--k 10,100]
                             [--rounds 9] [--reps 20] [--out FILE]

Per shape: after a warm-up of both, ``rounds`` rounds alternate ``reps`` calls of
``ProductSearch.find_neighbors`` with ``reps`` of the baseline, each timed with device events; the
figures are the medians over the rounds (us per call).  ``scan_us`` is ``ncf_nn_scan`` alone on
the same plan, and ``scan_TBps`` is ``I * D * 4 * blocks / t`` (the matrix is read once per block
of 32 queries), to set beside the 6.29 TB/s measured copy rate of the part (a 256 MB matrix sits
at the edge of the 256 MiB Infinity Cache, so warm figures may exceed the HBM rate).  Prints one
JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

_ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402
from ncf_amd._lib import ptr  # noqa: E402
from ncf_amd.neighbors import QUERY_BLOCK, ProductSearch, plan  # noqa: E402

DEV = torch.device("cuda")
D = 64


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="100000,1000000")
    ap.add_argument("--queries", default="1,32,256")
    ap.add_argument("--k", default="10,100")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nn_bench: no GPU (a timing needs the MI355X)")
    lines = []
    for I in (int(x) for x in args.items.split(",")):
        g = torch.Generator().manual_seed(I)
        index = ProductSearch.from_vectors(torch.randn(I, D, generator=g).to(DEV))
        V = index.vectors
        for n in (int(x) for x in args.queries.split(",")):
            q = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).to(DEV)
            for k in (int(x) for x in args.k.split(",")):
                blocks = -(-n // QUERY_BLOCK)
                pl = plan(I, k, None, blocks)
                slabs = pl.g1 * pl.g2
                ps = torch.empty(n, slabs, k, device=DEV)
                pi = torch.empty(n, slabs, k, dtype=torch.int64, device=DEV)
                st = _lib.stream_ptr(DEV)
                ours = lambda: index.find_neighbors(q, k)   # noqa: E731
                base = lambda: torch.topk(q @ V.T, k)       # noqa: E731
                scan = lambda: _lib.call(  # noqa: E731
                    "ncf_nn_scan", ptr(q), n, 1, ptr(V), I, D, None, None, None, pl.slab_items,
                    slabs, k, ptr(ps), ptr(pi), st)
                s, i = ours()
                bs, bi = base()
                same = float((i == bi).float().mean())      # (ties and rounding may differ)
                for fn in (ours, base, scan):
                    timed(fn, 3)
                t = {"ours": [], "base": [], "scan": []}
                for _ in range(args.rounds):
                    t["ours"].append(timed(ours, args.reps))
                    t["base"].append(timed(base, args.reps))
                    t["scan"].append(timed(scan, args.reps))
                med = {name: statistics.median(v) for name, v in t.items()}
                rec = {"items": I, "queries": n, "k": k, "slabs": pl.n_slabs,
                       "slab_items": pl.slab_items, "merge_levels": 1 if pl.g1 == 1 else 2,
                       "ours_us": round(med["ours"], 1), "torch_us": round(med["base"], 1),
                       "scan_us": round(med["scan"], 1),
                       "ours_minmax_us": [round(min(t["ours"]), 1), round(max(t["ours"]), 1)],
                       "torch_minmax_us": [round(min(t["base"]), 1), round(max(t["base"]), 1)],
                       "scan_TBps": round(I * D * 4 * blocks / med["scan"] / 1e6, 2),
                       "ids_equal_torch": round(same, 5)}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
