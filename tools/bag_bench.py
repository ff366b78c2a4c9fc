"""Timing of the pooled lookup (``pool_rows``: ncf_bag_pool_fwd / ncf_bag_pool_bwd) against what a
user would otherwise write, ``torch.nn.functional.embedding_bag`` on the same device and tensors
(GPU only).

    python tools/bag_bench.py [--rows 100000,1000000] [--bags 4096,20480] [--rounds 9]
                              [--reps 20] [--out FILE]

Shapes: tables of ``rows`` x 64, bags of 50 ids (the reference's purchase-history length,
03_create_feature_views.py LIMIT 50) with uniform ids, and ragged bags of 0..50 ids drawn
Zipf(1.05) (the skew of the step benchmark), SUM and MEAN.  Per shape: after a warm-up of both
sides, ``rounds`` rounds alternate ``reps`` calls of ``pool_rows(check=False)`` with ``reps`` of
``embedding_bag``, each timed with device events, forward alone and forward + backward with a
dense table gradient on both sides; the figures are the medians over the rounds (us per call).
``fwd_bytes`` is what the algorithm needs (``n_ids * dim * 4`` read + ``bags * dim * 4``
written) and ``fwd_TBps`` that over the forward's time, to set beside the 6.29 TB/s measured copy
rate of the part.  A 100K x 64 table (25.6 MB) is served by the caches, and a 1M x 64 table
(256 MB) sits at the edge of the 256 MiB Infinity Cache, so warm figures may exceed the HBM rate;
the ids themselves (8 B each) are not counted.  Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

_ncf_pkg.load()
from ncf_amd.sparse import pool_rows  # noqa: E402

DEV = torch.device("cuda")
D = 64
HISTORY = 50


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # us


def make_ids(rows, bags, ragged, seed):
    rng = np.random.RandomState(seed)
    if ragged:
        lengths = rng.randint(0, HISTORY + 1, size=bags)
        ids = (rng.zipf(1.05, size=int(lengths.sum())) - 1) % rows
    else:
        lengths = np.full(bags, HISTORY)
        ids = rng.randint(0, rows, size=bags * HISTORY)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return torch.from_numpy(ids.astype(np.int64)).to(DEV), torch.from_numpy(off).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--bags", default="4096,20480")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bag_bench: no GPU (a timing needs the MI355X)")
    lines = []
    for rows in (int(x) for x in args.rows.split(",")):
        g = torch.Generator().manual_seed(rows)
        table = torch.randn(rows, D, generator=g).to(DEV).requires_grad_(True)
        frozen = table.detach()
        for bags in (int(x) for x in args.bags.split(",")):
            gout = torch.randn(bags, D, generator=g).to(DEV)
            for ragged in (False, True):
                ids, off = make_ids(rows, bags, ragged, seed=rows + bags)
                n = ids.numel()
                top = int(torch.bincount(ids).max())
                for mode in ("sum", "mean"):
                    def ours_f():
                        return pool_rows(frozen, ids, off, None, mode, check=False)

                    def base_f():
                        return torch.nn.functional.embedding_bag(
                            ids, frozen, off, mode=mode, include_last_offset=True)

                    def ours_fb():
                        table.grad = None
                        pool_rows(table, ids, off, None, mode, check=False).backward(gout)

                    def base_fb():
                        table.grad = None
                        torch.nn.functional.embedding_bag(
                            ids, table, off, mode=mode, include_last_offset=True).backward(gout)

                    diff = float((ours_f() - base_f()).abs().max())
                    ours_fb()
                    g_ours = table.grad.clone()
                    base_fb()
                    gdiff = float((g_ours - table.grad).abs().max())
                    fns = {"ours_fwd": ours_f, "torch_fwd": base_f, "ours_fwd_bwd": ours_fb,
                           "torch_fwd_bwd": base_fb}
                    for fn in fns.values():
                        timed(fn, 3)
                    t = {name: [] for name in fns}
                    for _ in range(args.rounds):
                        for name, fn in fns.items():
                            t[name].append(timed(fn, args.reps))
                    med = {name: statistics.median(v) for name, v in t.items()}
                    nbytes = n * D * 4 + bags * D * 4
                    rec = {"rows": rows, "dim": D, "bags": bags,
                           "lengths": "0..50 zipf(1.05)" if ragged else "50", "mode": mode,
                           "n_ids": n, "max_id_count": top, "fwd_bytes": nbytes}
                    for name in fns:
                        rec[name + "_us"] = round(med[name], 1)
                        rec[name + "_minmax_us"] = [round(min(t[name]), 1), round(max(t[name]), 1)]
                    rec["fwd_TBps"] = round(nbytes / med["ours_fwd"] / 1e6, 2)
                    rec["fwd_max_abs_diff_vs_torch"] = diff
                    rec["grad_max_abs_diff_vs_torch"] = gdiff
                    lines.append(json.dumps(rec))
                    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
