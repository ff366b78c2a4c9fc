"""Timing of the sparse table gradient of the pooled lookup (``pool_rows(sparse=True)``:
ncf_bag_pool_bwd with NCF_BAG_COMPACT) and of ``ncf_amd.SparseAdam``, beside the dense path as it
stands and beside torch's own sparse path (GPU only).

    python tools/bag_sparse_bench.py [--rounds 7] [--reps 10] [--out profiles/bag_sparse_bench.json]

Shapes, those of README's pooled-bags line: a 1M x 64 table; 20,480 and 4,096 bags of 50 uniform
ids, and 20,480 ragged bags of 0..50 ids drawn Zipf(1.05).  All legs of a shape run in one
process: after a warm-up of every leg, ``rounds`` rounds run the legs one after another, ``reps``
calls each, so drift of the part hits every leg alike; a figure is the median over the rounds and
``minmax`` the spread of identical legs (us per call).

  bwd_*     the backward alone: the forward runs outside the device events, which bracket
            ``out.backward(gout)`` of every rep and are read after the last one.  ``bwd_dense``:
            the dense path; ``bwd_sparse``: the compact one, its host read of the unique count
            included; ``bwd_torch_sparse``: ``F.embedding_bag(sparse=True)``.
  step_*    whole training steps, forward + backward + optimizer, events around the ``reps``
            steps: dense + torch.optim.Adam; sparse=True + torch.optim.SparseAdam; sparse=True +
            ncf_amd.SparseAdam; nn.EmbeddingBag(sparse=True) + torch.optim.SparseAdam.
  rows_*    the compact backward on a 100K-row and on a 1M-row table with the same ids (all below
            100K): what the table's height still costs (the id sort takes one pass per 11 bits of
            ``rows``: 2 passes both times here).

Prints one JSON line per shape and writes them to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd.sparse import pool_rows  # noqa: E402

DEV = torch.device("cuda")
D = 64
HISTORY = 50
ROWS = 1_000_000
SMALL = 100_000
SHAPES = ((20480, False), (4096, False), (20480, True))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3   # us


def timed_backward(table, forward, gout, reps):
    """us per ``forward().backward(gout)`` into an empty ``table.grad``, the forward outside the
    events."""
    pairs = []
    for _ in range(reps):
        table.grad = None
        out = forward()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out.backward(gout)
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / reps * 1e3


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "bag_sparse_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bag_sparse_bench: no GPU (a timing needs the MI355X)")
    g = torch.Generator().manual_seed(ROWS)
    init = torch.randn(ROWS, D, generator=g).to(DEV)

    def leaf(rows=ROWS):
        return init[:rows].clone().requires_grad_(True)

    lines = []
    for bags, ragged in SHAPES:
        gout = torch.randn(bags, D, generator=g).to(DEV)
        ids, off = make_ids(ROWS, bags, ragged, seed=ROWS + bags)
        ids_small = ids % SMALL
        legs = {}

        # ---- the backward alone
        t_b = leaf()

        def bwd(sparse_flag):
            def forward():
                return pool_rows(t_b, ids, off, None, "sum", check=False, sparse=sparse_flag)
            return lambda reps: timed_backward(t_b, forward, gout, reps)

        def bwd_torch(reps):
            def forward():
                return torch.nn.functional.embedding_bag(ids, t_b, off, mode="sum", sparse=True,
                                                         include_last_offset=True)
            return timed_backward(t_b, forward, gout, reps)

        legs["bwd_dense"], legs["bwd_sparse"] = bwd(False), bwd(True)
        legs["bwd_torch_sparse"] = bwd_torch

        # ---- whole steps
        def stepper(table, opt, forward):
            def one():
                opt.zero_grad(set_to_none=True)
                forward(table).backward(gout)
                opt.step()
            return lambda reps: timed(one, reps)

        def ours(sparse_flag):
            return lambda t: pool_rows(t, ids, off, None, "sum", check=False, sparse=sparse_flag)

        t1, t2, t3 = leaf(), leaf(), leaf()
        legs["step_dense_torch_adam"] = stepper(t1, torch.optim.Adam([t1], lr=1e-3), ours(False))
        legs["step_sparse_torch_sparse_adam"] = stepper(
            t2, torch.optim.SparseAdam([t2], lr=1e-3), ours(True))
        legs["step_sparse_ncf_sparse_adam"] = stepper(t3, ncf.SparseAdam([t3], lr=1e-3), ours(True))
        eb = torch.nn.EmbeddingBag(ROWS, D, mode="sum", sparse=True, include_last_offset=True,
                                   _weight=init.clone()).to(DEV)
        legs["step_torch_bag_torch_sparse_adam"] = stepper(
            eb.weight, torch.optim.SparseAdam([eb.weight], lr=1e-3), lambda t: eb(ids, off))

        # ---- the table's height: the same ids on 100K and 1M rows
        for name, rows in (("rows_100k_bwd_sparse", SMALL), ("rows_1m_bwd_sparse", ROWS)):
            def rows_leg(reps, t=leaf(rows)):
                def forward():
                    return pool_rows(t, ids_small, off, None, "sum", check=False, sparse=True)
                return timed_backward(t, forward, gout, reps)
            legs[name] = rows_leg

        for fn in legs.values():          # warm-up: every leg, allocator and step tables included
            fn(3)
        t = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, fn in legs.items():
                t[name].append(fn(args.reps))
        rec = {"rows": ROWS, "dim": D, "bags": bags,
               "lengths": "0..50 zipf(1.05)" if ragged else "50", "n_ids": ids.numel(),
               "unique_ids": int(torch.unique(ids).numel()),
               "unique_ids_mod_100k": int(torch.unique(ids_small).numel()),
               "max_id_count": int(torch.bincount(ids).max()), "rounds": args.rounds,
               "reps": args.reps}
        for name, v in t.items():
            rec[name + "_us"] = round(statistics.median(v), 1)
            rec[name + "_minmax_us"] = [round(min(v), 1), round(max(v), 1)]
        # the two sparse steps took the same gradients: how far apart the tables ended
        rec["ncf_vs_torch_sparse_adam_max_abs_diff"] = float(
            (t3.detach() - t2.detach()).abs().max())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del legs, t1, t2, t3, eb, t_b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
