"""Exact-rank micro-benchmark (GPU only): score_rank against score_topk(exclude=) on one index.

    python tools/rank_bench.py [--users 10000] [--items 1000000] [--seen 50] [--k 10 100]
        [--rounds 7] [--inner 3] [--json profiles/NAME.json]
The workload of DESIGN's scoring sections: 10K users x 1M items, D = 64, ``--seen`` random seen
items per user, one random held-out item per user outside the user's history.  The variants
(score_rank, and score_topk at every ``--k``) run alternated in one process after a warm-up of
each; a round times ``--inner`` back-to-back calls of one variant between two device events and
the figure kept per variant is the median round.  ``stages``: score_rank's launches timed one by
one in a further run (the library's PROFILE instrumentation).  Prints one JSON object; ``--json``
also writes it to a file."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402
from ncf_amd.scoring import ItemIndex, SeenItems, score_rank, score_topk  # noqa: E402


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--num-users", type=int, default=1000000)
    ap.add_argument("--seen", type=int, default=50)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_bench: needs the GPU (no CPU fallback)")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = ncf.AdvancedNCF(a.num_users, a.items, 5, 24).to(dev).eval()
    idx = ItemIndex(m)
    users = torch.randperm(a.num_users, device=dev)[:a.users]
    seen = None
    if a.seen:
        items = torch.randint(0, a.items, (a.users, a.seen), device=dev)
        seen = SeenItems(users.repeat_interleave(a.seen), items.reshape(-1), a.num_users, a.items)
    held = torch.randint(0, a.items, (a.users,), device=dev)
    if seen is not None:   # a held-out item outside the history: redraw the few that are inside
        for _ in range(8):
            inside = seen.contains(users, held)
            if not bool(inside.any()):
                break
            held[inside] = torch.randint(0, a.items, (int(inside.sum()),), device=dev)
    variants = {"score_rank": lambda: score_rank(m, users, held, idx, exclude=seen)}
    for k in a.k:
        variants[f"score_topk@{k}"] = lambda k=k: score_topk(m, users, k, idx, exclude=seen)
    for fn in variants.values():   # warm-up: code objects, workspaces, the allocator's pools
        fn()
        fn()
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            rounds[name].append(timed(fn, a.inner))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    _lib.PROFILE = []
    variants["score_rank"]()
    torch.cuda.synchronize()
    prof, _lib.PROFILE = _lib.PROFILE, None
    stages = {}
    for name, _, e0, e1 in prof:
        stages[name] = round(stages.get(name, 0.0) + e0.elapsed_time(e1), 4)
    place, cand = variants["score_rank"]()
    scan_flop = 2.0 * a.users * a.items * idx.p.shape[1]
    out = {
        "workload": {"users": a.users, "items": a.items, "dim": idx.p.shape[1],
                     "seen_per_user": a.seen, "rounds": a.rounds, "inner": a.inner},
        "median_ms": {name: round(med(v), 4) for name, v in rounds.items()},
        "rounds_ms": {name: [round(x, 4) for x in v] for name, v in rounds.items()},
        "score_rank_stages_ms": stages,
        "scan_tflops": round(scan_flop / (stages.get("ncf_rank_scan", float("nan")) * 1e-3)
                             / 1e12, 2),
        "mean_place": float(place.double().mean()),
        "mean_candidates": float(cand.double().mean()),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
