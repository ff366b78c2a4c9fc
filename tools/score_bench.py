"""C5 scoring micro-benchmark (GPU only): 10K users x 1M items top-K through ncf_amd.scoring.

    python tools/score_bench.py [--users 10000] [--items 1000000] [--k 10 100] [--graph]
        [--seen N [--seen-top T]] [--set scoring.CONST=value ...]
Prints per-stage device times and pairs/s (eager), and with --graph the GraphedScorer time (the
bench's C5 line).  --set overrides ncf_amd module constants before anything runs (A/B).
--seen N: every line once more with ``exclude=``: N random seen items per queried user (about a
tenth of the users none; N no multiple of the 64-lane wave, so the lists end inside one), and the
share of users the select flagged for the exact re-run.  --seen-top T adds each such user's own
best T items to its list (a trained model's history: the re-run's worst case)."""
import importlib
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402
from ncf_amd.scoring import GraphedScorer, ItemIndex, SeenItems, _TopKRun, score_topk  # noqa: E402


def make_seen(m, users, idx, n_seen, n_top, num_users, num_items):
    """N random items (and the best ``n_top``) per queried user, nine users in ten."""
    dev = users.device
    has = torch.rand(users.numel(), device=dev) >= 0.1
    u = users[has]
    items = torch.randint(0, num_items, (u.numel(), n_seen), device=dev)
    if n_top:
        items = torch.cat([items, score_topk(m, u, n_top, idx)[1]], 1)
    return SeenItems(u.repeat_interleave(items.shape[1]), items.reshape(-1), num_users, num_items)


def rerun_share(m, users, k, idx, seen):
    """Share of the users whose first pass the select flagged (overflow or check failed)."""
    run = _TopKRun(idx, users.numel(), k, 8192, exclude=seen)
    run.uid.copy_(users)
    run.launch(m, _lib.stream_ptr(users.device))
    return float((run.overflow[:users.numel()] != 0).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--num-users", type=int, default=1000000)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--seen", type=int, default=0)
    ap.add_argument("--seen-top", type=int, default=0)
    ap.add_argument("--set", nargs="*", default=[])
    a = ap.parse_args()
    if a.seen and a.seen % 64 == 0:
        ap.error("--seen must not be a multiple of the wave size (64)")
    for spec in a.set:
        path, _, val = spec.partition("=")
        mod, _, const = path.rpartition(".")
        mm = importlib.import_module("ncf_amd." + mod)
        old = getattr(mm, const)
        setattr(mm, const, type(old)(int(val)) if isinstance(old, (bool, int)) else type(old)(val))
        print(f"set {path} = {getattr(mm, const)!r}", flush=True)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = ncf.AdvancedNCF(a.num_users, a.items, 5, 24).to(dev)
    m.eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = ItemIndex(m)
    torch.cuda.synchronize()
    print(f"item index ({a.items} items): {(time.perf_counter() - t0) * 1e3:.2f} ms", flush=True)
    for _ in range(2):   # a rebuild after a parameter change (warm caches and workspaces)
        _lib.PROFILE = []
        t0 = time.perf_counter()
        idx = ItemIndex(m)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prof, _lib.PROFILE = _lib.PROFILE, None
        per = {}
        for name, _, e0, e1 in prof:
            per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
        print(f"item index rebuild: {dt * 1e3:.2f} ms  "
              + " ".join(f"{n}={v:.2f}ms" for n, v in per.items()), flush=True)
    users = torch.randperm(a.num_users, device=dev)[:a.users]
    variants = [("", None)]
    if a.seen:
        seen = make_seen(m, users, idx, a.seen, a.seen_top, a.num_users, a.items)
        print(f"seen: {seen.items.numel()} items over {int((seen.lengths > 0).sum())} of "
              f"{a.users} users, longest {int(seen.lengths.max())}", flush=True)
        variants.append((f" seen={a.seen}+top{a.seen_top}", seen))
    for k in a.k:
        for tag, ex in variants:
            score_topk(m, users, k, idx, exclude=ex)
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(a.reps):
                _lib.PROFILE = []
                t0 = time.perf_counter()
                s, it = score_topk(m, users, k, idx, exclude=ex)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                prof, _lib.PROFILE = _lib.PROFILE, None
                best = min(best, dt)
            per = {}
            for name, _, e0, e1 in prof:
                per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
            pairs = a.users * a.items
            print(f"k={k}{tag}: {best * 1e3:.2f} ms  {pairs / best / 1e9:.1f} G pairs/s  "
                  + " ".join(f"{n}={v:.2f}ms" for n, v in per.items()), flush=True)
            if ex is not None:
                print(f"k={k}{tag}: {100 * rerun_share(m, users, k, idx, ex):.2f}% of the users "
                      "re-run", flush=True)
            if a.graph:
                sc = GraphedScorer(m, n_users=a.users, k=k, index=idx, exclude=ex)
                sc(users, copy=False)
                torch.cuda.synchronize()
                g = 1e9
                for _ in range(max(3, a.reps)):
                    t0 = time.perf_counter()
                    sc(users, copy=False)
                    torch.cuda.synchronize()
                    g = min(g, time.perf_counter() - t0)
                print(f"k={k}{tag}: graphed {g * 1e3:.3f} ms", flush=True)
                del sc

if __name__ == "__main__":
    main()
