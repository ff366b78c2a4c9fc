"""C5 scoring micro-benchmark (GPU only): 10K users x 1M items top-K through ncf_amd.scoring.

    python tools/score_bench.py [--users 10000] [--items 1000000] [--k 10 100] [--graph]
        [--seen N [--seen-top T]] [--hour H|mixed] [--set scoring.CONST=value ...]
Prints per-stage device times and pairs/s (eager), and with --graph the GraphedScorer time (the
bench's C5 line).  --set overrides ncf_amd module constants before anything runs (A/B).
--seen N: every line once more with ``exclude=``: N random seen items per queried user (about a
tenth of the users none; N no multiple of the 64-lane wave, so the lists end inside one), and the
share of users the select flagged for the exact re-run.  --seen-top T adds each such user's own
best T items to its list (a trained model's history: the re-run's worst case).
--hour H: every line once more at that hour of day (``hour=H``, a fixed random projection on the
index), the graphed lines of a k measured in alternated rounds with their median, and the time to
build one hour's item bias; --hour mixed: a uniform random hour per user instead (eager only: up
to 24 grouped runs)."""
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
    ap.add_argument("--hour", default=None, help="an hour in [0, 24), or 'mixed'")
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
    # (the hour path of a T != D model needs one fixed projection; hour=None never reads it)
    proj = torch.nn.Linear(m.temporal_dim, m.mf_embedding_dim, device=dev) \
        if a.hour is not None and m.temporal_dim != m.mf_embedding_dim else None
    t0 = time.perf_counter()
    idx = ItemIndex(m, projection=proj)
    torch.cuda.synchronize()
    print(f"item index ({a.items} items): {(time.perf_counter() - t0) * 1e3:.2f} ms", flush=True)
    for _ in range(2):   # a rebuild after a parameter change (warm caches and workspaces)
        _lib.PROFILE = []
        t0 = time.perf_counter()
        idx = ItemIndex(m, projection=proj)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prof, _lib.PROFILE = _lib.PROFILE, None
        per = {}
        for name, _, e0, e1 in prof:
            per[name] = per.get(name, 0.0) + e0.elapsed_time(e1)
        print(f"item index rebuild: {dt * 1e3:.2f} ms  "
              + " ".join(f"{n}={v:.2f}ms" for n, v in per.items()), flush=True)
    users = torch.randperm(a.num_users, device=dev)[:a.users]
    variants = [("", None, None)]
    if a.hour is not None:
        if a.hour == "mixed":
            hour = torch.randint(0, 24, (a.users,), device=dev)
        else:
            hour = int(a.hour)
        idx.hour_table()
        torch.cuda.synchronize()
        for h in (1, 2, 3):   # (the first one warms the workspaces)
            t0 = time.perf_counter()
            idx.hour_bias(h)
            torch.cuda.synchronize()
            print(f"hour bias build (hour {h}): {(time.perf_counter() - t0) * 1e3:.2f} ms",
                  flush=True)
        variants.append((f" hour={a.hour}", None, hour))
    if a.seen:
        seen = make_seen(m, users, idx, a.seen, a.seen_top, a.num_users, a.items)
        print(f"seen: {seen.items.numel()} items over {int((seen.lengths > 0).sum())} of "
              f"{a.users} users, longest {int(seen.lengths.max())}", flush=True)
        variants.append((f" seen={a.seen}+top{a.seen_top}", seen, None))
        if a.hour is not None:
            variants.append((f" hour={a.hour} seen={a.seen}+top{a.seen_top}", seen, hour))
    for k in a.k:
        scorers = []
        for tag, ex, hr in variants:
            score_topk(m, users, k, idx, exclude=ex, hour=hr)
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(a.reps):
                _lib.PROFILE = []
                t0 = time.perf_counter()
                s, it = score_topk(m, users, k, idx, exclude=ex, hour=hr)
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
            if ex is not None and hr is None:
                print(f"k={k}{tag}: {100 * rerun_share(m, users, k, idx, ex):.2f}% of the users "
                      "re-run", flush=True)
            if a.graph and not isinstance(hr, torch.Tensor):
                sc = GraphedScorer(m, n_users=a.users, k=k, index=idx, exclude=ex, hour=hr)
                sc(users, copy=False)
                torch.cuda.synchronize()
                g = 1e9
                for _ in range(max(3, a.reps)):
                    t0 = time.perf_counter()
                    sc(users, copy=False)
                    torch.cuda.synchronize()
                    g = min(g, time.perf_counter() - t0)
                print(f"k={k}{tag}: graphed {g * 1e3:.3f} ms", flush=True)
                if a.hour is not None:
                    scorers.append((tag, sc, hr))
                del sc
        if len(scorers) > 1:
            # A/B in one process: the scorers of this k replayed in alternated rounds (each
            # round: the mean of 10 replays), the median round per scorer; an hour scorer also
            # switching between two hours on every replay (the in-place bias copies)
            rounds = {tag: [] for tag, _, _ in scorers}
            switch = {tag: [] for tag, _, hr in scorers if hr is not None}
            for _ in range(max(3, a.reps)):
                for tag, sc, hr in scorers:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _i in range(10):
                        sc(users, copy=False)
                    torch.cuda.synchronize()
                    rounds[tag].append((time.perf_counter() - t0) / 10)
                    if hr is not None:
                        t0 = time.perf_counter()
                        for i in range(10):
                            sc(users, copy=False, hour=(hr + 1 + i % 2) % 24)
                        torch.cuda.synchronize()
                        switch[tag].append((time.perf_counter() - t0) / 10)
                        sc(users, copy=False, hour=hr)
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            for tag, _, _ in scorers:
                print(f"k={k}{tag}: graphed, alternated rounds "
                      + " ".join(f"{x * 1e3:.3f}" for x in rounds[tag])
                      + f" ms, median {med(rounds[tag]) * 1e3:.3f} ms"
                      + (f"; another hour every call: median {med(switch[tag]) * 1e3:.3f} ms"
                         if tag in switch else ""), flush=True)
        del scorers

if __name__ == "__main__":
    main()
