"""Timing of the forward_simple(hour) training step (``model.hour_backward = True``)
beside the plain ``forward_simple(hour=None)`` training step, and of ``ncf_hour_grad`` beside the
existing ``ncf_temporal_bwd`` (GPU only).

    python tools/hour_train_bench.py [--n 4096,20480] [--rounds 9] [--reps 20] [--out FILE]

Model: the demo's widths (D = 64, T = 32, [256, 128, 64], 4 heads, dropout 0.2) over 1M x 100K
tables, ``torch.optim.Adam(lr=1e-3, weight_decay=1e-5)`` through the fused hook; the projection
pinned (``ops.forward_simple_hour(projection=(w, b))``).  Users uniform, items Zipf(1.05), hours
uniform over 0..23.  Per ``n``, after a warm-up of both, ``rounds`` rounds alternate ``reps`` eager
hour steps (forward + BCE + backward + ``Adam.step``) with ``reps`` plain steps on the same model
and optimizer, each block timed with device events and closed by a synchronise; the figures are
medians over the rounds (ms per step), with the rounds' min and max.  The plain step runs as it
does without this feature: from its launch tapes once they are recorded (``tape_replays`` counts
them; an hour step is eager in every phase and makes the next plain backward record anew).
``kernels_us`` is one instrumented hour step and one instrumented plain step (``_lib.PROFILE``:
device events around each C-ABI call, eager on both sides, a run of their own after the timing):
the per-entry-point sums show where the hour step's extra time sits; what torch itself launches
(BCE, ``hour_embed``'s Adam, gradient bookkeeping) is not in it.
``hour_grad_us`` / ``temporal_bwd_us``: the two reductions alone on the same contiguous dte
[n, T]; ``ncf_temporal_bwd`` has no hour-only call, so its figure covers its three tables (hour,
day, month: 24 + 7 + 12 rows), ``temporal_bwd_hour_share_us`` scales it by 24 / 43.
Prints one JSON line per ``n``."""
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
from ncf_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda")
U, I, D, T, HID, H = 1_000_000, 100_000, 64, 32, [256, 128, 64], 4


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps      # ms


def profile_step(fn):
    """{entry point: summed us} of one call of fn (device events around each C-ABI call)."""
    fn()
    torch.cuda.synchronize()
    _lib.PROFILE = []
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        for name, _, a, b in _lib.PROFILE:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e3
    finally:
        _lib.PROFILE = None
    return {k: round(v, 1) for k, v in sorted(out.items(), key=lambda kv: -kv[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,20480")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hour_train_bench: no GPU (a timing needs the MI355X)")
    torch.manual_seed(0)
    m = ncf.AdvancedNCF(U, I, 5, 24, D, D, T, HID, H, 0.2, 4).to(DEV).train()
    m.hour_backward = True
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    proj = (torch.randn(D, T, generator=g).mul_(0.1).to(DEV), torch.zeros(D, device=DEV))
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        rng = np.random.RandomState(n)
        u = torch.from_numpy(rng.randint(0, U, size=n)).to(DEV)
        p = torch.from_numpy(((rng.zipf(1.05, size=n) - 1) % I).astype(np.int64)).to(DEV)
        h = torch.from_numpy(rng.randint(0, 24, size=n)).to(DEV)
        t = torch.from_numpy((rng.rand(n) < 0.3).astype(np.float32)).to(DEV)

        def hour_step():
            out = ops.forward_simple_hour(m, u, p, h, projection=proj)
            loss = torch.nn.functional.binary_cross_entropy(out, t)
            opt.zero_grad()
            loss.backward()
            opt.step()

        def plain_step():
            loss = torch.nn.functional.binary_cross_entropy(m.forward_simple(u, p), t)
            opt.zero_grad()
            loss.backward()
            opt.step()

        fns = {"hour_step": hour_step, "plain_step": plain_step}
        for fn in fns.values():
            timed(fn, 6)
        r0 = m.engine.tapes.replays
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn, args.reps))
        replays = m.engine.tapes.replays - r0
        # the two reductions alone, on the same dte
        dte = torch.randn(n, T, device=DEV)
        zero = torch.zeros(n, dtype=torch.int64, device=DEV)
        ws = torch.empty(max(1, _lib.query("ncf_hour_grad_workspace", n, T)), device=DEV)
        g_new = torch.empty(24, T, device=DEV)
        g_old, g_day, g_mon = (torch.empty(r, T, device=DEV) for r in (24, 7, 12))
        st = _lib.stream_ptr(DEV)

        def new():
            _lib.call("ncf_hour_grad", h.data_ptr(), n, dte.data_ptr(), T, None, 0, T,
                      g_new.data_ptr(), ws.data_ptr(), ws.numel(), st)

        def old():
            _lib.call("ncf_temporal_bwd", h.data_ptr(), zero.data_ptr(), zero.data_ptr(), n,
                      dte.data_ptr(), T, g_old.data_ptr(), g_day.data_ptr(), g_mon.data_ptr(), st)
        kt = {"new": [], "old": []}
        for fn in (new, old):
            timed(fn, 5)
        for _ in range(args.rounds):
            kt["new"].append(timed(new, 50) * 1e3)
            kt["old"].append(timed(old, 50) * 1e3)
        ref = torch.zeros(24, T, dtype=torch.float64, device=DEV).index_add_(0, h, dte.double())
        rec = {"n": n, "users": U, "items": I, "dim": D, "temporal_dim": T, "hidden": HID,
               "dropout": 0.2, "rounds": args.rounds, "reps": args.reps,
               "hour_grad_chunk": ops.HOUR_GRAD_CHUNK, "plain_tape_replays": replays}
        for k in fns:
            rec[k + "_ms"] = round(statistics.median(ts[k]), 4)
            rec[k + "_minmax_ms"] = [round(min(ts[k]), 4), round(max(ts[k]), 4)]
        rec["hour_over_plain"] = round(rec["hour_step_ms"] / rec["plain_step_ms"], 3)
        rec["hour_grad_us"] = round(statistics.median(kt["new"]), 2)
        rec["hour_grad_minmax_us"] = [round(min(kt["new"]), 2), round(max(kt["new"]), 2)]
        rec["temporal_bwd_us"] = round(statistics.median(kt["old"]), 2)
        rec["temporal_bwd_minmax_us"] = [round(min(kt["old"]), 2), round(max(kt["old"]), 2)]
        rec["temporal_bwd_hour_share_us"] = round(rec["temporal_bwd_us"] * 24 / 43, 2)
        rec["hour_grad_max_abs_err_vs_f64"] = float((g_new.double() - ref).abs().max())
        rec["temporal_bwd_max_abs_err_vs_f64"] = float((g_old.double() - ref).abs().max())
        rec["kernels_us"] = {"hour_step": profile_step(hour_step),
                             "plain_step": profile_step(plain_step)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
