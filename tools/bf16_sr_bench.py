"""What stochastic rounding of the bf16 tables costs at C2 (1M x 100K tables, D = 64, 4096 groups
x 5 rows; GPU only).

    python tools/bf16_sr_bench.py [--rounds 7] [--reps 64] [--variants fp32,nearest,stochastic]
                                  [--no-sweep] [--out profiles/bf16_sr_bench.json]

1. ``fused_step_ms``: FusedTrainStep on twin models, one per variant (fp32 tables; bf16 tables
   rounded to nearest even; bf16 tables rounded stochastically), each told its next batch,
   primed 2 x the rolling sweep's period so that every replay has its steady length, then
   alternated in one process: device events around ``reps`` steps, median of ``rounds``.
2. ``sweep_us``: ncf_adam_pairs_sweep_rolling alone on synthetic tables of the same size, one
   set per param_dtype (0, 1, 2), every row 128 steps behind: each call closes one more step
   (ncf_step_clock_advance between calls, timed alone as ``advance_us`` and subtracted), so every
   call replays 128 steps on 1/128 of the rows, as the step's sweep does in steady state.
   ``elem_steps``: replayed element-steps per call; ``ps_per_elem_step``: time over them.
``--variants`` without ``stochastic`` (and ``--no-sweep``) is what an A/B against a library
built from other sources runs (NCF_HIP_LIB), whose kernels may not know param_dtype 2.
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402
from ncf_amd import trainer as Tr  # noqa: E402

DEV = torch.device("cuda")
U, I, D, T, HID, H, B, M = 1_000_000, 100_000, 64, 32, [256, 128, 64], 4, 4096, 5
HP = (0.9, 0.999, 1e-8, 1e-5)
EVERY = Tr.SWEEP_EVERY
VARIANTS = {"fp32": dict(), "nearest": dict(table_dtype=torch.bfloat16),
            "stochastic": dict(table_dtype=torch.bfloat16, table_rounding="stochastic",
                               rounding_seed=1)}


def make_batches(count, seed):
    """Users uniform, the positive item Zipf(1.05), negatives uniform (bench.py's batches)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    w = 1.0 / torch.arange(1, I + 1, dtype=torch.float64) ** 1.05
    cdf = torch.cumsum(w / w.sum(), 0).to(DEV)
    perm = torch.randperm(I, generator=torch.Generator().manual_seed(7)).to(DEV)
    out = []
    for _ in range(count):
        users = torch.randint(0, U, (B,), generator=gen, device=DEV).repeat_interleave(M)
        r = torch.rand(B, generator=gen, device=DEV, dtype=torch.float64)
        pos = perm[torch.searchsorted(cdf, r).clamp_max(I - 1)]
        neg = torch.randint(0, I, (B, M - 1), generator=gen, device=DEV)
        items = torch.cat([pos[:, None], neg], 1).reshape(-1).contiguous()
        t = torch.zeros(B, M, device=DEV)
        t[:, 0] = 1
        out.append((users.contiguous(), items, t.reshape(-1, 1)))
    return out


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps      # ms


def stats(xs, scale=1.0, nd=4):
    return {"median": round(statistics.median(xs) * scale, nd),
            "minmax": [round(min(xs) * scale, nd), round(max(xs) * scale, nd)]}


def fused_steps(variants, rounds, reps):
    batches = make_batches(256, 1)
    steps, pos = {}, {}
    for k in variants:
        torch.manual_seed(0)
        m = ncf.AdvancedNCF(U, I, 5, 24, D, D, T, HID, H, 0.2, M - 1).to(DEV).train()
        steps[k] = Tr.FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, **VARIANTS[k])
        pos[k] = 0

    def step(k):
        s = pos[k]
        pos[k] += 1
        u, i, t = batches[s % len(batches)]
        steps[k](u, i, t, next=batches[(s + 1) % len(batches)][:2])
    for k in steps:
        timed(lambda: step(k), 2 * EVERY + 16)
    ts = {k: [] for k in steps}
    for _ in range(rounds):
        for k in steps:
            ts[k].append(timed(lambda: step(k), reps))
    out = {k: stats(v) for k, v in ts.items()}
    if "nearest" in ts and "stochastic" in ts:
        out["stochastic_adds"] = round(statistics.median(ts["stochastic"]) -
                                       statistics.median(ts["nearest"]), 4)
    return out


class SweepSet:
    """Synthetic C2 tables of one param_dtype, their pairs, a clock at T0 and every stamp
    EVERY steps behind it."""
    T0 = 1000

    def __init__(self, dtype, table):
        g = torch.Generator(device=DEV).manual_seed(3)
        self.keep = []
        self.pairs = (_lib.TablePair * 2)()
        for pr, rows in zip(self.pairs, (U, I)):
            ptrs = []
            for _ in range(2):
                p = torch.randn(rows, D, generator=g, device=DEV) * 0.1
                if dtype != _lib.DTYPE_F32:
                    p = p.to(torch.bfloat16)
                m = torch.randn(rows, D, generator=g, device=DEV) * 1e-3
                v = torch.rand(rows, D, generator=g, device=DEV) * 1e-5
                self.keep += [p, m, v]
                ptrs += [p.data_ptr(), m.data_ptr(), v.data_ptr()]
            pr.p0, pr.m0, pr.v0, pr.p1, pr.m1, pr.v1 = ptrs
            stamp = torch.full((rows,), self.T0 - EVERY, dtype=torch.int32, device=DEV)
            self.keep.append(stamp)
            pr.stamp, pr.rows, pr.param_dtype, pr.round_seed = stamp.data_ptr(), rows, dtype, 1
        self.clock = torch.tensor([self.T0, 1], dtype=torch.int64, device=DEV)
        self.table = table
        self.st = _lib.stream_ptr(DEV)

    def advance(self):
        _lib.call("ncf_step_clock_advance", self.clock.data_ptr(), 1, self.st)

    def call(self):
        self.advance()
        _lib.call("ncf_adam_pairs_sweep_rolling", ctypes.addressof(self.pairs), 2, D, EVERY, 0,
                  self.clock.data_ptr(), self.table.data_ptr(), *HP, self.st)


def sweeps(variants, rounds):
    steps = SweepSet.T0 + EVERY * (rounds + 3) + 4096
    host = np.zeros(4 * (steps + 1), dtype=np.float32)
    _lib.call("ncf_adam_step_scalars", 1e-3, HP[0], HP[1], HP[2], 1, steps, host[4:].ctypes.data)
    table = torch.from_numpy(host).to(DEV)
    dt = {"fp32": _lib.DTYPE_F32, "nearest": _lib.DTYPE_BF16, "stochastic": _lib.DTYPE_BF16_SR}
    sets = {k: SweepSet(dt[k], table) for k in variants}
    for s in sets.values():
        timed(s.call, EVERY)             # one pass: every slice once, the rows EVERY behind again
    adv = [timed(next(iter(sets.values())).advance, EVERY) * 1e3 for _ in range(3)]
    for s in sets.values():              # (the advances alone moved that set's clock 3 passes on)
        s.clock[0] = SweepSet.T0 + EVERY
    ts = {k: [] for k in sets}
    for _ in range(rounds):
        for k, s in sets.items():
            ts[k].append(timed(s.call, EVERY) * 1e3)      # us per call, one pass per window
    a = statistics.median(adv)
    slice_rows = sum((r + EVERY - 1) // EVERY for r in (U, I))
    elem_steps = slice_rows * 2 * D * EVERY
    out = {"advance_us": round(a, 2), "elem_steps": elem_steps}
    for k, v in ts.items():
        net = statistics.median(v) - a
        out[k] = dict(stats(v, nd=2), net_us=round(net, 2),
                      ps_per_elem_step=round(net * 1e6 / elem_steps, 3))
    if "nearest" in ts and "stochastic" in ts:
        out["stochastic_over_nearest"] = round(out["stochastic"]["net_us"] /
                                               out["nearest"]["net_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--variants", default="fp32,nearest,stochastic")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bf16_sr_bench: no GPU (a timing needs the MI355X)")
    variants = [v for v in args.variants.split(",") if v]
    if set(variants) - set(VARIANTS):
        sys.exit(f"bf16_sr_bench: variants are {', '.join(VARIANTS)}")
    rec = {"users": U, "items": I, "dim": D, "groups": B, "rows": B * M, "rounds": args.rounds,
           "reps": args.reps, "sweep_every": EVERY, "lib": os.path.basename(os.path.dirname(
               os.path.abspath(_lib.LIB_PATH))) + "/" + os.path.basename(_lib.LIB_PATH)}
    rec["fused_step_ms"] = fused_steps(variants, args.rounds, args.reps)
    torch.cuda.empty_cache()
    if not args.no_sweep:
        rec["sweep_us"] = sweeps(variants, args.rounds)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
