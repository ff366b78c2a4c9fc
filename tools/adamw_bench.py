"""What decoupled weight decay (torch.optim.AdamW's rule) costs or saves at C2 (1M x 100K tables,
D = 64, 4096 groups x 5 rows; one GPU).

    python tools/adamw_bench.py [--rounds 5] [--reps 4096] [--out profiles/adamw_bench.json]

1. ``fused_step_ms``: FusedTrainStep on twin models, coupled and decoupled (fp32 tables), each told
   its next batch, primed 2 x the rolling sweep's period so that every replay has its steady
   length, then alternated in one process: device events around ``reps`` steps (more than a
   second per leg at the defaults), median of ``rounds``.  ``coupled_again``: a third twin of the
   coupled build in the same alternation: the spread two legs of the same code show.
2. ``sweep_us``: ncf_adam_pairs_sweep_rolling alone on synthetic tables of the same size in both
   modes, every row 128 steps behind: each call closes one more step (ncf_step_clock_advance
   between calls, timed alone and subtracted), so every call replays 128 steps on 1/128 of the
   rows, as the step's sweep does in steady state.
3. ``dropin_ms``: the reference call pattern (model(kjt) -> BCELoss -> zero_grad -> backward ->
   step) with torch.optim.AdamW on the fused path, and with the same optimizer forced onto the
   fallback (dense table gradients, torch's own loop), wall clock per step with a device
   synchronise at the end.
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402
from ncf_amd import optim as Opt  # noqa: E402
from ncf_amd import trainer as Tr  # noqa: E402
from ncf_amd.deferred import adamw_step_scalars  # noqa: E402

DEV = torch.device("cuda")
U, I, D, T, HID, H, B, M = 1_000_000, 100_000, 64, 32, [256, 128, 64], 4, 4096, 5
HP = (0.9, 0.999, 1e-8, 1e-2)
EVERY = Tr.SWEEP_EVERY
VARIANTS = {"coupled": False, "decoupled": True, "coupled_again": False}


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


def new_model():
    torch.manual_seed(0)
    return ncf.AdvancedNCF(U, I, 5, 24, D, D, T, HID, H, 0.2, M - 1).to(DEV).train()


def fused_steps(rounds, reps, batches):
    steps, pos = {}, {}
    for k, dec in VARIANTS.items():
        steps[k] = Tr.FusedTrainStep(new_model(), lr=1e-3, weight_decay=HP[3],
                                     decoupled_weight_decay=dec)
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
    med = {k: statistics.median(v) for k, v in ts.items()}
    out["decoupled_minus_coupled"] = round(med["decoupled"] - med["coupled"], 4)
    out["same_build_spread"] = round(med["coupled_again"] - med["coupled"], 4)
    return out


def sweep(decoupled, calls=48):
    """ncf_adam_pairs_sweep_rolling on synthetic C2 tables, every row EVERY steps behind."""
    g = torch.Generator(device=DEV).manual_seed(3)
    keep, T0 = [], 1000
    pairs = (_lib.TablePair * 2)()
    for pr, rows in zip(pairs, (U, I)):
        ptrs = []
        for _ in range(2):
            p = torch.randn(rows, D, generator=g, device=DEV) * 0.1
            m = torch.randn(rows, D, generator=g, device=DEV) * 1e-3
            v = torch.rand(rows, D, generator=g, device=DEV) * 1e-4 + 1e-8
            keep += [p, m, v]
            ptrs += [p.data_ptr(), m.data_ptr(), v.data_ptr()]
        stamp = torch.full((rows,), T0 - EVERY, dtype=torch.int32, device=DEV)
        keep.append(stamp)
        pr.p0, pr.m0, pr.v0, pr.p1, pr.m1, pr.v1 = ptrs
        pr.stamp, pr.rows = stamp.data_ptr(), rows
        pr.param_dtype = _lib.DTYPE_F32 | (_lib.ADAM_DECOUPLED if decoupled else 0)
    S = _lib.ADAMW_TABLE_STRIDE if decoupled else 4
    n = T0 + calls + 4200
    import numpy as np
    host = np.zeros(S * (n + 1), np.float32)
    if decoupled:
        adamw_step_scalars(1e-3, *HP, 1, n, host[S:])
    else:
        _lib.call("ncf_adam_step_scalars", 1e-3, *HP[:3], 1, n, host[S:].ctypes.data)
    table = torch.from_numpy(host).to(DEV)
    clock = torch.tensor([T0, 5], dtype=torch.int64, device=DEV)
    st = _lib.stream_ptr(DEV)
    pa = ctypes.addressof(pairs)

    def one():
        _lib.call("ncf_adam_pairs_sweep_rolling", pa, 2, D, EVERY, 1, clock.data_ptr(),
                  table.data_ptr(), *HP, st)
        _lib.call("ncf_step_clock_advance", clock.data_ptr(), 5, st)
    timed(one, 4)
    both = timed(one, calls)
    adv = timed(lambda: _lib.call("ncf_step_clock_advance", clock.data_ptr(), 5, st), calls)
    clock[0] = T0
    elem_steps = EVERY * ((U + EVERY - 1) // EVERY + (I + EVERY - 1) // EVERY) * D * 2
    us = (both - adv) * 1e3
    return {"us_per_launch": round(us, 2), "advance_us": round(adv * 1e3, 2),
            "elem_steps": elem_steps, "ps_per_elem_step": round(us * 1e6 / elem_steps, 4)}


def dropin(fallback, steps, batches):
    """torch.optim.AdamW behind the reference call pattern; ``fallback``: the hook told it is not
    a plain Adam (dense table gradients, torch's loop)."""
    m = new_model()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=HP[3])
    crit = torch.nn.BCELoss()
    plain = Opt._is_plain_adam
    if fallback:
        Opt._is_plain_adam = lambda o: False
    try:
        def one(s):
            u, i, t = batches[s % len(batches)]
            kjt = ncf.KeyedJaggedTensor.from_lengths_sync(
                keys=["user_id", "product_id"], values=torch.cat([u, i]),
                lengths=torch.ones(2 * u.numel(), dtype=torch.long, device=DEV))
            loss = crit(m(kjt), t)
            opt.zero_grad()
            loss.backward()
            opt.step()
        for s in range(8):
            one(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            one(8 + s)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        bound = Opt.binding_of(opt, m) is not None
    finally:
        Opt._is_plain_adam = plain
    return {"ms_per_step": round(ms, 4), "fused_path": bound, "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4096)
    ap.add_argument("--no-dropin", action="store_true")
    ap.add_argument("--out", default="profiles/adamw_bench.json")
    a = ap.parse_args()
    batches = make_batches(256, 1)
    out = {"config": {"U": U, "I": I, "D": D, "groups": B, "M": M, "sweep_every": EVERY,
                      "weight_decay": HP[3], "rounds": a.rounds, "reps": a.reps},
           "fused_step_ms": fused_steps(a.rounds, a.reps, batches)}
    torch.cuda.empty_cache()
    out["sweep_us"] = {"coupled": sweep(False), "decoupled": sweep(True)}
    torch.cuda.empty_cache()
    if not a.no_dropin:
        out["dropin_ms"] = {"fused": dropin(False, 400, batches),
                            "fallback": dropin(True, 30, batches)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
