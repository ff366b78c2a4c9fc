"""What global gradient-norm clipping costs at C2 (1M x 100K tables, D = 64, 4096 groups x 5 rows;
DESIGN §20; GPU only).

    python tools/clip_bench.py [--rounds 9] [--reps 20] [--out FILE]

1. ``kernels``: ncf_grad_clip alone over the compact table gradients and the flat buffer of one
   backward (device events around ``reps`` calls, median of ``rounds``): the norm only
   (max_norm = +inf: launch 1 reads every valid element, launch 2 is one workgroup), a clip that
   does not bite (launch 2 reads the partials in every workgroup and stores nothing) and one that
   bites (launch 2 reads and writes every valid element).  ``bytes`` is what the algorithm moves
   (valid elements x 4 B, once / once / three times; the partials are noise), ``floor_us`` that
   over the guide's measured copy rate (6.29 TB/s), ``x_floor`` the time over the floor.  The
   gradients fit the Infinity Cache, so launch 2's re-read need not come from HBM.
2. ``reference_step``: ``model(kjt) -> BCELoss -> zero_grad -> backward -> [clip_grad_norm_] ->
   Adam.step`` through the fused hook, with and without the clip, alternated on one model and
   optimizer (ms per step; launch tapes on, as a user runs it).  ``clipped`` passes
   ``model.parameters()`` as the reference does, ``clipped_module`` the model itself (its
   parameter list is then kept between calls: the module walk is host time on a host-bound step).
3. ``fused_step``: FusedTrainStep(max_grad_norm=None) against FusedTrainStep(max_grad_norm=...)
   on twin models, alternated, each told its next batch: the clipped step gives up the apply
   fused into the embedding backward and the late catch-up, beside the two clip launches.
Prints one JSON line."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _ncf_pkg  # noqa: E402

ncf = _ncf_pkg.load()
from ncf_amd import _lib, clip  # noqa: E402
from ncf_amd.trainer import FusedTrainStep  # noqa: E402

DEV = torch.device("cuda")
U, I, D, T, HID, H, B, M = 1_000_000, 100_000, 64, 32, [256, 128, 64], 4, 4096, 5
COPY_RATE = 6.29e12      # B/s, the measured streaming copy rate of the MI355X


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


def model():
    torch.manual_seed(0)
    return ncf.AdvancedNCF(U, I, 5, 24, D, D, T, HID, H, 0.2, M - 1).to(DEV).train()


def kjt(u, i):
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([u, i]),
        lengths=torch.ones(2 * u.numel(), dtype=torch.long, device=DEV))


def stats(xs, scale=1.0, nd=4):
    return {"median": round(statistics.median(xs) * scale, nd),
            "minmax": [round(min(xs) * scale, nd), round(max(xs) * scale, nd)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_bench: no GPU (a timing needs the MI355X)")
    batches = make_batches(8, 1)
    crit = torch.nn.BCELoss()
    rec = {"users": U, "items": I, "dim": D, "groups": B, "rows": B * M, "rounds": args.rounds,
           "reps": args.reps, "chunk": _lib.query("ncf_grad_clip_chunk"), "copy_rate_TBps": 6.29}

    # ---- 1. the two launches alone
    m = model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    u, i, t = batches[0]
    crit(m(kjt(u, i)), t).backward()
    eng = m.engine
    w = eng.pending
    segs = clip.table_segments(w) + [(eng.flat_grad, None, 1, eng.flat_grad.numel())]
    nu, ni = w.num_unique.tolist()
    valid = 2 * (nu + ni) * D + eng.flat_grad.numel()
    capacity = sum(r * d for _, _, r, d in segs)
    norm0 = float(ncf.grad_norm(m.parameters()))
    rec.update(unique_users=nu, unique_items=ni, valid_floats=valid, capacity_floats=capacity,
               workgroups=_lib.query("ncf_grad_clip_workspace",
                                     ctypes.addressof(clip.seg_array(segs)), len(segs)) // 8,
               first_norm=round(norm0, 6))
    cases = {"norm_only": (math.inf, 1), "no_bite": (1e30, 1), "bites": (norm0 / 2, 3)}
    kern = {}
    for name, (mx, passes) in cases.items():
        def fn(mx=mx):
            clip.run(segs, 0, mx, DEV)
        timed(fn, 5)
        ts = [timed(fn, 50) * 1e3 for _ in range(args.rounds)]      # us
        byts = 4 * valid * passes
        floor = byts / COPY_RATE * 1e6
        kern[name] = dict(stats(ts, nd=2), bytes=byts, floor_us=round(floor, 2),
                          x_floor=round(statistics.median(ts) / floor, 2))
    rec["kernels_us"] = kern

    # ---- 2. the reference call pattern, with and without the clip (one model, alternated)
    state = {"s": 0}

    def ref_step(clipped):
        u_, i_, t_ = batches[state["s"] % len(batches)]
        state["s"] += 1
        loss = crit(m(kjt(u_, i_)), t_)
        opt.zero_grad()
        loss.backward()
        if clipped:       # (1e-3 always bites; "module": the model itself instead of its parameters())
            ncf.clip_grad_norm_(m if clipped == "module" else m.parameters(), 1e-3)
        opt.step()
    opt.zero_grad()
    fns = {"plain": lambda: ref_step(False), "clipped": lambda: ref_step(True),
           "clipped_module": lambda: ref_step("module")}
    for fn in fns.values():
        timed(fn, 8)
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, args.reps))
    rec["reference_step_ms"] = {k: stats(v) for k, v in ts.items()}
    for k in ("clipped", "clipped_module"):
        rec["reference_step_ms"][k + "_adds"] = round(
            statistics.median(ts[k]) - statistics.median(ts["plain"]), 4)
    rec["reference_tape_replays"] = m.engine.tapes.replays
    del m, opt, eng, w, segs
    torch.cuda.empty_cache()

    # ---- 3. FusedTrainStep with and without max_grad_norm (twin models, alternated)
    steps, pos = {}, {}
    for k, mx in (("plain", None), ("clipped", 1e-3)):
        steps[k] = FusedTrainStep(model(), lr=1e-3, weight_decay=1e-5, max_grad_norm=mx)
        pos[k] = 0

    def fused(k):
        s = pos[k]
        pos[k] += 1
        u_, i_, t_ = batches[s % len(batches)]
        steps[k](u_, i_, t_, next=batches[(s + 1) % len(batches)][:2])
    for k in steps:
        timed(lambda: fused(k), 16)
    ts = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k in steps:
            ts[k].append(timed(lambda: fused(k), args.reps))
    rec["fused_step_ms"] = {k: stats(v) for k, v in ts.items()}
    rec["fused_step_ms"]["clip_adds"] = round(
        statistics.median(ts["clipped"]) - statistics.median(ts["plain"]), 4)
    rec["fused_last_grad_norm"] = round(float(steps["clipped"].last_grad_norm), 6)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
