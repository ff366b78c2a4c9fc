"""Stochastic rounding of the bf16 tables' Adam updates (NCF_DTYPE_BF16_SR) on the
MI355X, against tests/sr_stream.py's restatement of the stream and the store.

1. One step against float64 (``check_adam_sr``): test_gpu_bf16's ``adam_inputs`` through
   ncf_adam_pairs_apply_clock (touched rows) and ncf_adam_pairs_catchup_clock (the others), three
   steps, both tables of both kinds.
2. The stall (``check_stall``): p = 1, gradient +1, lr = 2^-12 = 1/16 of the spacing below 1:
   nearest-even never moves, stochastic rounding moves 4 spacings in 64 steps on average.
3. Replay equals stepping (``schedules``): every way of bringing the same rows to step 140 gives
   the same bits.
4. FusedTrainStep: every schedule of the step gives the same bits; one step against the float64
   oracle.

The check functions take the code under test as a callable, so tests/test_sr_stream_cpu.py runs
them on the CPU stand-in (the fp32 CPU Adam with the restated store) to confirm every expected
value and bound before a GPU sees them, and with nearest-even in the store's place to confirm
that they fail.  Figures of that stand-in (this file's inputs and seeds; ``mix32`` stream):

* check_adam_sr: at most 3 of a table's 64,000 elements (D = 64) and 3 of 128,000 (D = 128)
  differ from the restated decision in a step, within 3.7e-3 / 0.12 bf16 steps of the threshold
  (the latter on elements that cancel to near 0, where fp32 and float64 differ by up to 0.2
  steps); |mean signed error| at most 2.1e-3 / 1.4e-3 steps against 2 / sqrt(n) = 7.9e-3 /
  5.6e-3.
* check_stall: mean displacement 3.979 .. 4.011 spacings over the four tables (bound 4 +-
  0.0856).
* check_step_tables: the fp32 oracle with the restated store agrees on every element.

Runs on a real MI355X only (marker ``gpu``)."""
import ctypes

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import sr_stream as SR
from tests import test_gpu_bf16 as TB

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")
SEED = 0x5EED1234                 # rounding seed of the primitive cases
LOCK = 0x40000000                 # NCF_STAMP_LOCK
NAMES = ("p0", "m0", "v0", "p1", "m1", "v1")


def bf16_bits(t):
    """uint16 numpy bits of a bf16 tensor."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_f32(x):
    """A bf16 tensor holding the fp32 numpy values x (which bf16 holds exactly)."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    out = t.to(torch.bfloat16)
    assert torch.equal(out.float(), t)
    return out


# --------------------------------------------------------------------------- 1. one step
def check_adam_sr(D, apply, seed, report=None):
    """Three steps of ``apply(kind, j, p0, m0, v0, grad, has, t) -> (p bf16, m, v)`` on
    test_gpu_bf16.adam_inputs, each table (kind, j) against the float64 Adam restarted from the
    state ``apply`` left:
    * m, v within rtol 1e-6;
    * the stored p is one of the two bf16 neighbours of the float64 p (the value itself where
      bf16 holds it);
    * it is the neighbour the restated bits choose for the float64 p (up in magnitude iff
      frac + r / 65536 >= 1), except within 4 x the largest |fp32 torch Adam - float64| on
      these inputs of the threshold (as an absolute distance and in bf16 steps, as
      check_adam_bf16 measures it); at most 0.1 % of the elements;
    * |mean signed error| < 2 / sqrt(n) bf16 steps (n elements; the error of a stochastic store
      has at most variance 1/4 per element: 4 standard deviations of the mean)."""
    p_in, slot, touched, G = TB.adam_inputs(D, TB.ADAM_SEED[D])
    grad = torch.zeros(TB.ADAM_ROWS, D)
    grad[touched] = G
    has = np.zeros(TB.ADAM_ROWS, bool)
    has[touched.numpy()] = True
    e = np.arange(TB.ADAM_ROWS * D, dtype=np.uint64).reshape(TB.ADAM_ROWS, D)
    for kind in (0, 1):
        for j in (0, 1):
            p, m, v = p_in.clone(), torch.zeros(TB.ADAM_ROWS, D), torch.zeros(TB.ADAM_ROWS, D)
            for t in (1, 2, 3):
                p0, m0, v0 = p.clone(), m.clone(), v.clone()
                p, m, v = apply(kind, j, p0, m0, v0, grad, has, t)
                assert p.dtype == torch.bfloat16 and m.dtype == torch.float32
                p64, m64, v64 = TB._adam_ref(p0, m0, v0, grad, t, torch.float64)
                p32, _, _ = TB._adam_ref(p0, m0, v0, grad, t, torch.float32)
                torch.testing.assert_close(m.double(), m64, rtol=1e-6, atol=0)
                torch.testing.assert_close(v.double(), v64, rtol=1e-6, atol=0)
                lo, hi, ulp = SR.neighbours(p64.numpy())
                got = p.double().numpy()
                assert bool(((got == lo) | (got == hi)).all()), (kind, j, t)
                frac = (np.abs(p64.numpy()) - np.abs(lo)) / ulp            # in [0, 1)
                r = SR.bits(seed, kind, j, t, e).astype(np.float64) / 65536.0
                want = np.where(frac + r >= 1.0, hi, lo)
                e32 = np.abs(p32.double().numpy() - p64.numpy())
                e_abs, e_steps = e32.max(), (e32 / ulp).max()
                diff = got != want
                nd = int(diff.sum())
                dist = np.abs(frac + r - 1.0)                              # in bf16 steps
                signed = float(((got - p64.numpy()) / ulp).mean())
                if report is not None:
                    report.append((kind, j, t, nd, float(dist[diff].max()) if nd else 0.0, signed))
                assert nd <= 1e-3 * got.size, (kind, j, t, nd)
                assert bool((dist[diff] * ulp[diff] <= 4 * e_abs).all()), (kind, j, t)
                assert bool((dist[diff] <= 4 * e_steps).all()), (kind, j, t)
                assert abs(signed) < 2 / got.size ** 0.5, (kind, j, t, signed)


class Pairs:
    """Two kinds' GMF + MLP tables on the device with their ncf_table_pair array, a clock and a
    step table.  tables[kind]: p0 / p1 (bf16), m0 / v0 / m1 / v1 (fp32), stamp (int32)."""

    def __init__(self, tables, D, dtype, seed, lr_of_step, hp, steps):
        from ncf_amd import _lib
        self.L = _lib
        self.D, self.hp = D, hp
        self.t = [{k: v.to(DEV).contiguous() for k, v in kd.items()} for kd in tables]
        self.pairs = (_lib.TablePair * 2)()
        for pr, kd in zip(self.pairs, self.t):
            for n in NAMES:
                setattr(pr, n, kd[n].data_ptr())
            pr.stamp, pr.rows = kd["stamp"].data_ptr(), kd["stamp"].numel()
            pr.param_dtype = dtype
            pr.round_seed = seed - (1 << 32) * (seed >> 31)
        self.clock = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
        host = np.zeros(4 * (steps + 4096 + 1), dtype=np.float32)
        s = 1
        while s <= steps + 4096:        # (runs of one lr: ncf_adam_step_scalars takes one)
            e = s
            while e + 1 <= steps + 4096 and lr_of_step(e + 1) == lr_of_step(s):
                e += 1
            _lib.call("ncf_adam_step_scalars", lr_of_step(s), hp[0], hp[1], hp[2], s, e - s + 1,
                      host[4 * s:].ctypes.data)
            s = e + 1
        self.table = torch.from_numpy(host).to(DEV)
        self.st = _lib.stream_ptr(DEV)
        self.keep = []

    def at(self, t):
        self.clock[0] = t

    def ids(self, rows, G=None):
        """List rows (a list per kind) as the pairs' unique rows; -> count tensor, max_n."""
        cnt = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
        for pr, r in zip(self.pairs, rows):
            ids = torch.tensor(list(r) + [0], dtype=torch.int64, device=DEV)
            self.keep.append(ids)
            pr.row_ids = ids.data_ptr()
        if G is not None:
            for pr, (g0, g1) in zip(self.pairs, G):
                self.keep += [g0, g1]
                pr.g0, pr.g1 = g0.data_ptr(), g1.data_ptr()
        self.keep.append(cnt)
        return cnt, max(max(len(r) for r in rows), 1)

    def addr(self):
        return ctypes.addressof(self.pairs)

    def catchup(self, rows, rel=0, lock=None, claim=False, fused=False):
        L, a = self.L, (self.clock.data_ptr(), self.table.data_ptr(), *self.hp, self.st)
        if claim:       # raw lists, every row three times, both lists of one length
            n = 3 * max(len(r) for r in rows)
            raw = [torch.tensor((list(r) * 3 + [r[0] if len(r) else 0] * n)[:n], dtype=torch.int64,
                                device=DEV) if len(r) else None for r in rows]
            assert all(x is not None for x in raw)
            self.keep += raw
            L.call("ncf_adam_pairs_catchup_claim_clock", self.addr(), 2, self.D,
                   raw[0].data_ptr(), raw[1].data_ptr(), n, rel, *a)
            return
        cnt, mx = self.ids(rows)
        if fused:       # inside the first launch of a (one-descriptor) reduction
            part = torch.ones(5, 64, device=DEV)
            out = torch.zeros(64, device=DEV)
            lst = L.ReduceList()
            d = lst.d[0]
            d.part, d.out, d.stride, d.ldo = part.data_ptr(), out.data_ptr(), 64, 64
            d.L, d.cols, d.P, d.accumulate, d.scale, d.reserved = 64, 64, 5, 0, 1.0, 0
            lst.count = 1
            need = L.query("ncf_reduce_batch_scratch", lst.address)
            scr = torch.zeros(max(need, 1), device=DEV)
            self.keep += [part, out, scr]
            L.call("ncf_reduce_batch_catchup", lst.address, scr.data_ptr(), scr.numel(),
                   self.addr(), 2, self.D, cnt.data_ptr(), mx, rel, *a)
            torch.cuda.synchronize()
            assert float(out.sum()) == 5.0 * 64
        elif lock is None:
            L.call("ncf_adam_pairs_catchup_clock", self.addr(), 2, self.D, cnt.data_ptr(), mx, rel,
                   *a)
        else:
            L.call("ncf_adam_pairs_catchup_lock_clock", self.addr(), 2, self.D, cnt.data_ptr(), mx,
                   rel, lock, *a)

    def apply(self, rows, G, rel=1):
        cnt, mx = self.ids(rows, G)
        self.L.call("ncf_adam_pairs_apply_clock", self.addr(), 2, self.D, cnt.data_ptr(), mx, rel,
                    self.clock.data_ptr(), self.table.data_ptr(), *self.hp, self.st)

    def sweep(self, every, part=None, nparts=1):
        a = (self.clock.data_ptr(), self.table.data_ptr(), *self.hp, self.st)
        if part is None:
            self.L.call("ncf_adam_pairs_sweep_rolling", self.addr(), 2, self.D, every, 0, *a)
        else:
            self.L.call("ncf_adam_pairs_sweep_rolling_part", self.addr(), 2, self.D, every, 0, part,
                        nparts, *a)

    def result(self):
        torch.cuda.synchronize()
        return [{k: v.cpu().clone() for k, v in kd.items()} for kd in self.t]


@pytest.mark.parametrize("D", [64, 128])
def test_one_step_is_a_stochastic_rounding_of_the_float64_result(D):
    """Touched rows through ncf_adam_pairs_apply_clock, the others through
    ncf_adam_pairs_catchup_clock (target_rel 1), param_dtype NCF_DTYPE_BF16_SR."""
    from ncf_amd import _lib
    hp = (*TB.ADAM_HP["betas"], TB.ADAM_HP["eps"], TB.ADAM_HP["wd"])
    _, _, touched, G = TB.adam_inputs(D, TB.ADAM_SEED[D])
    others = sorted(set(range(TB.ADAM_ROWS)) - set(touched.tolist()))
    report = []

    def apply(kind, j, p0, m0, v0, grad, has, t):
        # the table under test sits at (kind, j); the three others hold the same data
        kd = dict(p0=p0, m0=m0, v0=v0, p1=p0.clone(), m1=m0.clone(), v1=v0.clone(),
                  stamp=torch.full((TB.ADAM_ROWS,), t - 1, dtype=torch.int32))
        P = Pairs([kd, {k: v.clone() for k, v in kd.items()}], D, _lib.DTYPE_BF16_SR, SEED,
                  lambda s: TB.ADAM_HP["lr"], hp, 3)
        P.at(t - 1)
        Gd = G.to(DEV)
        P.apply([touched.tolist()] * 2, [(Gd, Gd)] * 2)
        P.catchup([others] * 2, rel=1)
        out = P.result()[kind]
        assert bool((out["stamp"] == t).all())
        return out[f"p{j}"], out[f"m{j}"], out[f"v{j}"]
    try:
        check_adam_sr(D, apply, SEED, report)
    finally:
        for kind, j, t, nd, far, sg in report:
            print(f"adam bf16 SR D={D} kind {kind} table {j} step {t}: {nd} elements differ from "
                  f"the restated decision (at most {far:.3g} steps from the threshold); mean "
                  f"signed error {sg:.3g} steps")


# --------------------------------------------------------------------------- 2. the stall
STALL_ROWS, STALL_D, STALL_STEPS, STALL_LR = 128, 64, 64, 2.0 ** -12
STALL_HP = (0.9, 0.999, 1e-8, 0.0)


def check_stall(run):
    """``run(stochastic) -> [kind][j] fp32 numpy [128, 64]`` after 64 gradient steps from p = 1
    with g = +1, lr = 2^-12, wd = 0 (m-hat / sqrt(v-hat) = 1: every step asks for 1/16 of the
    2^-8 spacing below 1).  Nearest even: nothing ever moves.  Stochastic: each step moves an
    element one spacing with probability 1/16, so after 64 steps the displacement has mean 4 and
    variance 64 * (1/16) * (15/16) = 3.75 per element; the mean over the 8192 elements of a
    table is asserted within 4 sigma = 4 sqrt(3.75 / 8192) = 0.0856 spacings."""
    for tab in (x for kd in run(False) for x in kd):
        assert bool((tab == 1.0).all())
    out = []
    for kind, kd in enumerate(run(True)):
        for j, tab in enumerate(kd):
            disp = (1.0 - tab.astype(np.float64)) * 256.0
            assert bool((disp == np.round(disp)).all()) and bool((disp >= 0).all()), (kind, j)
            mean = float(disp.mean())
            out.append(mean)
            assert abs(mean - 4.0) < 4 * (3.75 / disp.size) ** 0.5, (kind, j, mean)
            assert 2.5 < float(disp.var()) < 5.0, (kind, j, float(disp.var()))
    return out


def test_stochastic_rounding_moves_what_nearest_even_stalls():
    from ncf_amd import _lib

    def run(stochastic):
        kd = dict(stamp=torch.zeros(STALL_ROWS, dtype=torch.int32))
        for j in (0, 1):
            kd[f"p{j}"] = torch.ones(STALL_ROWS, STALL_D, dtype=torch.bfloat16)
            kd[f"m{j}"] = torch.zeros(STALL_ROWS, STALL_D)
            kd[f"v{j}"] = torch.zeros(STALL_ROWS, STALL_D)
        P = Pairs([kd, {k: v.clone() for k, v in kd.items()}], STALL_D,
                  _lib.DTYPE_BF16_SR if stochastic else _lib.DTYPE_BF16, SEED,
                  lambda s: STALL_LR, STALL_HP, STALL_STEPS)
        G = torch.ones(STALL_ROWS, STALL_D, device=DEV)
        rows = [list(range(STALL_ROWS))] * 2
        for t in range(1, STALL_STEPS + 1):
            P.at(t - 1)
            P.apply(rows, [(G, G)] * 2)
        out = P.result()
        assert all(bool((kd["stamp"] == STALL_STEPS).all()) for kd in out)
        return [[kd["p0"].float().numpy(), kd["p1"].float().numpy()] for kd in out]
    means = check_stall(run)
    print("stall: mean displacement in spacings per table", [f"{x:.3f}" for x in means])


# --------------------------------------------------------------------------- 3. the schedules
T_END = 140
REPLAY_HP = (0.9, 0.999, 1e-8, 1e-2)
LAGS = (1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 130)
ROWS = (300, 200)


def _lr(s):
    return 1e-3 if s <= 70 else 5e-4        # (a scheduler's change inside every owed span)


def _replay_tables(D):
    g = torch.Generator().manual_seed(100 + D)
    base = {}
    for j in (0, 1):        # the two kinds start from the same values: the kind enters the bits
        base[f"p{j}"] = (torch.randn(ROWS[0], D, generator=g) * 0.1).to(torch.bfloat16)
        base[f"m{j}"] = torch.randn(ROWS[0], D, generator=g) * 1e-2
        base[f"v{j}"] = torch.rand(ROWS[0], D, generator=g) * 1e-3
    return [dict({k: v[:r].clone() for k, v in base.items()},
                 stamp=torch.zeros(r, dtype=torch.int32)) for r in ROWS]


def _lagged(P, **how):
    """Row r of either kind brought to T_END - LAGS[r % 11] in one replay, then every row to
    T_END in another (through the catch-up form ``how``)."""
    for lag in sorted(set(LAGS), reverse=True):
        P.at(T_END - lag)
        P.catchup([[r for r in range(n) if LAGS[r % len(LAGS)] == lag] for n in ROWS],
                  **{k: v for k, v in how.items() if k != "lock"})
    P.at(T_END)
    P.catchup([list(range(n)) for n in ROWS], **how)


def _schedule(D, dtype, seed, how):
    P = Pairs(_replay_tables(D), D, dtype, seed, _lr, REPLAY_HP, T_END)
    if how == "every_step":
        rows = [list(range(n)) for n in ROWS]
        for t in range(1, T_END + 1):
            P.at(t)
            P.catchup(rows)
    elif how in ("sweep", "parts"):
        for t in range(1, T_END + 1):
            P.at(t)
            for part in (range(3) if how == "parts" else [None]):
                P.sweep(8, part, 3)
        P.at(T_END)
        for part in ((2, 0, 1) if how == "parts" else [None]):
            P.sweep(1, part, 3)
    else:
        _lagged(P, **dict(lagged={}, claim=dict(claim=True), lock=dict(lock=1),
                          fused=dict(fused=True))[how])
    return P.result()


@pytest.mark.parametrize("D", [16, 64, 128])
def test_every_schedule_of_the_same_steps_stores_the_same_bits(D):
    from ncf_amd import _lib
    want = _schedule(D, _lib.DTYPE_BF16_SR, SEED, "every_step")
    for how in ("lagged", "sweep", "parts", "claim", "lock", "fused"):
        got = _schedule(D, _lib.DTYPE_BF16_SR, SEED, how)
        for k, (a, b) in enumerate(zip(got, want)):
            for n in NAMES:
                assert torch.equal(a[n], b[n]), (how, k, n)
            assert bool((b["stamp"] == T_END).all())
            if how == "lock":       # the listed rows are marked in flight, at the same step
                assert bool((a["stamp"] == (T_END | LOCK)).all())
            else:
                assert torch.equal(a["stamp"], b["stamp"]), (how, k)
    near = _schedule(D, _lib.DTYPE_BF16, SEED, "every_step")
    other = _schedule(D, _lib.DTYPE_BF16_SR, SEED + 1, "every_step")
    for k in (0, 1):
        for n in ("p0", "p1"):
            assert not torch.equal(want[k][n], near[k][n]), (k, n)
            assert not torch.equal(want[k][n], other[k][n]), (k, n)
    # the kind and the table enter the bits: equal inputs, different stored values
    r = ROWS[1]
    assert not torch.equal(want[0]["p0"][:r], want[1]["p0"])
    assert torch.equal(near[0]["p0"][:r], near[1]["p0"])


def test_the_row_sharded_apply_refuses_stochastic_rounding():
    """ncf_adam_pairs_apply_gsum_clock returns NCF_ERR_ARG for NCF_DTYPE_BF16_SR before any
    launch, as every pairs entry point does for a dtype it does not know."""
    from ncf_amd import _lib
    P = Pairs(_replay_tables(64), 64, _lib.DTYPE_BF16_SR, SEED, _lr, REPLAY_HP, 4)
    before = P.result()
    cnt, mx = P.ids([[0, 1], [0, 1]])
    got = torch.zeros(4, 128, device=DEV)
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.NCFArgumentError):
        _lib.call("ncf_adam_pairs_apply_gsum_clock", P.addr(), 2, 64, cnt.data_ptr(), mx, 1,
                  got.data_ptr(), pos.data_ptr(), pos.data_ptr(), 1, P.clock.data_ptr(),
                  P.table.data_ptr(), *REPLAY_HP, P.st)
    for pr in P.pairs:
        pr.param_dtype = 7
    with pytest.raises(_lib.NCFArgumentError):
        P.catchup([[0, 1], [0, 1]])
    with pytest.raises(_lib.NCFArgumentError):
        P.sweep(8)
    after = P.result()
    for a, b in zip(after, before):
        assert all(torch.equal(a[k], b[k]) for k in a)


# --------------------------------------------------------------------------- 4. the step
STEP_SEED = 77


def _step_run(monkeypatch, steps=70, sw=None, split=None, **kw):
    """``steps`` FusedTrainStep steps at test_gpu_bf16's small shape (U = 3000, I = 500, B = 64),
    dropout 0.2, bf16 tables; -> (tables as bf16 bits, moments, the step).  ``split``: the run is
    cut there by export_optimizer_state / load_optimizer_state into a fresh step object."""
    import ncf_amd.deferred as Dm
    import ncf_amd.trainer as Tr
    from tests import dropout_stream as DS
    for mod, name, val in sw or ():
        monkeypatch.setattr({"trainer": Tr, "deferred": Dm}[mod], name, val)
    U, I, B = 3000, 500, 64
    torch.manual_seed(31)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
    kw = dict(dict(lr=1e-3, weight_decay=1e-5, table_dtype=torch.bfloat16), **kw)
    step = Tr.FusedTrainStep(m, **kw)
    base = step.base_seed
    batches = [(u.to(DEV), i.to(DEV), t.to(DEV)) for u, i, t in TB._batches(U, I, B, 5, steps, 32)]
    for s, (u, i, t) in enumerate(batches):
        if s == split:
            opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
            step.export_optimizer_state(opt)
            state = opt.state_dict()
            step = Tr.FusedTrainStep(m, **kw)
            step.load_optimizer_state(state)
            # the dropout stream of the first run: its base seed, the clock's seed at step s
            step.base_seed = base
            step.clock[1] = DS.clock_seed(base, s)
        nxt = batches[s + 1][:2] if s + 1 < steps and not kw.get("graph") else None
        step(u, i, t, next=nxt)
    step.sync()
    torch.cuda.synchronize()
    tabs = {k: bf16_bits(v) for k, v in step.tables_lp.items()}
    mom = {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
           for k, v in step.state.items()}
    return tabs, mom, step


def _same_run(a, b, what):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), (what, k)
        assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1]), (what, k)


SR_KW = dict(table_rounding="stochastic", rounding_seed=STEP_SEED)


@pytest.fixture(scope="module")
def sr_run():
    mp = pytest.MonkeyPatch()
    try:
        yield _step_run(mp, **SR_KW)
    finally:
        mp.undo()


@pytest.mark.parametrize("what,sw,kw", [
    ("apply_unfused", [("trainer", "FUSE_APPLY", False)], {}),
    ("tail_unfused", [("trainer", "FUSED_TAIL", False), ("deferred", "EARLY_CATCHUP", False)], {}),
    ("early_catchup", [("deferred", "EARLY_CATCHUP", True)], {}),
    ("late_catchup", [("deferred", "EARLY_CATCHUP", False)], {}),
    ("graph", [], dict(graph=True)),
    ("split", [], dict(split=33)),
])
def test_step_schedules_store_the_same_bits(monkeypatch, sr_run, what, sw, kw):
    split = kw.pop("split", None)
    got = _step_run(monkeypatch, sw=sw, split=split, **SR_KW, **kw)
    assert got[2].rounding_seed == STEP_SEED and got[2].deferred.stochastic
    _same_run(got, sr_run, what)


def test_step_seed_and_rounding_change_the_bits(monkeypatch, sr_run):
    other = _step_run(monkeypatch, table_rounding="stochastic", rounding_seed=STEP_SEED + 1)
    near = _step_run(monkeypatch, table_rounding="nearest")
    default = _step_run(monkeypatch)
    for k in sr_run[0]:
        assert not np.array_equal(sr_run[0][k], other[0][k]), k
        assert not np.array_equal(sr_run[0][k], near[0][k]), k
    _same_run(near, default, "nearest is the default")
    assert default[2].rounding_seed is None and not default[2].deferred.stochastic
    # (that the default's bits are the dense bf16 schedule's, ncf_adam_table_bf16, which this
    # feature does not touch, is test_gpu_bf16.test_bf16_deferred_bitwise_equals_dense_bf16)
    # a seed left out is drawn, and readable
    drawn = _step_run(monkeypatch, steps=2, table_rounding="stochastic")[2]
    assert isinstance(drawn.rounding_seed, int) and 0 <= drawn.rounding_seed < 2 ** 32


def test_constructor_refusals():
    from ncf_amd.trainer import FusedTrainStep
    torch.manual_seed(31)
    m = ncf.AdvancedNCF(300, 50, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.2, 4).to(DEV)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for kw in (dict(),                                                       # fp32 tables
               dict(table_dtype=torch.bfloat16, deferred=False),
               dict(table_dtype=torch.bfloat16, clock=False)):
        with pytest.raises(ValueError):
            FusedTrainStep(m, table_rounding="stochastic", **kw)
    with pytest.raises(ValueError):
        FusedTrainStep(m, table_dtype=torch.bfloat16, table_rounding="up")
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


# one step against the float64 oracle: a clocked bf16-table case on the fp32 tower, added to
# test_gpu_dropout's cases for gpu_run (data seed 1: bf16_d64_p02's batch)
ORACLE_CASE = "sr_bf16_d64_p02"


def oracle_case():
    from tests import test_gpu_dropout as TD
    if ORACLE_CASE not in TD.CASES:
        TD.CASES[ORACLE_CASE] = TD._case(64, 4, 5, 37, 0.2, 1, "clock", "fused_small",
                                         {"BF16_MM": False}, 1, None, table_dtype="bf16")
    return TD.CASES[ORACLE_CASE]


def check_step_tables(final, want64, seed, min_equal=0.99):
    """The four tables after one step (``final``: fp32, the stored bf16 widened) against the
    float64 oracle's (``want64``): every element a bf16 neighbour of the oracle's value, and at
    least ``min_equal`` of them the neighbour the restated bits choose.  -> the worst fraction."""
    from tests import test_gpu_dropout as TD
    worst = 1.0
    for k, K in TD.TABLE_KEYS.items():
        kind, j = int(k.endswith("item")), int(k.startswith("mlp"))
        x = want64[K].double().numpy()
        got = final[K].double().numpy()
        lo, hi, ulp = SR.neighbours(x)
        assert bool(((got == lo) | (got == hi)).all()), k
        e = np.arange(x.size, dtype=np.uint64).reshape(x.shape)
        frac = (np.abs(x) - np.abs(lo)) / ulp
        r = SR.bits(seed, kind, j, 1, e).astype(np.float64) / 65536.0
        same = float((got == np.where(frac + r >= 1.0, hi, lo)).mean())
        worst = min(worst, same)
        assert same >= min_equal, (k, same)
    return worst


def test_one_step_against_the_float64_oracle(monkeypatch):
    import ncf_amd.trainer as Tr
    from tests import test_gpu_dropout as TD
    c = oracle_case()

    class Step(Tr.FusedTrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **SR_KW))
    monkeypatch.setattr(Tr, "FusedTrainStep", Step)
    init, batches, rec, final = TD.gpu_run(ORACLE_CASE, monkeypatch, table_dtype=torch.bfloat16)
    assert rec[0]["seed"] == TD.case_seeds(ORACLE_CASE, 1)[0]
    _, ref = TD.oracle_run(init, batches, [rec[0]["seed"]], c["H"], c["M"], c["p"])
    worst = check_step_tables(final, ref, STEP_SEED)
    print(f"{ORACLE_CASE}: at least {worst:.4%} of a table's elements equal the restated decision")
    # nearest-even in its place fails the same check
    near = {K: ref[K].float().to(torch.bfloat16).float() for K in TD.TABLE_KEYS.values()}
    with pytest.raises(AssertionError):
        check_step_tables(near, ref, STEP_SEED)
