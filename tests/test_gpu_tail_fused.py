"""The late catch-up of the next batch's rows inside the first launch of the step's final
reductions (ncf_reduce_batch_catchup, trainer.FUSED_TAIL): the entry point against the two it
replaces and the step against the side-stream schedule, bit for bit.
Runs on a real MI355X only (marker ``gpu``)."""
import ctypes

import numpy as np
import pytest
import torch

import _ncf_pkg

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")

T_NOW, REL = 200, 1            # clock->t and target_rel: the catch-up's target is step 201
TARGET = T_NOW + REL
HP = (0.9, 0.999, 1e-8, 1e-5)  # beta1, beta2, eps, weight decay
SHAPES = [(1, 3), (5, 64), (256, 260), (257, 1000)]   # (P, L)


def _step_table():
    """4 floats per step s at [4s .. 4s+3], padded past the target as deferred.py pads it (the
    replay fetches its scalars a chunk ahead)."""
    from ncf_amd import _lib
    steps = TARGET + 4096
    host = np.zeros(4 * (steps + 1), dtype=np.float32)
    _lib.call("ncf_adam_step_scalars", 1e-3, HP[0], HP[1], HP[2], 1, steps, host[4:].ctypes.data)
    return torch.from_numpy(host).to(DEV)


def _tables(D, bf, counts, max_n, seed):
    """Two kinds (700 user rows, 300 item rows), a GMF and an MLP table each with moments,
    stamps in [target - 130, target] (some equal to the target: left alone), 300 listed ids
    per kind in a buffer of max_n."""
    g = torch.Generator().manual_seed(seed)
    kinds = []
    for rows in (700, 300):
        t = {}
        for name in ("p0", "p1"):
            p = torch.randn(rows, D, generator=g) * 0.1
            t[name] = (p.to(torch.bfloat16) if bf else p).to(DEV)
        for name in ("m0", "m1"):
            t[name] = (torch.randn(rows, D, generator=g) * 1e-2).to(DEV)
        for name in ("v0", "v1"):
            t[name] = (torch.rand(rows, D, generator=g) * 1e-3).to(DEV)
        stamp = torch.randint(TARGET - 130, TARGET + 1, (rows,), generator=g, dtype=torch.int32)
        stamp[::9] = TARGET
        t["stamp"] = stamp.to(DEV)
        ids = torch.zeros(max(max_n, 300), dtype=torch.int64)
        ids[:300] = torch.randperm(rows, generator=g)[:300]
        t["ids"] = ids.to(DEV)
        kinds.append(t)
    return kinds, torch.tensor(counts, dtype=torch.int32, device=DEV)


def _descs(n, seed):
    """n descriptors cycling SHAPES with accumulate 0 / 1, scale 0.5, partial rows strided wider
    than L: [(partials, previous out, P, L, stride, accumulate)]."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        P, L = SHAPES[j % len(SHAPES)]
        stride = L + 8 if L % 4 == 0 else L + 3
        part = torch.from_numpy(rng.standard_normal((P, stride)).astype(np.float32)).to(DEV)
        prev = torch.from_numpy(rng.standard_normal(L).astype(np.float32)).to(DEV)
        out.append((part, prev, P, L, stride, (j // len(SHAPES)) % 2))
    return out


def _run(fused, descs, kinds, counts, max_n, D, bf, table, order=None):
    """Both pieces of work on clones of the inputs: the fused entry point, or ncf_reduce_batch
    then ncf_adam_pairs_catchup_lock_clock (lock 0).  Returns every tensor either may write."""
    from ncf_amd import _lib
    outs = [d[1].clone() for d in descs]
    lst = _lib.ReduceList()
    for j, ((part, _, P, L, stride, acc), o) in enumerate(zip(descs, outs)):
        d = lst.d[j]
        d.part, d.out, d.stride, d.ldo = part.data_ptr(), o.data_ptr(), stride, L
        d.L, d.cols, d.P, d.accumulate, d.scale, d.reserved = L, L, P, acc, 0.5, 0
    lst.count = len(descs)
    need = _lib.query("ncf_reduce_batch_scratch", lst.address)
    scratch = torch.zeros(max(need, 1), dtype=torch.float32, device=DEV)
    mine = [{k: v.clone() for k, v in t.items()} for t in kinds]
    pairs = (_lib.TablePair * 2)()
    for pr, t in zip(pairs, mine):
        pr.p0, pr.m0, pr.v0 = t["p0"].data_ptr(), t["m0"].data_ptr(), t["v0"].data_ptr()
        pr.p1, pr.m1, pr.v1 = t["p1"].data_ptr(), t["m1"].data_ptr(), t["v1"].data_ptr()
        pr.row_ids, pr.stamp, pr.rows = t["ids"].data_ptr(), t["stamp"].data_ptr(), t["stamp"].numel()
        pr.param_dtype = _lib.DTYPE_BF16 if bf else _lib.DTYPE_F32
    clock = torch.tensor([T_NOW, 12345], dtype=torch.int64, device=DEV)
    st = _lib.stream_ptr(DEV)
    pa = ctypes.addressof(pairs)
    if fused:
        prev = _lib.query("ncf_reduce_catchup_set_order", -1 if order is None else order)
        try:
            _lib.call("ncf_reduce_batch_catchup", lst.address, scratch.data_ptr(), scratch.numel(),
                      pa, 2, D, counts.data_ptr(), max_n, REL, clock.data_ptr(), table.data_ptr(),
                      *HP, st)
        finally:
            _lib.query("ncf_reduce_catchup_set_order", prev)
    else:
        _lib.call("ncf_reduce_batch", lst.address, scratch.data_ptr(), scratch.numel(), st)
        _lib.call("ncf_adam_pairs_catchup_lock_clock", pa, 2, D, counts.data_ptr(), max_n, REL, 0,
                  clock.data_ptr(), table.data_ptr(), *HP, st)
    torch.cuda.synchronize()
    assert clock.tolist() == [T_NOW, 12345]
    return outs, mine


def _same(a, b):
    (oa, ta), (ob, tb) = a, b
    for j, (x, y) in enumerate(zip(oa, ob)):
        assert torch.equal(x, y), ("reduction", j)
    for k, (x, y) in enumerate(zip(ta, tb)):
        for name in ("p0", "m0", "v0", "p1", "m1", "v1", "stamp"):
            assert torch.equal(x[name], y[name]), (k, name)


@pytest.fixture(scope="module")
def table():
    return _step_table()


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_entry_point_equals_the_two_calls(table, D, bf, order):
    """One launch group (8 descriptors: every (P, L) with accumulate 0 and 1), 300 of 320 listed
    rows per kind, every block order of the fused launch (ncf_reduce_catchup_set_order).  The catch-up must also have moved
    something: rows behind the target changed, rows at the target did not."""
    descs = _descs(8, 5)
    kinds, counts = _tables(D, bf, [300, 300], 320, seed=D + bf)
    want = _run(False, descs, kinds, counts, 320, D, bf, table)
    got = _run(True, descs, kinds, counts, 320, D, bf, table, order)
    _same(got, want)
    for k, t in enumerate(kinds):
        listed = t["ids"][:300]
        behind = listed[t["stamp"][listed] < TARGET]
        assert behind.numel() > 100
        assert (got[1][k]["stamp"][listed] == TARGET).all()
        assert not torch.equal(got[1][k]["p0"][behind], t["p0"][behind])
        rest = torch.ones(t["stamp"].numel(), dtype=torch.bool, device=DEV)
        rest[behind] = False
        assert torch.equal(got[1][k]["p1"][rest], t["p1"][rest])
        assert torch.equal(got[1][k]["stamp"][rest], t["stamp"][rest])
    for (_, prev, *_), o in zip(descs, got[0]):
        assert not torch.equal(o, prev)


def test_two_launch_groups_and_an_empty_kind(table):
    """30 descriptors (the fused launch holds the first 24, a plain stage-1 launch the rest;
    stage-2 scratch offsets run across both) and count = 0 for the users."""
    descs = _descs(30, 6)
    kinds, counts = _tables(64, False, [0, 300], 320, seed=3)
    want = _run(False, descs, kinds, counts, 320, 64, False, table)
    got = _run(True, descs, kinds, counts, 320, 64, False, table)
    _same(got, want)
    assert torch.equal(got[1][0]["stamp"], kinds[0]["stamp"])       # no user row listed
    assert not torch.equal(got[1][1]["stamp"], kinds[1]["stamp"])


@pytest.mark.parametrize("ndesc,max_n", [(0, 320), (8, 0), (0, 0)])
def test_empty_sides(table, ndesc, max_n):
    """An empty list (the plain catch-up runs), max_n = 0 (ncf_reduce_batch) and both (nothing
    is launched, NCF_OK)."""
    descs = _descs(ndesc, 7)
    kinds, counts = _tables(64, False, [300, 300], max_n, seed=4)
    want = _run(False, descs, kinds, counts, max_n, 64, False, table)
    got = _run(True, descs, kinds, counts, max_n, 64, False, table)
    _same(got, want)
    if max_n == 0:
        for k, t in enumerate(kinds):
            for name in ("p0", "m0", "v0", "p1", "m1", "v1", "stamp"):
                assert torch.equal(got[1][k][name], t[name]), (k, name)
    else:
        assert not torch.equal(got[1][0]["stamp"], kinds[0]["stamp"])
    if ndesc == 0:
        assert got[0] == []


# ------------------------------------------------------------------ the step
def _step_run(monkeypatch, on, **kw):
    """30 pipelined clocked steps with the late catch-up, trainer.FUSED_TAIL = on: the model's
    state, the table moments, the dense Adam state and the calls of the new entry point."""
    from ncf_amd import _lib
    import ncf_amd.trainer as Tr
    from tests.test_gpu_parity import _fused_run
    monkeypatch.setattr(Tr, "FUSED_TAIL", on)
    calls = []
    orig = _lib.call

    def counted(name, *a):
        if name == "ncf_reduce_batch_catchup":
            calls.append(name)
        return orig(name, *a)
    monkeypatch.setattr(_lib, "call", counted)
    steps = []
    sd, mom = _fused_run(True, 30, sweep_every=8, clock=True, overlap_sweep=True, pipelined=True,
                         on_step=lambda step, s: steps.append(step), **kw)
    monkeypatch.setattr(_lib, "call", orig)
    torch.cuda.synchronize()
    flat = (steps[-1].m_flat.cpu().clone(), steps[-1].v_flat.cpu().clone())
    assert (len(calls) >= 28) if on else len(calls) == 0, (on, kw, len(calls))
    return sd, mom, flat


def _same_state(a, b):
    (a_sd, a_m, a_f), (b_sd, b_m, b_f) = a, b
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k
    for k in a_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k
    assert torch.equal(a_f[0], b_f[0]) and torch.equal(a_f[1], b_f[1])


@pytest.mark.parametrize("kw", [dict(dropout=0.2), dict(dropout=0.2, U=400, I=150),
                                dict(dropout=0.2, table_dtype=torch.bfloat16)],
                         ids=["dropout", "rows_shared_with_the_previous_batch", "bf16_tables"])
def test_step_fused_tail_bitwise_equals_side_stream(monkeypatch, kw):
    """FUSED_TAIL on against off.  U=400, I=150: most rows of a batch are in the previous one
    too — the rows the fused apply has just stamped, which the catch-up must then leave alone."""
    import ncf_amd.deferred as Dm
    monkeypatch.setattr(Dm, "EARLY_CATCHUP", False)     # (on by default at this batch size)
    _same_state(_step_run(monkeypatch, True, **kw), _step_run(monkeypatch, False, **kw))


def test_step_fused_tail_bitwise_equals_dense(monkeypatch):
    """Without dropout: FUSED_TAIL on against off and against the dense schedule (every table
    swept every step)."""
    import ncf_amd.deferred as Dm
    from tests.test_gpu_parity import _fused_run
    monkeypatch.setattr(Dm, "EARLY_CATCHUP", False)
    on = _step_run(monkeypatch, True, dropout=0.0)
    _same_state(on, _step_run(monkeypatch, False, dropout=0.0))
    steps = []
    sd, mom = _fused_run(False, 30, on_step=lambda step, s: steps.append(step))
    flat = (steps[-1].m_flat.cpu().clone(), steps[-1].v_flat.cpu().clone())
    _same_state(on, (sd, mom, flat))
