"""A pipelined FusedTrainStep whose batch is above the early catch-up's limit, so the next
batch's rows are caught up late, inside the first launch of the step's final reductions, and
whose embedding backward has more LayerNorm partial rows than one
reduction stage (their first stage rides in the fix-up launch): against the dense schedule
(every table row stepped every step), bit for bit.
Runs on a real MI355X only (marker ``gpu``)."""
import pytest
import torch

import _ncf_pkg

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")

U, I, B, M, STEPS = 3000, 700, 2049, 5, 12


def _run(deferred, monkeypatch=None):
    from ncf_amd import _lib
    from ncf_amd.trainer import FusedTrainStep
    torch.manual_seed(11)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 32, [256, 128, 64], 4, 0.0, M - 1).to(DEV)
    kw = dict(sweep_every=8, clock=True, overlap_sweep=True) if deferred else {}
    step = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, deferred=deferred, **kw)
    g = torch.Generator().manual_seed(12)
    batches = []
    for _ in range(STEPS):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M).to(DEV)
        i = torch.randint(0, I, (B * M,), generator=g).to(DEV)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        batches.append((u, i, t.reshape(-1, 1).to(DEV)))
    calls, scratch = [], []
    if monkeypatch is not None:
        orig_call, orig_query = _lib.call, _lib.query

        def counted(name, *a):
            if name == "ncf_reduce_batch_catchup":
                calls.append(a[7])                       # max_n of the catch-up it carries
            return orig_call(name, *a)

        def queried(name, *a):
            r = orig_query(name, *a)
            if name == "ncf_reduce_batch_scratch":
                scratch.append(r)
            return r
        monkeypatch.setattr(_lib, "call", counted)
        monkeypatch.setattr(_lib, "query", queried)
    losses = []
    for s, (u, i, t) in enumerate(batches):
        nxt = batches[s + 1][:2] if deferred and s + 1 < STEPS else None
        step(u, i, t, next=nxt)
        losses.append(step.last_loss.detach().clone())
    if monkeypatch is not None:
        monkeypatch.undo()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}   # syncs deferred rows
    step.sync()
    mom = {k: (v["exp_avg"].cpu().clone(), v["exp_avg_sq"].cpu().clone())
           for k, v in step.state.items()}
    flat = (step.m_flat.cpu().clone(), step.v_flat.cpu().clone())
    return sd, mom, flat, torch.stack([x.reshape(()) for x in losses]).cpu(), calls, scratch


def test_late_tail_step_bitwise_equals_dense(monkeypatch):
    from ncf_amd import deferred as Dm
    assert not Dm.early_on(B * M) and Dm.early_on(B * M - M)     # just above the limit
    a_sd, a_m, a_f, a_loss, calls, scratch = _run(True, monkeypatch)
    # the late catch-up rode in the tail launch, and the step's list needed no stage-2 scratch
    assert len(calls) >= STEPS - 2 and all(n >= B * M for n in calls), calls
    assert scratch and all(r == 0 for r in scratch), scratch
    b_sd, b_m, b_f, b_loss, _, _ = _run(False)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
    assert torch.equal(bits(a_loss), bits(b_loss))
    for k in b_sd:
        assert torch.equal(bits(a_sd[k]), bits(b_sd[k])), k
    for k in b_m:
        assert torch.equal(a_m[k][0], b_m[k][0]) and torch.equal(a_m[k][1], b_m[k][1]), k
    assert torch.equal(a_f[0], b_f[0]) and torch.equal(a_f[1], b_f[1])
