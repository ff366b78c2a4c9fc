"""torch.optim.AdamW on an AdvancedNCF through the fused path, and FusedTrainStep with
``decoupled_weight_decay=True``, against the CPU oracle model (oracle/ncf_oracle.py) stepped by
torch's own AdamW on the same batches.  MI355X only.

Model: U = 301, I = 97, B = 8 groups, M = 5, dropout 0, at D = 64 with 4 heads and at D = 16 with
one; sweep_every = 4 (the rolling sweep wraps within the run); 6 steps, lr 1e-3 -> 3e-4 after step
3, weight_decay 1e-2.  Parameters and moments are compared with tests/parity.py's tolerances
(parameters outside the zone: abs 1e-6); the sign-flip zone of a step is the elements with
reference |g| < parity.ZONE (no wd term: decoupled decay does not enter the moments).

The inputs (model seed 17, batch seed 23; max_grad_norm 0.9 at D = 16 and 1.4 at D = 64) are
chosen from the CPU oracle alone, and tests/test_adamw_cpu.py holds what they were chosen for: at
every step every tensor's zone is within parity.ZONE_CAP of its elements (one element in tensors
under 1000), every step of the clipped runs clips, and outside the zone the fp32 oracle stands
within half the tolerance of the same oracle run in float64 (3.6e-7 at most), so that two fp32
runs summing in different orders fit the 1e-6.  Decoupled decay leaves no wd p term beside g, so
on most seeds some tensor (user_product_attention.k_proj.weight first) has gradients of a few
1e-6 whose fp32 noise alone moves the parameter by about 1e-6.
"""
import copy

import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")
U, I, B, M, T = 301, 97, 8, 5, 8
GEOMS = {64: (4, [64, 32]), 16: (1, [32, 16])}       # D: heads, hidden
STEPS, LR, LR_LATE, LR_AFTER, WD, EVERY = 6, 1e-3, 3e-4, 3, 1e-2, 4
CLIP = {16: 0.9, 64: 1.4}     # max_grad_norm of the clipped cases: below every step's total norm


def kjt(u, i):
    return ncf.KeyedJaggedTensor.from_lengths_sync(
        keys=["user_id", "product_id"], values=torch.cat([u, i]),
        lengths=torch.ones(2 * u.numel(), dtype=torch.long, device=u.device))


def batches(n=STEPS + 2, seed=23):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        u = torch.randint(0, U, (B,), generator=g).repeat_interleave(M)
        i = torch.randint(0, I, (B * M,), generator=g)
        t = torch.zeros(B, M)
        t[:, 0] = 1
        out.append((u, i, t.reshape(-1, 1)))
    return out


def model(D, seed=17):
    H, hid = GEOMS[D]
    torch.manual_seed(seed)
    return ncf.AdvancedNCF(U, I, 5, 24, D, D, T, hid, H, 0.0, M - 1)


def lr_of(s):
    """lr of the (0-based) step s."""
    return LR if s < LR_AFTER else LR_LATE


class TorchStep:
    """torch's own optimizer over the oracle's leaf tensors, in the model's parameter order (so a
    state_dict of the model's optimizer loads), as the ``opt`` of O.train_step; optionally
    torch.nn.utils.clip_grad_norm_ first.  ``seen``: per step the gradients the optimizer saw."""

    def __init__(self, params, order, cls=torch.optim.AdamW, max_norm=None, **kw):
        self.order = order
        self.opt = cls([params[k] for k in order], lr=LR, weight_decay=WD, foreach=False, **kw)
        self.max_norm, self.seen, self.norms = max_norm, [], []

    def step(self, params, grads):
        for k in self.order:
            g = grads.get(k)
            params[k].grad = None if g is None else g.detach().clone()
        if self.max_norm is not None:
            self.norms.append(float(torch.nn.utils.clip_grad_norm_(
                [params[k] for k in self.order], self.max_norm, foreach=False)))
        self.seen.append({k: params[k].grad.clone() for k in grads if grads[k] is not None})
        self.opt.step()

    def moments(self, params):
        return {k: self.opt.state[params[k]] for k in self.order if params[k] in self.opt.state}


def oracle_run(D, init, order, data, first=0, max_norm=None, state=None, cls=torch.optim.AdamW,
               **kw):
    """The oracle model from ``init`` stepped by torch's optimizer over ``data`` (steps first ..):
    (parameters, moments, per parameter the zone mask of every step)."""
    H, hid = GEOMS[D]
    ref = {k: v.detach().clone() for k, v in init.items()}
    ts = TorchStep(ref, order, cls, max_norm, **kw)
    if state is not None:
        ts.opt.load_state_dict(state)
    zones = {}
    for s, (u, i, t) in enumerate(data, start=first):
        for g in ts.opt.param_groups:
            g["lr"] = lr_of(s)
        O.train_step(ref, ts, u, i, t, negative_samples=M - 1, num_heads=H, temporal_dim=T,
                     n_layers=len(hid))
        for k, g in ts.seen[-1].items():
            zones.setdefault(k, []).append(parity.zone_from_grads(g.numpy(), 0.0, 0.0))
    oracle_run.norms = ts.norms        # (the last run's total gradient norms before clipping)
    return ref, ts.moments(ref), zones


def setup(D, seed=17):
    m = model(D, seed)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    order = [n for n, _ in m.named_parameters()]
    return m.to(DEV), init, order


def assert_matches(m, moments_of, ref, mom, zones, lr=LR):
    """Model parameters and moments (``moments_of(name)`` -> state dict or None) against the
    oracle's, within parity's tolerances."""
    sd = m.state_dict()
    for k, zs in zones.items():
        parity.assert_params_close(k, sd[k].detach().cpu().numpy(), ref[k].numpy(), zs, lr)
        st = moments_of(k)
        assert st is not None, k
        assert float(st["step"]) == float(mom[k]["step"]), k
        for key in ("exp_avg", "exp_avg_sq"):
            parity.assert_moment_close(k, st[key].detach().cpu().numpy(), mom[k][key].numpy(), zs)


def dropin(D, make_opt, data, monkeypatch, steps=STEPS, seed=17):
    """The reference call pattern (model(kjt) -> BCELoss -> zero_grad -> backward -> step) with
    ``make_opt(params)``; the binding exists after the first step and no table ever holds a dense
    .grad."""
    from ncf_amd import optim
    monkeypatch.setattr(optim, "SWEEP_EVERY", EVERY)
    m, init, order = setup(D, seed)
    opt = make_opt(m.parameters())
    crit = torch.nn.BCELoss()
    m.train()
    for s, (u, i, t) in enumerate(data[:steps]):
        for g in opt.param_groups:
            g["lr"] = lr_of(s)
        loss = crit(m(kjt(u.to(DEV), i.to(DEV))), t.to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert optim.binding_of(opt, m) is not None, "torch.optim.AdamW fell off the fused path"
        assert all(p.grad is None for p in m.engine.table_params().values())
    return m, opt, init, order


def opt_moments(m, opt):
    st = opt.state_dict()["state"]
    idx = {n: i for i, (n, _) in enumerate(m.named_parameters())}
    return lambda k: st.get(idx[k])


@pytest.mark.parametrize("D", sorted(GEOMS))
@pytest.mark.parametrize("kind", ["AdamW", "Adam(decoupled_weight_decay=True)"])
def test_dropin_adamw_binds_and_matches_torch(D, kind, monkeypatch):
    kw = {} if kind == "AdamW" else {"decoupled_weight_decay": True}
    cls = torch.optim.AdamW if kind == "AdamW" else torch.optim.Adam
    data = batches()
    m, opt, init, order = dropin(D, lambda ps: cls(ps, lr=LR, weight_decay=WD, **kw), data,
                                 monkeypatch)
    from ncf_amd import optim
    b = optim.binding_of(opt, m)
    assert b.decoupled and b.D is not None and b.D.decoupled
    ref, mom, zones = oracle_run(D, init, order, data[:STEPS], cls=cls, **kw)
    assert_matches(m, opt_moments(m, opt), ref, mom, zones)


def fused(D, data, steps=STEPS, **kw):
    from ncf_amd.trainer import FusedTrainStep
    m, init, order = setup(D)
    step = FusedTrainStep(m, lr=LR, weight_decay=WD, sweep_every=EVERY,
                          decoupled_weight_decay=True, **kw)
    dev = [(u.to(DEV), i.to(DEV), t.to(DEV)) for u, i, t in data]
    for s in range(steps):
        step.lr = lr_of(s)
        step(*dev[s])
    step.sync()
    torch.cuda.synchronize()
    return m, step, init, order


def fused_moments(m, step):
    opt = torch.optim.AdamW(m.parameters(), lr=LR, weight_decay=WD)
    step.export_optimizer_state(opt)
    by_name = dict(m.named_parameters())
    return lambda k: opt.state.get(by_name[k])


def bits(m, step):
    out = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    f = fused_moments(m, step)
    for k, _ in m.named_parameters():
        st = f(k)
        if st is not None:
            out[k + "/m"], out[k + "/v"] = st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone()
    return out


@pytest.mark.parametrize("D", sorted(GEOMS))
def test_fused_step_decoupled_matches_torch_adamw(D):
    data = batches()
    m, step, init, order = fused(D, data)
    assert step.deferred is not None and step.deferred.decoupled
    ref, mom, zones = oracle_run(D, init, order, data[:STEPS])
    assert_matches(m, fused_moments(m, step), ref, mom, zones)
    eager = bits(m, step)
    mg, sg, _, _ = fused(D, data, graph=True)          # captured: the same bits
    got = bits(mg, sg)
    assert eager.keys() == got.keys()
    for k in eager:
        assert torch.equal(eager[k], got[k]), ("graph", k)
    md, sd_, _, _ = fused(D, data, deferred=False)      # the dense per-step schedule: the same bits
    got = bits(md, sd_)
    for k in eager:
        assert torch.equal(eager[k], got[k]), ("deferred=False", k)


@pytest.mark.parametrize("D", sorted(GEOMS))
def test_fused_step_decoupled_with_clipping_matches_clip_grad_norm(D):
    data = batches()
    m, step, init, order = fused(D, data, max_grad_norm=CLIP[D])
    ref, mom, zones = oracle_run(D, init, order, data[:STEPS], max_norm=CLIP[D])
    assert_matches(m, fused_moments(m, step), ref, mom, zones)


def test_state_round_trip_into_stock_adamw(monkeypatch):
    """Four fused steps; the optimizer's state_dict loads into a stock torch.optim.AdamW over the
    oracle's tensors; two more steps there equal two more fused steps."""
    D, data = 64, batches()
    m, opt, init, order = dropin(D, lambda ps: torch.optim.AdamW(ps, lr=LR, weight_decay=WD), data,
                                 monkeypatch, steps=4)
    osd = copy.deepcopy(opt.state_dict())      # (its tensors are the live kernel buffers)
    msd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    # (a copy: torch keeps a CPU ``step`` of the dict it loads by reference and counts on it)
    ref, mom, zones = oracle_run(D, msd, order, data[4:6], first=4, state=copy.deepcopy(osd))
    crit = torch.nn.BCELoss()
    for s, (u, i, t) in enumerate(data[4:6], start=4):
        for g in opt.param_groups:
            g["lr"] = lr_of(s)
        loss = crit(m(kjt(u.to(DEV), i.to(DEV))), t.to(DEV))
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert_matches(m, opt_moments(m, opt), ref, mom, zones, lr=LR_LATE)
    # and back: a stock AdamW's state into the fused path
    m2, init2, _ = setup(D, seed=9)
    m2.load_state_dict(msd)
    o2 = torch.optim.AdamW(m2.parameters(), lr=LR, weight_decay=WD)
    o2.load_state_dict(osd)
    for s, (u, i, t) in enumerate(data[4:6], start=4):
        for g in o2.param_groups:
            g["lr"] = lr_of(s)
        loss = crit(m2(kjt(u.to(DEV), i.to(DEV))), t.to(DEV))
        o2.zero_grad()
        loss.backward()
        o2.step()
    a, b = m.state_dict(), m2.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_coupled_adam_is_untouched_by_an_adamw_model_in_between(monkeypatch):
    data = batches()

    def adam_bits():
        m, opt, _, _ = dropin(64, lambda ps: torch.optim.Adam(ps, lr=LR, weight_decay=WD), data,
                              monkeypatch, seed=5)
        from ncf_amd import optim
        assert not optim.binding_of(opt, m).decoupled
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        st = opt.state_dict()["state"]
        return sd, {k: (s["exp_avg"].cpu().clone(), s["exp_avg_sq"].cpu().clone()) for k, s in st.items()}
    a = adam_bits()
    dropin(64, lambda ps: torch.optim.AdamW(ps, lr=LR, weight_decay=WD), data, monkeypatch, seed=5)
    b = adam_bits()
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        assert torch.equal(a[1][k][0], b[1][k][0]) and torch.equal(a[1][k][1], b[1][k][1]), k


def test_decay_rule_switch_rebinds(monkeypatch):
    """A group that switches from coupled to decoupled decay mid-run gets a new binding (the old
    one settles every row under its own rule first)."""
    from ncf_amd import optim
    data = batches()
    m, opt, _, _ = dropin(16, lambda ps: torch.optim.Adam(ps, lr=LR, weight_decay=WD), data,
                          monkeypatch, steps=2)
    b0 = optim.binding_of(opt, m)
    assert not b0.decoupled
    for g in opt.param_groups:
        g["decoupled_weight_decay"] = True
    crit = torch.nn.BCELoss()
    u, i, t = data[2]
    loss = crit(m(kjt(u.to(DEV), i.to(DEV))), t.to(DEV))
    opt.zero_grad()
    loss.backward()
    opt.step()
    b1 = optim.binding_of(opt, m)
    assert b1 is not b0 and b1.decoupled and b1.step == 3
