"""Top-k scoring at an hour of day (``score_topk(hour=)``: forward_simple's hour path through the
factorised scorer): ncf_score_queries_hour at the C ABI, the pipeline against the reference's own
outputs (F6) and against the float64 oracle, mixed hours, ``exclude``, the captured graph, item
shards, invalidation, metrics and the refusals.  Runs on a real MI355X only (marker ``gpu``).

Reference: ``oracle.forward_simple_hour`` in float64 per user over all items, ordered by (score
desc, item id asc); items identical except between oracle scores tied within 2e-6, scores within
2e-6 (the tolerance of the hour forward, test_gpu_parity.test_f6_forward_simple_hour)."""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import _lib, scoring  # noqa: E402
from ncf_amd._lib import ptr  # noqa: E402
from ncf_amd.engine import LN_EPS  # noqa: E402
from ncf_amd.scoring import (GraphedScorer, ItemIndex, SeenItems, merge_topk,  # noqa: E402
                             score_topk, shard_items)
DEV = torch.device("cuda:0")
ATOL = 2e-6
MAX_ERR = []     # every |score - oracle| maximum seen (printed by the last test)


def _model(U, I, seed, *more):
    torch.manual_seed(seed)
    return ncf.AdvancedNCF(U, I, 5, 24, *more).to(DEV).eval()


def _proj(T, D, seed):
    torch.manual_seed(seed)
    return torch.nn.Linear(T, D).to(DEV)


class _Ref:
    """The oracle's rows, one forward_simple_hour call per (user, hour), computed on first use and
    shared by the tests of a module fixture (never written to)."""

    def __init__(self, m, proj, I, num_heads=4, n_layers=3):
        self.p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
        self.w = None if proj is None else proj.weight.detach().cpu().double()
        self.b = None if proj is None else proj.bias.detach().cpu().double()
        self.I, self.H, self.L = I, num_heads, n_layers
        self.rows = {}

    def row(self, u, h):
        r = self.rows.get((u, h))
        if r is None:
            items = torch.arange(self.I)
            r = self.rows[(u, h)] = O.forward_simple_hour(
                self.p, torch.full_like(items, u), items, torch.full_like(items, h), self.w,
                self.b, num_heads=self.H, n_layers=self.L)
        return r

    def __call__(self, users, hours):
        hours = [hours] * len(users) if isinstance(hours, int) else hours.tolist()
        return torch.stack([self.row(u, h) for u, h in zip(users.tolist(), hours)])


def _seen(lists, U, I):
    rows = [sorted(set(int(x) for x in lists.get(u, ()))) for u in range(U)]
    off = np.zeros(U + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    items = np.array([x for r in rows for x in r], dtype=np.int32)
    return SeenItems.from_csr(torch.from_numpy(off), torch.from_numpy(items), I).to(DEV), rows


def _assert_vs_oracle(s, it, ref, users, k, rows=None):
    """test_gpu_score_exclude._assert_vs_oracle at the hour forward's 2e-6."""
    for r, u in enumerate(users.tolist()):
        row = ref[r].clone()
        seen = rows[u] if rows is not None else []
        if seen:
            row[seen] = float("-inf")
        order = torch.argsort(-row, stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        assert not set(got) & set(seen), (r, u)              # exact: nothing seen comes back
        assert min(got) >= 0 and len(set(got)) == k
        if got != order:    # only between oracle scores tied within the tolerance
            np.testing.assert_allclose(ref[r, got].numpy(), ref[r, order].numpy(), atol=ATOL)
        err = (s[r].cpu().double() - ref[r, got]).abs().max().item()
        MAX_ERR.append(err)
        assert err <= ATOL, (r, u, err)


# ------------------------------------------------------------ 1. the reference's own outputs
def test_f6_ranking_equals_the_references(f5, f6):
    """The demo model (F5's state dict, 366 items) at F6's four (user, hour, projection) cases:
    the top 10 are the stable descending argsort of the reference's own scores (the smallest
    gap among the top 11 of any case is 3.4e-4) and the scores are within 2e-6 of them."""
    sd = {k[3:]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in f5.items()
          if k.startswith("sd/")}
    nu = sd["mf_embedding_collection.embedding_bags.user_id.weight"].shape[0]
    m = ncf.AdvancedNCF(nu, 366, 5, 24).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.eval()
    for c in range(len(f6["hours"])):
        want = torch.from_numpy(np.ascontiguousarray(f6["scores"][c]))
        order = torch.argsort(-want, stable=True)[:11]
        assert float((want[order][:-1] - want[order][1:]).min()) > 1e-4     # the fixture's gaps
        idx = ItemIndex(m, projection=(torch.from_numpy(f6["proj_w"][c]),
                                       torch.from_numpy(f6["proj_b"][c])))
        s, it = score_topk(m, torch.tensor([int(f6["user_pos"][c])]), k=10, index=idx,
                           hour=int(f6["hours"][c]))
        assert it[0].cpu().tolist() == order[:10].tolist(), c
        np.testing.assert_allclose(s[0].cpu().numpy(), want[order[:10]].numpy(), atol=ATOL)


# ------------------------------------------------------------------- 2. against the oracle
U0, I0 = 300, 20011


@pytest.fixture(scope="module")
def world():
    """Two models over 20011 items (T = 32 with a projection; T = 64 = D without), their
    indexes, 37 users with repeats (12 distinct) and the lazily computed oracle rows."""
    g = torch.Generator().manual_seed(17)
    # (12 distinct users: an oracle row over 20011 items takes a quarter of a second)
    users = torch.randperm(U0, generator=g)[:12][torch.randint(0, 12, (37,), generator=g)]
    assert len(set(users.tolist())) < 37
    out = {"users": users}
    for T, seed in ((32, 3), (64, 4)):
        m = _model(U0, I0, seed, 64, 64, T)
        proj = _proj(32, 64, 50) if T == 32 else None
        idx = ItemIndex(m, projection=proj)
        out[T] = (m, proj, idx, _Ref(m, proj, I0))
    return out


@pytest.mark.parametrize("k,cap", [(1, 8192), (10, 8192), (100, 8192), (100, 128)])
@pytest.mark.parametrize("hour", [0, 13, 23])
@pytest.mark.parametrize("T", [32, 64])
def test_hour_vs_oracle(world, T, hour, k, cap):
    """The sample stride is above 1 (20011 items) in lists of 8192; lists of 128 at k = 100
    overflow and re-run (their plan samples every item: 2 k I / cap > I)."""
    m, _, idx, ref = world[T]
    users = world["users"]
    plan = scoring._TopKRun(idx.at_hour(hour), 37, k, cap)
    assert (plan.stride > 1) == (cap == 8192) and plan.hours is not None
    s, it = score_topk(m, users, k=k, index=idx, cap=cap, hour=hour)
    assert s.shape == (37, k) and it.dtype == torch.int64
    _assert_vs_oracle(s, it, ref(users, hour), users, k)


def test_hours_rank_differently(world):
    """The hour matters: the hour-0, hour-13 and hour=None top 10 are different lists."""
    m, _, idx, _ = world[32]
    users = world["users"]
    lists = [score_topk(m, users, 10, idx, hour=h)[1] for h in (0, 13, None)]
    assert not torch.equal(lists[0], lists[1]) and not torch.equal(lists[0], lists[2])


def test_hour_d128_vs_oracle():
    """D = 128: the fp32 scan's 128-deep form (k_collect<128>) and k_queries<128> with the hour."""
    U, I, k = 60, 3001, 10
    m = _model(U, I, 41, 128, 128, 32, [256, 128, 64], 4, 0.2, 4)
    proj = _proj(32, 128, 51)
    idx = ItemIndex(m, projection=proj)
    assert idx.p.shape[1] == 128 and idx.p3 is None and idx.pmax is None
    users = torch.arange(0, U, 3)
    ref = _Ref(m, proj, I)
    for hour in (0, 13):
        s, it = score_topk(m, users, k=k, index=idx, hour=hour)
        _assert_vs_oracle(s, it, ref(users, hour), users, k)


# ---------------------------------------------------------------- 3. the kernel at the C ABI
def _queries(D, uid, table, gamma, beta, w_mf, final_w, hours=None, scale=None, n=None):
    qd = max(64, D)
    n = uid.numel() if n is None else n
    q = torch.full((uid.numel(), qd), -77.0, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr(DEV)
    if hours is None:
        _lib.call("ncf_score_queries", ptr(uid), n, ptr(table), table.shape[0], D, ptr(gamma),
                  ptr(beta), LN_EPS, ptr(w_mf), ptr(final_w), ptr(q), ptr(err), st)
    else:
        _lib.call("ncf_score_queries_hour", ptr(uid), ptr(hours), n, ptr(table), table.shape[0],
                  D, ptr(gamma), ptr(beta), LN_EPS, ptr(w_mf), ptr(final_w), ptr(scale), ptr(q),
                  ptr(err), st)
    torch.cuda.synchronize()
    return q, int(err.item())


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_queries_hour_kernel(D):
    """ncf_score_queries_hour == ncf_score_queries' row times scale[hours] (one fp32 multiply, so
    bit for bit), neighbouring rows at different hours (a wave of 64 lanes holds 64 / (D / 4) rows,
    so several hours), the pad columns zero, an all-ones table the plain row's bits; hours -1 and
    24 flag bit 2 only and give the hour-0 row, a bad user id bit 1 only; n = 0 writes nothing."""
    g = torch.Generator().manual_seed(D)
    R, n = 50, 37
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)  # noqa: E731
    table, gamma, beta, w_mf, final_w = r(R, D), 1 + 0.1 * r(D), 0.1 * r(D), r(1, D), r(1, 2)
    scale = (1 + 0.3 * r(24, D)).contiguous()
    uid = torch.randint(0, R, (n,), generator=g).to(DEV)
    hours = ((torch.arange(n) * 7 + 3) % 24).to(DEV)
    assert bool((hours[1:] != hours[:-1]).all()) and len(set(hours.tolist())) == 24
    args = (D, uid, table, gamma, beta, w_mf, final_w)
    plain, e0 = _queries(*args)
    got, e1 = _queries(*args, hours, scale)
    assert e0 == 0 and e1 == 0
    want = plain.clone()
    want[:, :D] = plain[:, :D] * scale[hours]
    assert torch.equal(got, want)
    assert bool((got[:, D:] == 0).all()) and got.shape[1] == max(64, D)
    ones, e2 = _queries(*args, hours, torch.ones(24, D, device=DEV))
    assert e2 == 0 and torch.equal(ones, plain)
    # the last row of the table is not read past: a table of exactly 24 rows, hour 23
    h23, _ = _queries(*args, torch.full_like(hours, 23), scale)
    assert torch.equal(h23[:, :D], plain[:, :D] * scale[23])
    # hours out of range: bit 2 only, the hour-0 row
    bad_h = hours.clone()
    bad_h[4], bad_h[30] = -1, 24
    got_b, eb = _queries(*args, bad_h, scale)
    fixed = bad_h.clone()
    fixed[4] = fixed[30] = 0
    want_b = plain.clone()
    want_b[:, :D] = plain[:, :D] * scale[fixed]
    assert eb == 2 and torch.equal(got_b, want_b)
    # a bad user id: bit 1 only, row 0 of the table
    bad_u = uid.clone()
    bad_u[9], bad_u[21] = R, -1
    got_u, eu = _queries(D, bad_u, table, gamma, beta, w_mf, final_w, hours, scale)
    fixed_u = bad_u.clone()
    fixed_u[9] = fixed_u[21] = 0
    want_u, _ = _queries(D, fixed_u, table, gamma, beta, w_mf, final_w, hours, scale)
    assert eu == 1 and torch.equal(got_u, want_u)
    # both at once: both bits
    _, eub = _queries(D, bad_u, table, gamma, beta, w_mf, final_w, bad_h, scale)
    assert eub == 3
    # n = 0 launches nothing: the buffer keeps its sentinel
    none, en = _queries(*args, hours, scale, n=0)
    assert en == 0 and bool((none == -77.0).all())


# -------------------------------------------------------------------------- 4. mixed hours
def test_mixed_hours(world):
    """One call over users at 6 distinct hours (a group of one user, a group of 40): bitwise the
    per-hour int calls, in the caller's order, and the oracle's ranking."""
    m, _, idx, ref = world[32]
    g = torch.Generator().manual_seed(29)
    hours = torch.tensor([13] * 40 + [5] + [0] * 6 + [23] * 9 + [7] * 3 + [18] * 4)
    perm = torch.randperm(hours.numel(), generator=g)
    hours = hours[perm]
    n = hours.numel()
    users = world["users"][torch.randint(0, 37, (n,), generator=g)]
    assert len(set(hours.tolist())) >= 5
    assert sorted(len(p) for _, p in scoring.group_by_hour(hours)) == [1, 3, 4, 6, 9, 40]
    for k in (10, 100):
        s, it = score_topk(m, users, k=k, index=idx, hour=hours)
        for h in hours.unique().tolist():
            pos = (hours == h).nonzero().flatten()
            hs, hi = score_topk(m, users[pos], k=k, index=idx, hour=h)
            assert torch.equal(s[pos.to(DEV)], hs) and torch.equal(it[pos.to(DEV)], hi), h
        _assert_vs_oracle(s, it, ref(users, hours), users, k)
    # a tensor of one hour is that hour's call; device tensors and int32 are taken as well
    s1, i1 = score_topk(m, users, k=10, index=idx, hour=torch.full((n,), 13, dtype=torch.int32,
                                                                   device=DEV))
    s2, i2 = score_topk(m, users, k=10, index=idx, hour=13)
    assert torch.equal(s1, s2) and torch.equal(i1, i2)
    # no users
    s0, i0 = score_topk(m, users[:0], k=10, index=idx, hour=hours[:0])
    assert s0.shape == (0, 10) and i0.shape == (0, 10)


# ----------------------------------------------------------------- 5. hour=None is untouched
def test_hour_none_is_untouched(world):
    m, proj, idx, _ = world[32]
    users = world["users"]
    plain = ItemIndex(m)
    idx.hour_bias(3)        # (hour state on the index changes nothing either)
    for k in (10, 100):
        s0, i0 = score_topk(m, users, k, plain)
        s1, i1 = score_topk(m, users, k, idx)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
    assert torch.equal(plain.bias, idx.bias) and torch.equal(plain.p, idx.p)
    # the projection given with the index must be the index's own
    score_topk(m, users, 10, idx, projection=proj)
    with pytest.raises(ValueError, match="projection"):
        score_topk(m, users, 10, idx, hour=3, projection=_proj(32, 64, 99))
    with pytest.raises(ValueError, match="projection"):
        score_topk(m, users, 10, plain, hour=3, projection=proj)
    # a call that builds the index itself takes it
    s2, i2 = score_topk(m, users, 10, hour=3, projection=proj)
    s3, i3 = score_topk(m, users, 10, idx, hour=3)
    assert torch.equal(s2, s3) and torch.equal(i2, i3)


# ------------------------------------------------------------------------- 6. with exclude
@pytest.mark.parametrize("k,cap", [(10, 8192), (100, 128)])
def test_hour_with_exclude(world, k, cap):
    """Histories of 0..50 random items; one user has seen its own top 50 at that hour."""
    m, _, idx, ref = world[32]
    users = world["users"]
    hour = 13
    g = torch.Generator().manual_seed(31)
    lists = {}
    for u in range(U0):
        cnt = int(torch.randint(0, 51, (1,), generator=g))
        lists[u] = torch.randperm(I0, generator=g)[:cnt].tolist()
    u_top = int(users[3])
    _, top = score_topk(m, torch.tensor([u_top]), k=50, index=idx, hour=hour)
    lists[u_top] = top[0].cpu().tolist()
    seen, rows = _seen(lists, U0, I0)
    s, it = score_topk(m, users, k=k, index=idx, cap=cap, exclude=seen, hour=hour)
    _assert_vs_oracle(s, it, ref(users, hour), users, k, rows)
    r = (users == u_top).nonzero().flatten()[0]
    assert not set(it[r].tolist()) & set(lists[u_top])


# --------------------------------------------------------------------------------- 7. graph
def test_graphed_scorer_at_hours():
    """One captured graph serves every hour (the hour buffer, the bias buffer and the sample's
    bias rows are overwritten in place); a parameter change re-captures; mixed hours are
    refused; an hour=None scorer is as before and refuses an hour."""
    m = _model(U0, I0, 9, 64, 64, 32)
    proj = _proj(32, 64, 52)
    idx = ItemIndex(m, projection=proj)
    g = torch.Generator().manual_seed(10)
    n, k = 37, 10
    sc = GraphedScorer(m, n, k, index=idx, hour=0)
    graph, run = sc.graph, sc.run
    bias_ptr, sbias_ptr = run.index.bias.data_ptr(), run.sbias.data_ptr()
    for h in (3, 17, 3):
        users = torch.randint(0, U0, (n,), generator=g).to(DEV)
        gs, gi = sc(users, hour=h)
        es, ei = score_topk(m, users, k=k, index=idx, hour=h)
        assert torch.equal(gs, es) and torch.equal(gi, ei), h
        assert sc.graph is graph and sc.run is run
        assert run.index.bias.data_ptr() == bias_ptr and run.sbias.data_ptr() == sbias_ptr
    gs2, gi2 = sc(users)                       # no hour: the last one
    assert torch.equal(gs2, gs) and torch.equal(gi2, gi)
    assert not torch.equal(gi, score_topk(m, users, k=k, index=idx, hour=17)[1])
    with pytest.raises(ValueError, match="score_topk"):
        sc(users, hour=torch.arange(n) % 24)
    with pytest.raises(IndexError):
        sc(users, hour=24)
    gs3, gi3 = sc(users, hour=torch.full((n,), 3))      # one hour as a tensor is fine
    assert torch.equal(gs3, gs) and torch.equal(gi3, gi) and sc.graph is graph
    with torch.no_grad():
        m.final[0].bias.add_(0.25)
    gs4, gi4 = sc(users, hour=17)
    assert sc.graph is not graph
    es4, ei4 = score_topk(m, users, k=k, index=ItemIndex(m, projection=proj), hour=17)
    assert torch.equal(gs4, es4) and torch.equal(gi4, ei4)
    assert not torch.equal(gs4, score_topk(m, users, k=k, index=sc.index, hour=3)[0])
    # a scorer without an hour replays as before and refuses one
    plain = GraphedScorer(m, n, k, index=sc.index)
    pg = plain.graph
    ps, pi = plain(users)
    es, ei = score_topk(m, users, k=k, index=sc.index)
    assert torch.equal(ps, es) and torch.equal(pi, ei) and plain.run.hours is None
    with pytest.raises(ValueError, match="hour"):
        plain(users, hour=3)
    ps2, pi2 = plain(users)
    assert torch.equal(ps2, ps) and torch.equal(pi2, pi) and plain.graph is pg


def test_graphed_scorer_at_hours_overflow_and_exclude():
    """k = 100 in lists of 128 overflows: the eager re-run after the replay reads the scorer's
    own bias buffer, with seen items as well."""
    m = _model(U0, I0, 11, 64, 64, 64)
    g = torch.Generator().manual_seed(12)
    n, k, cap = 37, 100, 128
    lists = {u: torch.randperm(I0, generator=g)[:20].tolist() for u in range(U0)}
    seen, rows = _seen(lists, U0, I0)
    sc = GraphedScorer(m, n, k, cap=cap, exclude=seen, hour=5)
    for h in (5, 21):
        users = torch.randint(0, U0, (n,), generator=g).to(DEV)
        gs, gi = sc(users, hour=h)
        es, ei = score_topk(m, users, k=k, index=sc.index, cap=cap, exclude=seen, hour=h)
        assert torch.equal(gs, es) and torch.equal(gi, ei), h
        for row, u in enumerate(users.tolist()):
            assert not set(gi[row].tolist()) & set(rows[u])


# -------------------------------------------------------------------------------- 8. shards
@pytest.mark.parametrize("strided", [False, True])
def test_hour_on_item_shards(strided):
    """W = 3 item shards, each with the hour's bias over its own ids: the merged per-shard lists
    are the whole catalogue's, with and without exclude."""
    U, I, k, W, hour = 200, 5003, 10, 3, 13
    m = _model(U, I, 5, 64, 64, 32)
    proj = _proj(32, 64, 53)
    g = torch.Generator().manual_seed(6)
    users = torch.randint(0, U, (45,), generator=g)
    lists = {u: torch.randperm(I, generator=g)[:int(torch.randint(0, 31, (1,), generator=g))]
             .tolist() for u in range(U)}
    seen, rows = _seen(lists, U, I)
    shards = [torch.arange(r, I, W) if strided else shard_items(I, W, r) for r in range(W)]
    whole = ItemIndex(m, projection=proj)
    parts = [ItemIndex(m, items=sh, projection=proj) for sh in shards]
    for r in range(W):
        assert torch.equal(parts[r].hour_bias(hour), whole.hour_bias(hour)[shards[r].to(DEV)])
    for ex in (None, seen):
        ref_s, ref_i = score_topk(m, users, k=k, index=whole, exclude=ex, hour=hour)
        ls, li = [], []
        for r in range(W):
            s, i = score_topk(m, users, k=k, index=parts[r], exclude=ex, hour=hour)
            assert set(i.flatten().tolist()) <= set(shards[r].tolist())
            ls.append(s)
            li.append(i)
        gs, gi = merge_topk(torch.cat(ls, 1), torch.cat(li, 1), k)
        assert torch.equal(gs, ref_s)
        diff = gi != ref_i    # identical ids except between exactly tied probabilities
        if diff.any():
            assert bool((gs[diff] == ref_s[diff]).all())
        if ex is not None:
            for row, u in enumerate(users.tolist()):
                assert not set(gi[row].tolist()) & set(rows[u])
    # the single-process form of the sharded entry point (W = 1), eager and graphed
    ref_s, ref_i = score_topk(m, users, k=k, index=whole, hour=hour)
    for graph in (False, True):
        s, i = scoring.sharded_score_topk(m, users.to(DEV), k, index=whole, graph=graph,
                                          hour=hour)
        assert torch.equal(s, ref_s) and torch.equal(i, ref_i)
    keys = list(whole._graphed)
    assert len(keys) == 1 and keys[0][-1] == "hour"
    scoring.sharded_score_topk(m, users.to(DEV), k, index=whole, graph=True, hour=2)
    scoring.sharded_score_topk(m, users.to(DEV), k, index=whole, graph=True)
    assert len(whole._graphed) == 2          # one hour scorer for every hour, one without


# -------------------------------------------------------------------------- 9. invalidation
def test_hour_state_follows_the_weights():
    """In-place changes of the hour embedding, then of the projection: the index is stale, the
    results follow the new weights (against the oracle) and the cached hour biases are rebuilt."""
    U, I, k, hour = 80, 3001, 10, 5
    m = _model(U, I, 61, 64, 64, 32)
    proj = _proj(32, 64, 54)
    users = torch.arange(0, U, 8)
    idx = ItemIndex(m, projection=proj)
    sc = GraphedScorer(m, users.numel(), k, index=idx, hour=hour)
    s0, i0 = score_topk(m, users, k=k, index=idx, hour=hour)
    _assert_vs_oracle(s0, i0, _Ref(m, proj, I)(users, hour), users, k)
    g = torch.Generator().manual_seed(62)
    changes = [lambda: m.temporal_encoding.hour_embed.weight.add_(
                   0.5 * torch.randn(24, 32, generator=g).to(DEV)),
               lambda: proj.weight.add_(0.2 * torch.randn(64, 32, generator=g).to(DEV)),
               lambda: proj.bias.mul_(-1.0)]
    prev_s = s0
    for change in changes:
        old_idx, old_bias = sc.index, sc.index.hour_bias(hour)
        assert old_idx.valid_for(m)
        with torch.no_grad():
            change()
        assert not old_idx.valid_for(m) and not idx.valid_for(m)
        s, it = score_topk(m, users, k=k, index=idx, hour=hour)     # a stale index is rebuilt
        ref = _Ref(m, proj, I)(users, hour)
        _assert_vs_oracle(s, it, ref, users, k)
        assert not torch.equal(s, prev_s)
        gs, gi = sc(users.to(DEV), hour=hour)
        assert torch.equal(gs, s) and torch.equal(gi, it)
        assert sc.index is not old_idx and sc.index.projection is proj
        assert hour in sc.index._hour_bias
        assert not torch.equal(sc.index.hour_bias(hour), old_bias)
        prev_s = s


# ------------------------------------------------------------------------------ 10. metrics
def _metrics_case():
    """No GPU: 60 users at an hour each (6 distinct), a held-out item each (for every other user
    one of the oracle's own top 10 at that hour, else a random item), histories of 0..30 items
    without it; the three sums from the oracle's ranking, and the smallest gap between a held-out
    item and the other scores of its user's top k + 1."""
    U, I, k, n = 100, 2003, 10, 60
    torch.manual_seed(73)
    m = ncf.AdvancedNCF(U, I, 5, 24, 64, 64, 64).eval()
    g = torch.Generator().manual_seed(74)
    users = torch.randperm(U, generator=g)[:n]
    hours = torch.tensor([0, 6, 9, 13, 18, 23])[torch.randint(0, 6, (n,), generator=g)]
    ref = _Ref(m, None, I)(users, hours)
    lists = {u: torch.randperm(I, generator=g)[:int(torch.randint(0, 31, (1,), generator=g))]
             .tolist() for u in range(U)}
    held = torch.randint(0, I, (n,), generator=g)
    for r in range(0, n, 2):
        row = ref[r].clone()
        row[lists[int(users[r])]] = float("-inf")
        held[r] = torch.argsort(-row, stable=True)[int(torch.randint(0, k, (1,), generator=g))]
    for u, h in zip(users.tolist(), held.tolist()):
        lists[u] = [x for x in lists[u] if x != h]
    rows = [sorted(set(lists[u])) for u in range(U)]
    hr = ndcg = mrr = 0.0
    margin = float("inf")
    for r, u in enumerate(users.tolist()):
        row = ref[r].clone()
        row[rows[u]] = float("-inf")
        order = torch.argsort(-row, stable=True)[:k + 1]
        h = int(held[r])
        near = (row[order] - row[h]).abs()
        margin = min(margin, float(near[order != h].min()))
        place = (order[:k] == h).nonzero().flatten()
        if place.numel():
            pl = int(place[0])
            hr += 1.0
            ndcg += 1.0 / np.log2(pl + 2.0)
            mrr += 1.0 / (pl + 1.0)
    want = {f"hr@{k}": hr / n, f"ndcg@{k}": ndcg / n, f"mrr@{k}": mrr / n}
    return m, users, hours, held, lists, want, margin, (U, I, k)


def test_full_ranking_metrics_at_hours():
    from ncf_amd.metrics import full_ranking_metrics
    m, users, hours, held, lists, want, margin, (U, I, k) = _metrics_case()
    # the seed's precondition (from the oracle alone): every held-out item is more than twice the
    # score tolerance away from the other scores of its user's top k + 1, so its place is the
    # oracle's (seed 73: 1.9e-4)
    assert margin > 2 * ATOL, margin
    assert 0.5 <= want[f"hr@{k}"] <= 0.6
    m = m.to(DEV)
    seen, _ = _seen(lists, U, I)
    got = full_ranking_metrics(m, users, held, k, exclude=seen, index=ItemIndex(m), hour=hours)
    assert set(got) == set(want)
    for name in want:
        assert got[name] == pytest.approx(want[name], abs=1e-9), name


# ---------------------------------------------------------------------------- 11. refusals
def test_refusals_leave_the_scorer_working(world):
    m, proj, idx, _ = world[32]
    users = world["users"]
    good = lambda: score_topk(m, users, 10, idx, hour=3)  # noqa: E731
    s0, i0 = good()

    def same():
        s, i = good()
        assert torch.equal(s, s0) and torch.equal(i, i0)

    # temporal_dim != mf_embedding_dim without a projection
    with pytest.raises(ValueError, match="fresh random projection"):
        score_topk(m, users, 10, hour=3)
    with pytest.raises(ValueError, match="fixed projection"):
        ItemIndex(m).at_hour(3)
    with pytest.raises(ValueError, match="projection"):
        GraphedScorer(m, 37, 10, hour=3)
    same()
    # mf_embedding_dim != mlp_embedding_dim, as forward_simple(hour)
    split = _model(50, 501, 81, 64, 32, 32)
    with pytest.raises(RuntimeError, match="temporal scale"):
        score_topk(split, torch.arange(5), 10, hour=3, projection=_proj(32, 64, 55))
    same()
    # an hour out of range inside a tensor raises after the run (the kernel's bit 2)
    for bad in (24, -1):
        hours = torch.full((37,), 3)
        hours[11] = bad
        with pytest.raises(IndexError, match="hour"):
            score_topk(m, users, 10, idx, hour=hours)
        with pytest.raises(IndexError, match="hour"):      # alone in a one-hour tensor as well
            score_topk(m, users[:1], 10, idx, hour=torch.tensor([bad]))
        same()
    bad_u = users.clone()
    bad_u[2] = U0
    with pytest.raises(IndexError, match="user id"):
        score_topk(m, bad_u, 10, idx, hour=3)
    same()


def test_zz_report_max_error():
    """The largest |score - oracle| the tests above measured (DESIGN §12 quotes it)."""
    if MAX_ERR:
        print(f"hour scoring: max |score - oracle| = {max(MAX_ERR):.3e} over {len(MAX_ERR)} rows")
        assert max(MAX_ERR) <= ATOL
