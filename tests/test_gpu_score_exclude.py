"""Top-k scoring that leaves out the items each user has already seen (``exclude=SeenItems``):
the select's exclusion (ncf_score_select with its exclusion arguments), the exact
re-run of users whose seen items reach into their top k, shards, the captured graph, and
metrics.full_ranking_metrics.  Runs on a real MI355X only (marker ``gpu``).

Reference: the oracle's score_factorised in float64 with the seen items at -inf, ordered by
(score desc, item id asc); items identical except between oracle scores tied within 1e-6, scores
within 1e-6 (as test_gpu_parity.test_score_topk_vs_oracle); membership in a history is exact."""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import scoring  # noqa: E402
from ncf_amd.scoring import (GraphedScorer, ItemIndex, SeenItems, merge_topk,  # noqa: E402
                             score_topk, shard_items)
DEV = torch.device("cuda:0")


def _model(U, I, seed, *more):
    torch.manual_seed(seed)
    return ncf.AdvancedNCF(U, I, 5, 24, *more).to(DEV).eval()


def _oracle(m, users, I):
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    return O.score_factorised(p, users.cpu(), torch.arange(I), temporal_dim=32, n_layers=3)


def _seen(lists, U, I):
    """SeenItems on the device from {user id: iterable of item ids}."""
    rows = [sorted(set(int(x) for x in lists.get(u, ()))) for u in range(U)]
    off = np.zeros(U + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    items = np.array([x for r in rows for x in r], dtype=np.int32)
    return SeenItems.from_csr(torch.from_numpy(off), torch.from_numpy(items), I).to(DEV), rows


def _random_lists(U, I, longest, gen, none=()):
    lists = {}
    for u in range(U):
        n = 0 if u in none else int(torch.randint(0, longest + 1, (1,), generator=gen))
        lists[u] = torch.randperm(I, generator=gen)[:n].tolist()
    return lists


def _assert_vs_oracle(s, it, ref, users, rows, k):
    for r, u in enumerate(users.tolist()):
        row = ref[r].clone()
        if rows[u]:
            row[rows[u]] = float("-inf")
        order = torch.argsort(-row, stable=True)[:k].tolist()
        got = it[r].cpu().tolist()
        assert not set(got) & set(rows[u]), (r, u)           # exact: nothing seen comes back
        assert min(got) >= 0 and len(set(got)) == k
        if got != order:    # only between oracle scores tied within 1e-6
            np.testing.assert_allclose(ref[r, got].numpy(), ref[r, order].numpy(), atol=1e-6)
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, got].numpy(), atol=1e-6)


# ------------------------------------------------------------------- 1. against the oracle
@pytest.fixture(scope="module")
def vs_oracle():
    U, I = 300, 20011
    m = _model(U, I, 3)
    g = torch.Generator().manual_seed(17)
    users = torch.randint(0, U, (37,), generator=g)
    uniq = list(dict.fromkeys(users.tolist()))
    none = set(uniq[:5])
    lists = _random_lists(U, I, 50, g, none=none)
    idx = ItemIndex(m)
    # one user has seen exactly the threshold sample's items (every stride-th of the catalogue
    # under the default plan), one its own unfiltered top 50
    plan = scoring._TopKRun(idx, 37, 10, 8192)
    assert plan.stride > 1
    u_sample, u_top = uniq[5], uniq[6]
    lists[u_sample] = list(range(0, plan.S * plan.stride, plan.stride))
    _, top = score_topk(m, torch.tensor([u_top]), k=50, index=idx)
    lists[u_top] = top[0].cpu().tolist()
    seen, rows = _seen(lists, U, I)
    assert sum(1 for u in uniq if not rows[u]) >= 5
    return m, idx, users, seen, rows, _oracle(m, users, I)


@pytest.mark.parametrize("k,cap", [(1, 8192), (10, 8192), (100, 8192), (100, 128)])
def test_exclude_vs_oracle(vs_oracle, k, cap):
    """Histories of 0..50 random items (five users without), one user who has seen the whole
    threshold sample, one who has seen its own top 50; cap = 128 overflows and, with the top 50
    gone, needs longer candidate lists than the call's in the re-run."""
    m, idx, users, seen, rows, ref = vs_oracle
    s, it = score_topk(m, users, k=k, index=idx, cap=cap, exclude=seen)
    _assert_vs_oracle(s, it, ref, users, rows, k)


# ------------------------------------------------------------ 2. self-consistency, bit for bit
def _count_safe(monkeypatch):
    calls = []
    safe = scoring._TopKRun.safe_thresholds

    def counted(self, redo, st, **kw):
        calls.append(int(redo.numel()))
        return safe(self, redo, st, **kw)
    monkeypatch.setattr(scoring._TopKRun, "safe_thresholds", counted)
    return calls


def _top_e_seen(full_items, users, E, U, I):
    lists = {}
    for r, u in enumerate(users.tolist()):
        lists[u] = full_items[r, :E].cpu().tolist()
    return _seen(lists, U, I)[0]


@pytest.mark.parametrize("mode", ["terms1", "terms2", "fp32select"])
@pytest.mark.parametrize("E", [5, 64])
def test_exclude_own_top_items_bitwise(E, mode, monkeypatch):
    """The history is exactly the user's best E items (what a trained model's history looks
    like): the result must be places E .. E + k of the unfiltered ranking, the same items and
    score bits.  The first pass's threshold (the sample's 10th of 4096 sampled items, ~50 items
    of the catalogue above it) still covers place 15 (E = 5: nobody is re-run) but not place 74
    (E = 64: every user fails the select's check and is re-run from the sample's rank k + E);
    a re-scoring window derived before the exclusion would sit at the seen items' logits and
    drop the answers.

    (The catalogue items above the sample's 10th number ~49 +- 15, so about one user in 20 keeps
    74 of them: the users are drawn with a seed under which all 37 do not, and none keeps fewer
    than 15.  That precondition is asserted from the first pass's own thresholds.)"""
    U, I, k = 300, 20011, 10
    m = _model(U, I, 7)
    users = torch.randperm(U, generator=torch.Generator().manual_seed(12))[:37]
    idx = ItemIndex(m)
    if mode == "fp32select":
        idx.pmax = None          # the three-term scan, then the select without re-scoring
    else:
        idx.terms = int(mode[-1])
    full_s, full_i = score_topk(m, users, k=E + k, index=idx)
    seen = _top_e_seen(full_i, users, E, U, I)
    calls = _count_safe(monkeypatch)
    runs = []
    launch = scoring._TopKRun.launch

    def recorded(self, model, st):
        runs.append(self)
        return launch(self, model, st)
    monkeypatch.setattr(scoring._TopKRun, "launch", recorded)
    s, it = score_topk(m, users, k=k, index=idx, exclude=seen)
    print(f"E={E} {mode}: safe_thresholds over {calls} of {len(users)} users")
    assert torch.equal(it, full_i[:, E:])
    assert torch.equal(s, full_s[:, E:])
    # the k-th unseen item (place E + k of the whole ranking) against the checked threshold
    below = full_s[:, E + k - 1].double() < torch.sigmoid(runs[0].thr_chk[:len(users)].double())
    if E == 5:
        assert not bool(below.any()), "precondition: the first pass covers place 15"
        assert not calls, calls
    else:
        assert bool(below.all()), "precondition: place 74 is below every user's threshold"
        assert calls == [len(users)], calls


def test_exclude_own_top_items_bitwise_rank_j(monkeypatch):
    """The same under the rank-j plan (the threshold is the sample's 16th, checked by the select
    anyway): k = 100, the best 64 seen."""
    U, I, k, E = 2000, 100003, 100, 64
    m = _model(U, I, 23)
    users = torch.randperm(U, generator=torch.Generator().manual_seed(4))[:64]
    idx = ItemIndex(m)
    monkeypatch.setattr(scoring, "SAMPLE_MIN", 256)
    monkeypatch.setattr(scoring, "RANK_J", 16)
    full_s, full_i = score_topk(m, users, k=E + k, index=idx)
    seen = _top_e_seen(full_i, users, E, U, I)
    assert scoring._TopKRun(idx, len(users), k, 8192, exclude=seen).j == 16
    s, it = score_topk(m, users, k=k, index=idx, exclude=seen)
    assert torch.equal(it, full_i[:, E:])
    assert torch.equal(s, full_s[:, E:])


# ----------------------------------------------------------------------------------- 3. ties
def test_exclude_inside_a_tie_group():
    """The catalogue of test_score_topk_exact_ties_by_item_id (all but the last 10 items share
    one row): with tied ids 0, 1, 2, 5 and the user's best distinct item seen, the list is the
    other distinct items above the tie, then tied ids 3, 4, 6, 7, ... ascending."""
    U, I, k, distinct = 60, 3000, 10, 10
    m = _model(U, I, 21)
    with torch.no_grad():
        for t in m.parameters():
            if t.dim() == 2 and t.shape[0] == I:     # the item tables
                t[:I - distinct] = t[0]
    users = torch.arange(0, U, 3)
    ref = _oracle(m, users, I)
    lists, want = {}, []
    for r, u in enumerate(users.tolist()):
        tie = ref[r, 0].item()
        others = sorted(((ref[r, j].item(), j) for j in range(I - distinct, I)), reverse=True)
        assert all(abs(v - tie) > 1e-5 for v, _ in others)   # (no near-tie with the group)
        assert all(abs(a[0] - b[0]) > 1e-6 for a, b in zip(others, others[1:]))
        best = others[0][1]
        lists[u] = [0, 1, 2, 5, best]
        above = [j for v, j in others[1:] if v > tie]
        tied = [j for j in range(I - distinct) if j not in (0, 1, 2, 5)]
        want.append((above + tied)[:k])
    seen, _ = _seen(lists, U, I)
    s, it = score_topk(m, users, k=k, exclude=seen)
    assert it.cpu().tolist() == want
    for r in range(len(users)):
        np.testing.assert_allclose(s[r].cpu().numpy(), ref[r, want[r]].numpy(), atol=1e-6)


# ------------------------------------------------------------ 4. nothing excluded is a no-op
@pytest.mark.parametrize("k", [10, 100])
def test_empty_lists_change_nothing(k):
    U, I = 300, 20011
    m = _model(U, I, 3)
    users = torch.randint(0, U, (37,), generator=torch.Generator().manual_seed(1))
    idx = ItemIndex(m)
    seen = SeenItems(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                     U, I).to(DEV)
    assert seen.items.numel() == 0
    s0, i0 = score_topk(m, users, k=k, index=idx)
    s1, i1 = score_topk(m, users, k=k, index=idx, exclude=seen)
    assert torch.equal(i0, i1) and torch.equal(s0, s1)


# ------------------------------------------------------------------- 5. fewer than k left
def test_fewer_than_k_unseen_items():
    U, I, k = 20, 64, 10
    m = _model(U, I, 31)
    users = torch.arange(U)
    idx = ItemIndex(m)
    full_s, full_i = score_topk(m, users, k=I, index=idx)
    base_s, base_i = score_topk(m, users, k=k, index=idx)
    left = [7, 20, 63]
    seen, _ = _seen({4: [j for j in range(I) if j not in left], 11: range(I)}, U, I)
    s, it = score_topk(m, users, k=k, index=idx, exclude=seen)
    keep = torch.isin(full_i[4], torch.tensor(left, device=DEV))
    assert it[4, :3].tolist() == full_i[4][keep].tolist()
    assert torch.equal(s[4, :3], full_s[4][keep])
    assert it[4, 3:].tolist() == [-1] * 7 and s[4, 3:].tolist() == [0.0] * 7
    assert it[11].tolist() == [-1] * k and s[11].tolist() == [0.0] * k
    others = [u for u in range(U) if u not in (4, 11)]
    assert torch.equal(it[others], base_i[others]) and torch.equal(s[others], base_s[others])


# ------------------------------------------------------------------ 6. subset index and shards
@pytest.mark.parametrize("W,strided", [(4, True), (3, False)])
def test_exclude_on_item_shards(W, strided):
    """Histories are global ids; an ItemIndex over a subset maps its positions back before the
    lookup.  The shards' lists merged == the single index's list; one user has seen all but two
    items of shard 0, whose list there ends in empty slots that stay -1."""
    U, I, k = 200, 5003, 10
    m = _model(U, I, 5)
    g = torch.Generator().manual_seed(6)
    users = torch.randint(0, U, (45,), generator=g)
    lists = _random_lists(U, I, 30, g)
    shards = [torch.arange(r, I, W) if strided else shard_items(I, W, r) for r in range(W)]
    u0 = int(users[0])
    last2 = shards[0][-2:].tolist()
    lists[u0] = shards[0][:-2].tolist() + [x for x in lists[u0] if x not in last2]
    seen, rows = _seen(lists, U, I)
    ref_s, ref_i = score_topk(m, users, k=k, exclude=seen)
    ls, li = [], []
    for r in range(W):
        s, i = score_topk(m, users, k=k, index=ItemIndex(m, items=shards[r]), exclude=seen)
        mine = set(shards[r].tolist())
        for row, u in enumerate(users.tolist()):
            got = [x for x in i[row].tolist() if x >= 0]
            assert set(got) <= mine and not set(got) & set(rows[u]), (r, row)
        if r == 0:
            for row in (users == u0).nonzero().flatten().tolist():
                assert sorted(i[row, :2].tolist()) == last2
                assert i[row, 2:].tolist() == [-1] * (k - 2)
                assert s[row, 2:].tolist() == [0.0] * (k - 2)
        ls.append(s)
        li.append(i)
    gs, gi = merge_topk(torch.cat(ls, 1), torch.cat(li, 1), k)
    assert torch.equal(gs, ref_s)
    diff = gi != ref_i    # identical ids except between exactly tied probabilities
    if diff.any():
        assert bool((gs[diff] == ref_s[diff]).all())


# ---------------------------------------------------------------------------------- 7. graph
@pytest.mark.parametrize("k,cap,shard", [(10, 8192, False), (100, 128, False), (10, 8192, True)])
def test_graphed_scorer_with_exclude(k, cap, shard):
    """The captured pipeline looks the lists up by user id, so one graph serves any users; users
    who have seen their own best items take the eager re-run after the replay; a parameter change
    re-captures; an id out of range raises IndexError (no list is read for it) and the scorer
    goes on working."""
    U, I = 300, 20011
    m = _model(U, I, 9)
    g = torch.Generator().manual_seed(10)
    lists = _random_lists(U, I, 50, g, none=set(range(0, U, 10)))
    _, top = score_topk(m, torch.arange(40), k=30)
    for u in range(40):
        if u % 10:
            lists[u] = top[u].cpu().tolist()
    seen, rows = _seen(lists, U, I)
    ids = shard_items(I, 3, 1) if shard else None
    idx = ItemIndex(m, items=ids) if shard else None
    sc = GraphedScorer(m, 37, k=k, index=idx, cap=cap, exclude=seen)
    for rep in range(3):
        users = torch.randint(0, 60 if rep == 0 else U, (37,), generator=g).to(DEV)
        gs, gi = sc(users)
        es, ei = score_topk(m, users, k=k, index=idx, cap=cap, exclude=seen)
        assert torch.equal(gs, es) and torch.equal(gi, ei), rep
        for row, u in enumerate(users.tolist()):
            assert not set(gi[row].tolist()) & set(rows[u])
    with torch.no_grad():
        m.final[0].bias.add_(0.25)
    users = torch.randint(0, U, (37,), generator=g).to(DEV)
    gs, gi = sc(users)
    es, ei = score_topk(m, users, k=k, index=ItemIndex(m, items=ids) if shard else None, cap=cap,
                        exclude=seen)
    assert torch.equal(gs, es) and torch.equal(gi, ei)
    bad = users.clone()
    bad[3], bad[20] = U, -1
    with pytest.raises(IndexError):
        sc(bad)
    with pytest.raises(IndexError):
        score_topk(m, bad, k=k, cap=cap, exclude=seen)
    gs2, gi2 = sc(users)
    assert torch.equal(gs2, gs) and torch.equal(gi2, gi)


# --------------------------------------------------------------------------------- 8. D = 128
def test_exclude_d128_vs_oracle():
    """The fp32 scan and the select without re-scoring (exclusion only): histories of
    0..20 random items, and every fourth user has seen its own top 10."""
    U, I, k = 64, 3001, 10
    m = _model(U, I, 41, 128, 128, 32, [256, 128, 64], 4, 0.2, 4)
    users = torch.arange(U)
    idx = ItemIndex(m)
    assert idx.p.shape[1] == 128 and idx.p3 is None and idx.pmax is None
    g = torch.Generator().manual_seed(42)
    lists = _random_lists(U, I, 20, g, none={1, 2, 3})
    _, top = score_topk(m, users, k=k, index=idx)
    for u in range(0, U, 4):
        lists[u] = top[u].cpu().tolist()
    seen, rows = _seen(lists, U, I)
    s, it = score_topk(m, users, k=k, index=idx, exclude=seen)
    _assert_vs_oracle(s, it, _oracle(m, users, I), users, rows, k)


# -------------------------------------------------------------------- 9. full_ranking_metrics
METRICS_SEED = 13


def _metrics_case(seed=METRICS_SEED):
    """The metrics test's data and its float64 reference (no GPU): 100 users, a held-out item
    each, histories of 0..30 items without it; for half of the users the held-out item is one
    of five items whose bias is raised by 3, which puts them in everybody's top 10."""
    U, I, k, n = 300, 5003, 10, 100
    torch.manual_seed(seed)
    m = ncf.AdvancedNCF(U, I, 5, 24).eval()
    g = torch.Generator().manual_seed(seed + 1)
    users = torch.randperm(U, generator=g)[:n]
    boosted = torch.randperm(I, generator=g)[:5]
    held = torch.randint(0, I, (n,), generator=g)
    held[::2] = boosted[torch.randint(0, 5, (n // 2,), generator=g)]
    lists = _random_lists(U, I, 30, g)
    for u, h in zip(users.tolist(), held.tolist()):
        lists[u] = [x for x in lists[u] if x != h]
    rows = [sorted(set(lists[u])) for u in range(U)]
    p = {kk: v.detach().double() for kk, v in m.state_dict().items()}
    prob = O.score_factorised(p, users, torch.arange(I), temporal_dim=32, n_layers=3)
    logit = torch.logit(prob)
    logit[:, boosted] += 3.0
    score = torch.sigmoid(logit)
    hr = ndcg = mrr = 0.0
    margin = float("inf")
    for r, u in enumerate(users.tolist()):
        row = score[r].clone()
        row[rows[u]] = float("-inf")
        order = torch.argsort(-row, stable=True)[:k + 1]
        h = int(held[r])
        # the held-out item against every other score of the top k + 1 (the k-th among them)
        near = (row[order] - row[h]).abs()
        margin = min(margin, float(near[order != h].min()))
        place = (order[:k] == h).nonzero().flatten()
        if place.numel():
            pl = int(place[0])
            hr += 1.0
            ndcg += 1.0 / np.log2(pl + 2.0)
            mrr += 1.0 / (pl + 1.0)
    want = {f"hr@{k}": hr / n, f"ndcg@{k}": ndcg / n, f"mrr@{k}": mrr / n}
    return m, users, held, boosted, lists, want, margin, (U, I, k)


def test_full_ranking_metrics_vs_oracle():
    from ncf_amd.metrics import full_ranking_metrics
    m, users, held, boosted, lists, want, margin, (U, I, k) = _metrics_case()
    # the seed's precondition: no held-out item within 1e-6 of its user's k-th oracle score (nor
    # of any other of the top k + 1, so its place is the oracle's too)
    assert margin > 1e-6, margin
    assert 0.45 <= want[f"hr@{k}"] <= 0.6
    m = m.to(DEV)
    idx = ItemIndex(m)
    idx.bias[boosted.to(DEV)] += 3.0
    seen, _ = _seen(lists, U, I)
    got = full_ranking_metrics(m, users, held, k, exclude=seen, index=idx)
    assert set(got) == set(want)
    for name in want:
        assert got[name] == pytest.approx(want[name], abs=1e-9), name
    lists[int(users[7])] = lists[int(users[7])] + [int(held[7])]
    with pytest.raises(ValueError):
        full_ranking_metrics(m, users, held, k, exclude=_seen(lists, U, I)[0], index=idx)


# ------------------------------------------------------------ 10. DeviceNegativeSampler.seen()
def test_sampler_seen_shares_storage():
    from ncf_amd.data import DeviceNegativeSampler
    U, I, k = 120, 2003, 10
    m = _model(U, I, 15)
    g = torch.Generator().manual_seed(16)
    iu = torch.randint(0, U, (3000,), generator=g)
    ip = torch.randint(0, I, (3000,), generator=g)
    sampler = DeviceNegativeSampler(iu, ip, U, I, device=DEV)
    seen = sampler.seen()
    assert seen.offsets.data_ptr() == sampler.hist_offsets.data_ptr()
    assert seen.items.data_ptr() == sampler.hist_items.data_ptr()
    assert seen.num_users == U and seen.num_products == I
    built = SeenItems(iu, ip, U, I).to(DEV)
    assert torch.equal(built.offsets, seen.offsets) and torch.equal(built.items, seen.items)
    users = torch.arange(U)
    idx = ItemIndex(m)
    s0, i0 = score_topk(m, users, k=k, index=idx, exclude=seen)
    s1, i1 = score_topk(m, users, k=k, index=idx, exclude=built)
    assert torch.equal(s0, s1) and torch.equal(i0, i1)
    assert not bool(seen.contains(users.repeat_interleave(k), i0.reshape(-1)).any())


# ------------------------------------------- 11. an overflowed list that lost its k candidates
def test_select_excl_overflow_flags_at_the_c_abi():
    """ncf_score_select (exclusion) on hand-made lists that overflowed (count > cap = 16, K = 4): with
    two seen items the 4th remaining logit comes back as the re-run's threshold (flag 1); with 14
    seen only two candidates remain, which bound nothing: flag 2, the threshold untouched."""
    from ncf_amd import _lib
    from ncf_amd._lib import ptr
    cap, K = 16, 4
    logit = torch.arange(16, 0, -1, dtype=torch.float32)                 # item j: 16 - j
    cand = torch.stack([logit.view(torch.int32), torch.arange(16, dtype=torch.int32)], 1)
    cand = cand.unsqueeze(0).repeat(2, 1, 1).contiguous().to(DEV)         # [2, cap, (logit, item)]
    count = torch.tensor([21, 21], dtype=torch.int32, device=DEV)
    seen, _ = _seen({0: [0, 1], 1: range(14)}, 2, 16)
    uid = torch.tensor([0, 1], device=DEV)
    thr = torch.full((2,), 123.0, device=DEV)
    out_s = torch.empty(2, K, device=DEV)
    out_i = torch.empty(2, K, dtype=torch.int64, device=DEV)
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ncf_score_select", None, 2, ptr(count), ptr(cand), cap, K, None, None, None, 0,
              None, 0.0, ptr(out_s), ptr(out_i), ptr(thr), ptr(flag), None, ptr(uid), 2,
              ptr(seen.offsets), ptr(seen.items), None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert flag.tolist() == [1, 2]
    assert thr.tolist() == [11.0, 123.0]
    assert out_i.tolist() == [[2, 3, 4, 5], [14, 15, -1, -1]]
    want = torch.sigmoid(torch.tensor([14.0, 13.0, 12.0, 11.0]))
    torch.testing.assert_close(out_s[0].cpu(), want, rtol=0, atol=1e-6)
    assert out_s[1, 2:].tolist() == [0.0, 0.0]


def test_overflow_that_loses_its_candidates_is_rerun(monkeypatch):
    """k = 100, cap = 128, the best 50 seen, and the first pass's thresholds lowered to each
    user's 250th logit (two-term scan: its margin adds next to nothing): every list overflows,
    and the 128 records kept of ~250 hold 102 +- 5 unseen ones: fewer than 100 for about a third
    of the users (no valid threshold: re-run from the sample's rank k + e in longer lists), 100
    for the others (their 100th is the next threshold).  Places 50 .. 150 of the unfiltered
    ranking either way, the same bits."""
    U, I, k, E, cap = 300, 20011, 100, 50, 128
    m = _model(U, I, 7)
    users = torch.randperm(U, generator=torch.Generator().manual_seed(12))[:37]
    idx = ItemIndex(m)
    idx.terms = 2
    full_s, full_i = score_topk(m, users, k=300, index=idx)
    seen = _top_e_seen(full_i, users, E, U, I)
    low = torch.logit(full_s[:, 249].double()).float()
    runs, launch, collect = [], scoring._TopKRun.launch, scoring._collect

    def recorded(self, model, st):
        runs.append(self)
        return launch(self, model, st)

    def lowered(*a, **kw):
        if len(runs) == 1 and not hasattr(runs[0], "lowered"):
            runs[0].lowered = True
            runs[0].thr[:len(users)] = low
        return collect(*a, **kw)
    monkeypatch.setattr(scoring._TopKRun, "launch", recorded)
    monkeypatch.setattr(scoring, "_collect", lowered)
    calls = _count_safe(monkeypatch)
    s, it = score_topk(m, users, k=k, index=idx, cap=cap, exclude=seen)
    print(f"lost lists re-run from the safe threshold: {calls} of {len(users)} users")
    assert runs[0].lowered and calls, "some list lost its k candidates"
    assert torch.equal(it, full_i[:, E:E + k])
    assert torch.equal(s, full_s[:, E:E + k])
