"""CPU-only checks of hour-of-day scoring's host side (``hour=`` / ``projection=`` on the scoring
entry points, the grouping of users by hour, the declared entry point); the kernel and the
pipeline are tested in test_gpu_score_hour.py."""
import inspect
import types

import pytest
import torch

import _ncf_pkg

ncf = _ncf_pkg.load()
from ncf_amd import _lib, metrics, scoring  # noqa: E402


def test_hour_and_projection_are_keyword_only():
    for fn in (scoring.score_topk, scoring.GraphedScorer.__init__, scoring.sharded_score_topk):
        params = inspect.signature(fn).parameters
        for name in ("hour", "projection"):
            p = params[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, (fn, name)
        names = list(params)
        assert names.index("exclude") < names.index("hour") < names.index("projection")
    p = inspect.signature(scoring.ItemIndex.__init__).parameters["projection"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert list(inspect.signature(scoring.ItemIndex.__init__).parameters)[:4] == \
        ["self", "model", "chunk", "items"]
    p = inspect.signature(scoring.GraphedScorer.__call__).parameters
    assert list(p)[:3] == ["self", "user_ids", "copy"]
    assert p["hour"].kind is inspect.Parameter.KEYWORD_ONLY and p["hour"].default is None
    p = inspect.signature(metrics.full_ranking_metrics).parameters
    assert list(p)[:6] == ["model", "users", "heldout_items", "k", "exclude", "index"]
    assert p["hour"].default is None


def test_pinned_positions_still_hold():
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(scoring._TopKRun.__init__) == ["self", "index", "n", "k", "cap", "exclude"]
    assert sig(scoring._TopKRun.safe_thresholds)[:3] == ["self", "redo", "st"]
    assert sig(scoring._collect)[-2:] == ["expected", "terms"]
    assert sig(scoring.score_topk)[:5] == ["model", "user_ids", "k", "index", "cap"]
    assert sig(scoring._select)[-3:] == ["terms", "check", "exclude"]


def test_entry_point_is_declared():
    assert "ncf_score_queries_hour" in _lib.SIGNATURES
    # ncf_score_queries' 13 arguments + hours + scale
    assert len(_lib.SIGNATURES["ncf_score_queries_hour"][1]) == 15
    assert len(_lib.SIGNATURES["ncf_score_queries"][1]) == 13
    assert len(_lib.SIGNATURES["ncf_score_item_bias"][1]) == 7


def _groups(hours):
    return [(h, pos.tolist()) for h, pos in scoring.group_by_hour(hours)]


def test_group_by_hour_keeps_the_callers_order_within_a_group():
    hours = torch.tensor([13, 0, 13, 23, 0, 13, 5, 13])
    assert _groups(hours) == [(0, [1, 4]), (5, [6]), (13, [0, 2, 5, 7]), (23, [3])]
    for h, pos in scoring.group_by_hour(hours):
        assert pos.dtype == torch.int64 and bool((hours[pos] == h).all())


def test_group_by_hour_groups_of_one_and_one_group():
    assert _groups(torch.tensor([4, 2, 9])) == [(2, [1]), (4, [0]), (9, [2])]
    assert _groups(torch.tensor([7, 7, 7])) == [(7, [0, 1, 2])]
    assert _groups(torch.tensor([11])) == [(11, [0])]
    # values the kernel would refuse are grouped like any other (they raise after the run)
    assert _groups(torch.tensor([24, -1, 24], dtype=torch.int32)) == [(-1, [1]), (24, [0, 2])]


def test_group_by_hour_empty():
    assert scoring.group_by_hour(torch.zeros(0, dtype=torch.int64)) == []


def test_group_by_hour_random_is_a_stable_partition():
    g = torch.Generator().manual_seed(3)
    hours = torch.randint(0, 24, (500,), generator=g)
    groups = scoring.group_by_hour(hours)
    assert [h for h, _ in groups] == sorted(set(hours.tolist()))
    allpos = torch.cat([pos for _, pos in groups])
    assert sorted(allpos.tolist()) == list(range(500))
    for h, pos in groups:
        assert pos.tolist() == sorted(pos.tolist())
        assert bool((hours[pos] == h).all())


def test_bad_hours_raise_before_any_device_call():
    """A stand-in model without any tensor: the checks are reached before an index is built."""
    model = types.SimpleNamespace(num_users=6, num_products=8)
    users = torch.tensor([0, 1, 2])
    for bad in (24, -1):
        with pytest.raises(IndexError, match="hour"):
            scoring.score_topk(model, users, 3, hour=bad)
        with pytest.raises(IndexError, match="hour"):
            scoring.GraphedScorer(model, 3, 3, hour=bad)
        with pytest.raises(IndexError, match="hour"):
            scoring.sharded_score_topk(model, users, 3, hour=bad)
    for bad in (torch.tensor([1, 2]), torch.tensor([1, 2, 3, 4]), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="hour"):
            scoring.score_topk(model, users, 3, hour=bad)
    with pytest.raises(ValueError, match="score_topk"):      # mixed hours: not the graph's
        scoring.GraphedScorer(model, 3, 3, hour=torch.tensor([1, 2, 1]))
    with pytest.raises(TypeError):
        scoring.score_topk(model, users, 3, hour=1.5)
    with pytest.raises(TypeError):
        scoring.score_topk(model, users, 3, hour=torch.tensor([1.0, 2.0, 3.0]))
    # a good hour gets past the check and only then needs the model
    with pytest.raises(AttributeError):
        scoring.score_topk(model, users, 3, hour=23)
    with pytest.raises(AttributeError):
        scoring.score_topk(model, users, 3, hour=torch.tensor([0, 23, 5]))
