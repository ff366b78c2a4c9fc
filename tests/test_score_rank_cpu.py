"""CPU-only checks of the exact-rank feature (scoring.score_rank, csrc/rank.hip): the float64
reference of the contract on hand-made cases, the argument validation (which runs before any
launch and needs no GPU), and the new C-ABI entry points in the ctypes table and the header."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ncf_pkg
from tests import rank_ref as R

ncf = _ncf_pkg.load()
from ncf_amd import _lib, metrics, scoring  # noqa: E402
from ncf_amd.scoring import SeenItems  # noqa: E402

ENTRY_POINTS = ("ncf_rank_pair_logits", "ncf_rank_scan", "ncf_rank_seen_correct")


# ---- the reference itself

def test_ref_ties_go_by_item_id():
    #            0    1    2    3    4    5
    s = [[1.0, 3.0, 2.0, 2.0, 2.0, 0.5]]
    assert R.places(s, [2]).tolist() == [1]      # only item 1 is ahead
    assert R.places(s, [3]).tolist() == [2]      # item 1, and item 2 by its lower id
    assert R.places(s, [4]).tolist() == [3]
    assert R.places(s, [1]).tolist() == [0]
    assert R.places(s, [5]).tolist() == [5]


def test_ref_seen_item_ahead_and_tied():
    s = [[1.0, 3.0, 2.0, 2.0, 2.0, 0.5]]
    assert R.places(s, [4], [[1]]).tolist() == [2]       # a seen item ahead leaves the count
    assert R.places(s, [4], [[2]]).tolist() == [2]       # so does a seen item tied at a lower id
    assert R.places(s, [2], [[3, 4]]).tolist() == [1]    # tied at a higher id: never counted
    assert R.places(s, [4], [[5]]).tolist() == [3]       # a seen item behind changes nothing
    assert R.places(s, [4], [[1, 2, 3]]).tolist() == [0]
    assert R.places(s, [4], [[]]).tolist() == [3]


def test_ref_self_never_counted():
    s = np.zeros((3, 7))                                 # everything ties with everything
    held = [0, 3, 6]
    assert R.places(s, held).tolist() == [0, 3, 6]
    assert not R.beats(1.0, 4, 1.0, 4)
    assert not R.beats(2.0, 4, 1.0, 4)                   # (the j != h guard)
    assert R.beats(2.0, 5, 1.0, 4) and R.beats(1.0, 3, 1.0, 4) and not R.beats(1.0, 5, 1.0, 4)


def test_ref_vectorised_matches_literal():
    rng = np.random.default_rng(0)
    s = rng.integers(-3, 4, (9, 41)).astype(np.float64)  # many ties
    held = rng.integers(0, 41, 9)
    seen = [sorted(set(rng.integers(0, 41, rng.integers(0, 12)).tolist()) - {int(h)})
            for h in held]
    assert R.places(s, held).tolist() == R.places_literal(s, held).tolist()
    assert R.places(s, held, seen).tolist() == R.places_literal(s, held, seen).tolist()


# ---- argument validation (no launch, no GPU)

U, I = 6, 11


def _seen():
    return SeenItems(torch.tensor([0, 0, 2, 5]), torch.tensor([3, 7, 1, 10]), U, I)


def test_check_rank_accepts_good_arguments():
    users, held = torch.tensor([0, 2, 4, 0]), torch.tensor([4, 2, 10, 0])
    scoring._check_rank(users, held, I)
    scoring._check_rank(users, held, I, _seen(), SimpleNamespace(ids=None))
    scoring._check_rank(users[:0], held[:0], I, _seen())


def test_check_rank_length_mismatch():
    with pytest.raises(ValueError, match="one held-out item per user"):
        scoring._check_rank(torch.tensor([0, 1, 2]), torch.tensor([1, 2]), I)


@pytest.mark.parametrize("bad", [-1, I, 2 ** 40])
def test_check_rank_item_out_of_range(bad):
    with pytest.raises(IndexError, match="item id out of range"):
        scoring._check_rank(torch.tensor([0, 1]), torch.tensor([1, bad]), I)


def test_check_rank_heldout_in_history():
    with pytest.raises(ValueError, match="in its user's history"):
        scoring._check_rank(torch.tensor([1, 0]), torch.tensor([3, 7]), I, _seen())
    scoring._check_rank(torch.tensor([1, 0]), torch.tensor([7, 4]), I, _seen())   # another user's


def test_check_rank_subset_index():
    with pytest.raises(ValueError, match="subset of the catalogue"):
        scoring._check_rank(torch.tensor([0]), torch.tensor([1]), I, None,
                            SimpleNamespace(ids=torch.arange(5)))


def test_score_rank_validates_before_it_needs_a_gpu():
    """The public functions run the checks first: on a machine without a GPU the bad arguments
    raise their own errors, not the missing device's."""
    model = SimpleNamespace(num_users=U, num_products=I)
    with pytest.raises(ValueError, match="one held-out item per user"):
        scoring.score_rank(model, torch.tensor([0, 1]), torch.tensor([1]))
    with pytest.raises(IndexError, match="item id out of range"):
        scoring.score_rank(model, torch.tensor([0]), torch.tensor([I]))
    with pytest.raises(ValueError, match="in its user's history"):
        scoring.score_rank(model, torch.tensor([2]), torch.tensor([1]), exclude=_seen())
    with pytest.raises(ValueError, match="in its user's history"):
        metrics.ranking_report(model, torch.tensor([2]), torch.tensor([1]), exclude=_seen())
    with pytest.raises(IndexError, match="hour"):
        scoring.score_rank(model, torch.tensor([0]), torch.tensor([1]), hour=24)
    with pytest.raises(ValueError, match="hour holds"):
        scoring.score_rank(model, torch.tensor([0, 1]), torch.tensor([1, 2]),
                           hour=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="exclude covers"):
        scoring.score_rank(model, torch.tensor([0]), torch.tensor([1]),
                           exclude=SeenItems(torch.tensor([0]), torch.tensor([1]), U + 1, I))


def test_package_exports():
    assert ncf.score_rank is scoring.score_rank
    assert ncf.ranking_report is metrics.ranking_report


# ---- the C-ABI table and the header

def test_entry_points_in_table_and_header():
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} is not declared in include/ncf_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I32
        assert args[-1] is _lib.P      # the stream comes last
