"""CPU-only checks of the seen-item exclusion's host side (scoring.SeenItems and the ``exclude=``
argument's validation); the kernels are tested in test_gpu_score_exclude.py."""
import inspect
import types

import pytest
import torch

import _ncf_pkg

ncf = _ncf_pkg.load()
from ncf_amd import scoring  # noqa: E402
from ncf_amd.scoring import SeenItems  # noqa: E402


def _slices(seen):
    off = seen.offsets.tolist()
    it = seen.items.tolist()
    return [it[off[u]:off[u + 1]] for u in range(seen.num_users)]


def test_seen_items_from_interactions():
    """Duplicate interactions collapse, users without any get an empty slice, every slice is
    sorted and unique, and the offsets end at the number of items."""
    users = torch.tensor([3, 0, 3, 3, 5, 0, 3, 5])
    prods = torch.tensor([7, 2, 1, 7, 0, 2, 9, 8])
    seen = SeenItems(users, prods, 7, 10)
    assert seen.num_users == 7 and seen.num_products == 10
    assert seen.offsets.dtype == torch.int64 and seen.items.dtype == torch.int32
    assert seen.offsets.shape == (8,)
    assert int(seen.offsets[-1]) == seen.items.numel() == 6
    assert _slices(seen) == [[2], [], [], [1, 7, 9], [], [0, 8], []]
    assert seen.lengths.tolist() == [1, 0, 0, 3, 0, 2, 0]
    assert ncf.SeenItems is SeenItems


def test_seen_items_random_matches_python_sets():
    g = torch.Generator().manual_seed(5)
    U, I = 50, 97
    users = torch.randint(0, U, (600,), generator=g)
    users[users == 11] = 12                      # a user without interactions
    prods = torch.randint(0, I, (600,), generator=g)
    seen = SeenItems(users, prods, U, I)
    want = [sorted({p for u, p in zip(users.tolist(), prods.tolist()) if u == uu})
            for uu in range(U)]
    assert _slices(seen) == want and want[11] == []
    assert int(seen.offsets[-1]) == seen.items.numel()
    q_u = torch.tensor([12, 12, 11, 0])
    q_i = torch.tensor([want[12][0], (set(range(I)) - set(want[12])).pop(), 3, want[0][-1]])
    assert seen.contains(q_u, q_i).tolist() == [True, False, False, True]


def test_seen_items_empty_and_out_of_range():
    seen = SeenItems(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4, 9)
    assert seen.offsets.tolist() == [0] * 5 and seen.items.numel() == 0
    assert seen.contains(torch.tensor([1]), torch.tensor([2])).tolist() == [False]
    with pytest.raises(IndexError):
        SeenItems(torch.tensor([4]), torch.tensor([0]), 4, 9)
    with pytest.raises(IndexError):
        SeenItems(torch.tensor([0]), torch.tensor([9]), 4, 9)
    with pytest.raises(ValueError):
        SeenItems(torch.tensor([0, 1]), torch.tensor([1]), 4, 9)


def test_from_csr_validates():
    ok = SeenItems.from_csr([0, 2, 2, 5], [1, 4, 0, 3, 9], 10)
    assert _slices(ok) == [[1, 4], [], [0, 3, 9]]
    assert ok.items.dtype == torch.int32 and ok.offsets.dtype == torch.int64
    # a descent across two users' boundary is fine; inside one user it is not
    with pytest.raises(ValueError, match="sorted"):
        SeenItems.from_csr([0, 2, 2, 5], [4, 1, 0, 3, 9], 10)      # unsorted
    with pytest.raises(ValueError, match="sorted"):
        SeenItems.from_csr([0, 2, 2, 5], [1, 4, 3, 3, 9], 10)      # duplicated
    with pytest.raises(ValueError, match="range"):
        SeenItems.from_csr([0, 2, 2, 5], [1, 4, 0, 3, 10], 10)     # id == num_products
    with pytest.raises(ValueError, match="range"):
        SeenItems.from_csr([0, 2, 2, 5], [-1, 4, 0, 3, 9], 10)
    with pytest.raises(ValueError, match="offsets"):
        SeenItems.from_csr([0, 3, 2, 5], [1, 4, 0, 3, 9], 10)      # not monotone
    with pytest.raises(ValueError, match="offsets"):
        SeenItems.from_csr([0, 2, 2, 4], [1, 4, 0, 3, 9], 10)      # does not end at len(items)
    with pytest.raises(ValueError, match="offsets"):
        SeenItems.from_csr([1, 2, 2, 5], [1, 4, 0, 3, 9], 10)      # does not start at 0


def test_to_round_trips():
    seen = SeenItems(torch.tensor([1, 1, 2]), torch.tensor([5, 3, 0]), 3, 6)
    back = seen.to("cpu").to(torch.device("cpu"))
    assert back.num_users == 3 and back.num_products == 6
    assert torch.equal(back.offsets, seen.offsets) and torch.equal(back.items, seen.items)
    assert back.device == torch.device("cpu")


def test_exclude_mismatch_raises_before_any_gpu_call():
    """score_topk / GraphedScorer check ``exclude`` against the model before they touch the
    device: a stand-in model without any tensor gets as far as the ValueError."""
    seen = SeenItems(torch.tensor([1]), torch.tensor([2]), 5, 8)
    model = types.SimpleNamespace(num_users=6, num_products=8)
    with pytest.raises(ValueError, match="users"):
        scoring.score_topk(model, torch.tensor([0]), 3, exclude=seen)
    with pytest.raises(ValueError, match="users"):
        scoring.GraphedScorer(model, 4, 3, exclude=seen)
    with pytest.raises(ValueError, match="items"):
        scoring._check_exclude(seen, 5, 9)
    with pytest.raises(ValueError, match="move it"):
        scoring._check_exclude(seen, 5, 8, torch.device("cuda:0"))
    with pytest.raises(TypeError):
        scoring._check_exclude(torch.tensor([1]), 5, 8)
    scoring._check_exclude(seen, 5, 8, torch.device("cpu"))
    scoring._check_exclude(None, 5, 8)


def test_exclude_is_keyword_only_and_pinned_signatures_keep_their_positions():
    for fn in (scoring.score_topk, scoring.GraphedScorer.__init__, scoring.sharded_score_topk):
        p = inspect.signature(fn).parameters["exclude"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(scoring._TopKRun.__init__)[:5] == ["self", "index", "n", "k", "cap"]
    assert sig(scoring._TopKRun.safe_thresholds)[:3] == ["self", "redo", "st"]
    assert sig(scoring._collect)[-2:] == ["expected", "terms"]
    assert sig(scoring.score_topk)[:5] == ["model", "user_ids", "k", "index", "cap"]


def test_new_entry_points_are_declared():
    """One select entry, declared in the header and so bound; the three names it replaced are
    in neither the header nor SIGNATURES."""
    import os
    import re
    from ncf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ncf_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint\s+ncf_score_select\s*\(([^)]*)\)\s*;", header)
    assert decl is not None and "ncf_score_select" in _lib.SIGNATURES
    for name in ("ncf_score_select_rescored", "ncf_score_select_excl",
                 "ncf_score_select_rescored_excl"):
        assert name not in _lib.SIGNATURES
        assert name not in header
