"""GPU ranking metrics with the reference's ``calculate_metrics`` interface.

``calculate_metrics(predictions, targets, k_values, batch_size, negative_samples)`` returns the
same dictionary as src/utils/metrics.py:9-110 — ``hit_rate@k``, ``ndcg@k``, ``mrr@k``,
``map@k`` per k, ``auc``, ``accuracy``, ``pos_accuracy`` / ``neg_accuracy`` (when such rows
exist) — computed where the predictions already are: the per-group work (the reference's Python
loop over users) in one HIP launch (``ncf_group_metrics``), AUC as the Mann-Whitney statistic
(``ncf_auc_count``; sklearn's roc_auc_score with ties counted one half) over the negatives sorted
on the device.  Same argument checks and errors.  Tie order inside a group: prediction desc,
column asc (torch.topk / torch.sort leave it unspecified).  GPU only (no CPU fallback).

``full_ranking_metrics`` is the leave-one-out protocol over the whole catalogue instead of over
sampled negatives: the held-out item's place among all the items the user has not seen
(``scoring.score_topk(exclude=...)``).  ``ranking_report`` is the same protocol from the exact
place of every held-out item (``scoring.score_rank``): every k in one pass, untruncated MRR, mean
rank and per-user AUC.
"""
import warnings
from typing import Dict, List, Optional

import torch

from . import _lib
from ._lib import ptr


def calculate_metrics(predictions: torch.Tensor, targets: torch.Tensor,
                      k_values: List[int] = (1, 5, 10), batch_size: Optional[int] = None,
                      negative_samples: Optional[int] = None) -> Dict[str, float]:
    p = predictions.detach()
    t = targets.detach()
    if p.dim() == 2 and p.size(1) == 1:
        p = p.squeeze(1)
    if t.dim() == 2 and t.size(1) == 1:
        t = t.squeeze(1)
    if batch_size is None or negative_samples is None:
        raise ValueError("Please provide both batch_size and negative_samples "
                         "to reshape predictions into [batch_size, 1+negative_samples].")
    M = 1 + negative_samples
    if p.numel() != batch_size * M:
        raise ValueError(f"Size mismatch: got {p.numel()} total preds, "
                         f"but expected batch_size*M = {batch_size * M}.")
    if p.device.type != "cuda":
        raise RuntimeError("ncf_amd metrics run on the MI355X only (no CPU fallback)")
    dev = p.device
    p = p.to(torch.float32).contiguous()
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    ks = [int(k) for k in k_values]
    st = _lib.stream_ptr(dev)
    nf = 4 * len(ks) + 5
    ks_dev = torch.tensor(ks, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, _lib.query("ncf_group_metrics_workspace", batch_size, len(ks))),
                     dtype=torch.uint8, device=dev)
    sums = torch.empty(nf, dtype=torch.float64, device=dev)
    _lib.call("ncf_group_metrics", ptr(p), ptr(t), batch_size, M, ptr(ks_dev), len(ks), 0.5,
              ptr(sums), ptr(ws), ws.numel(), st)
    # AUC (metrics.py:243-256 -> sklearn.metrics.roc_auc_score)
    neg = torch.sort(p[t == 0]).values
    n_pos = int((t == 1).sum())
    n_neg = neg.numel()
    if n_pos + n_neg != t.numel():
        raise ValueError("roc_auc_score needs binary targets (0 / 1)")
    s2u = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("ncf_auc_count", ptr(p), ptr(t), p.numel(), ptr(neg), n_neg, ptr(s2u), st)
    h = sums.cpu().tolist()
    out: Dict[str, float] = {}
    B = float(batch_size)
    for j, k in enumerate(ks):
        out[f"hit_rate@{k}"] = h[4 * j] / B
        out[f"ndcg@{k}"] = h[4 * j + 1] / B
        out[f"mrr@{k}"] = h[4 * j + 2] / B
        out[f"map@{k}"] = h[4 * j + 3] / B
    if n_pos == 0 or n_neg == 0:
        # scikit-learn 1.6 (the reference's pin, requirements.txt:16) returns nan with an
        # UndefinedMetricWarning here; the reference's validate() always hits it (M = 1)
        warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in "
                      "that case.", RuntimeWarning)
        out["auc"] = float("nan")
    else:
        out["auc"] = float(int(s2u.item())) / (2.0 * n_pos * n_neg)
    base = 4 * len(ks)
    out["accuracy"] = h[base] / t.numel()
    if h[base + 1] > 0:
        out["pos_accuracy"] = h[base + 2] / h[base + 1]
    if h[base + 3] > 0:
        out["neg_accuracy"] = h[base + 4] / h[base + 3]
    return out


def full_ranking_metrics(model, users: torch.Tensor, heldout_items: torch.Tensor, k: int,
                         exclude=None, index=None, hour=None) -> Dict[str, float]:
    """Leave-one-out ``hr@k`` / ``ndcg@k`` / ``mrr@k`` of one held-out item per user, ranked
    against the whole catalogue without the user's training history (``exclude``: a
    ``scoring.SeenItems``; it must not hold the held-out items themselves).  A held-out item
    outside the user's top k counts 0 in all three.  ``hour``: the hour of day every held-out
    interaction carries (an int, or one per user), ranked as ``score_topk(hour=)`` does."""
    from .scoring import score_topk
    users = users.reshape(-1)
    held = heldout_items.reshape(-1)
    if users.numel() != held.numel():
        raise ValueError("one held-out item per user")
    if exclude is not None and bool(exclude.contains(users, held).any()):
        raise ValueError("full_ranking_metrics: a held-out item is in its user's history")
    _, items = score_topk(model, users, k, index, exclude=exclude, hour=hour)
    hit = items == held.to(items.device, torch.int64).unsqueeze(1)     # [n, k], one hit at most
    found = hit.any(1)
    place = hit.to(torch.int64).argmax(1).to(torch.float64)            # 0-based, where found
    n = max(1, users.numel())
    hr = found.to(torch.float64).sum() / n
    ndcg = torch.where(found, 1.0 / torch.log2(place + 2.0), torch.zeros_like(place)).sum() / n
    mrr = torch.where(found, 1.0 / (place + 1.0), torch.zeros_like(place)).sum() / n
    hr, ndcg, mrr = torch.stack([hr, ndcg, mrr]).tolist()
    return {f"hr@{k}": hr, f"ndcg@{k}": ndcg, f"mrr@{k}": mrr}


def ranking_report(model, users: torch.Tensor, heldout_items: torch.Tensor,
                   k_values=(1, 5, 10), exclude=None, index=None, hour=None) -> Dict[str, float]:
    """The leave-one-out protocol of ``full_ranking_metrics`` from the exact place of every
    held-out item (``scoring.score_rank``: one counting scan of the catalogue, no top-k lists):
    ``hr@k`` / ``ndcg@k`` / ``mrr@k`` for every k of ``k_values`` by the same formulas, and what a
    top-k list cannot give: ``mrr`` (untruncated), ``mean_rank`` (the mean of place + 1) and
    ``auc`` (the mean of 1 - place / (candidates - 1), the share of a user's other unseen items
    ranked below the held-out one, over the users with more than one candidate; nan without
    any).  ``exclude`` / ``index`` / ``hour`` as in ``full_ranking_metrics``."""
    from .scoring import score_rank
    ks = sorted({int(k) for k in k_values})
    if ks and ks[0] < 1:
        raise ValueError("ranking_report: k must be >= 1")
    place, cand = score_rank(model, users, heldout_items, index, exclude=exclude, hour=hour)
    pl = place.to(torch.float64)
    n = max(1, pl.numel())
    zero = torch.zeros_like(pl)
    sums = []
    for k in ks:
        found = place < k
        sums += [found.to(torch.float64).sum() / n,
                 torch.where(found, 1.0 / torch.log2(pl + 2.0), zero).sum() / n,
                 torch.where(found, 1.0 / (pl + 1.0), zero).sum() / n]
    many = cand > 1
    auc = torch.where(many, 1.0 - pl / (cand - 1).clamp_min(1).to(torch.float64), zero).sum() / \
        many.to(torch.float64).sum()      # (0 / 0 = nan: no user with two candidates)
    sums += [(1.0 / (pl + 1.0)).sum() / n, (pl + 1.0).sum() / n, auc]
    vals = torch.stack(sums).tolist()
    out: Dict[str, float] = {}
    for j, k in enumerate(ks):
        out[f"hr@{k}"], out[f"ndcg@{k}"], out[f"mrr@{k}"] = vals[3 * j:3 * j + 3]
    out["mrr"], out["mean_rank"], out["auc"] = vals[-3:]
    return out
