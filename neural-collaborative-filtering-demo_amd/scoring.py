"""Batch candidate scoring (C5): top-K items per user over the whole catalogue.

The reference serves recommendations with ``model.forward_simple(customer, all_products)`` and
``DataFrame.nlargest(top_k, 'score')`` (src/inference/demo/app.py:44-75).  ``score_topk`` returns
the same top-K (probabilities and item ids, ordered by score desc then item id asc) for many users
at once through the factorised eval form (csrc/score.hip):

    logit(u, i) = q_u . p_i + bias_i
    q_u    = w0 * LN_mf(U_mf[u]) * w_mf                 (ncf_score_queries)
    p_i    = LN_mf(I_mf[i])                              (ncf_gather_rows, cached per model state)
    bias_i = w1 * mlp_item(i) + w0 * b_mf + b_final      (the engine's eval forward + ncf_score_item_bias)

``ItemIndex`` caches the item side (p, bias) for a parameter version (optionally for a subset
of the catalogue: one rank's item shard); ``score_topk`` runs the threshold / MFMA-collect /
select pipeline (``GraphedScorer``: the same pipeline captured once as a hipGraph and replayed);
``sharded_score_topk`` is the item-sharded multi-GPU form: every
rank scores all queried users against its own item shard, the per-shard top-K lists are
all-gathered (RCCL) and merged per user by ``ncf_score_merge``.  GPU only; no CPU fallback.

``hour=`` ranks as ``forward_simple(user, all_items, hour)`` does (the reference's serving
default, app.py:43-77).  The hour path factorises the same way:

    logit(u, i, h) = (q_u * s_h) . p_i + bias_{h,i}
    s_h        = 1 + 0.3 * tp_h,  tp_h = hour_E[h], or proj(hour_E[h]) when T != D
    bias_{h,i} = w1 * mlp_item(i, h) + w0 * b_mf + b_final

so the item rows stay as they are, the hour scales the query (ncf_score_queries_hour, a 24-row
table built once per index) and picks the item bias (one vector per hour, built on first use
and cached on the index); everything after the queries runs unchanged on ``ItemIndex.at_hour``.
Where ``temporal_dim != mf_embedding_dim`` the reference draws a fresh random projection on
every call (architecture.py:437-442); a ranking needs one fixed projection, given to the index.

``exclude=SeenItems(...)`` ranks the items a user has not seen yet instead: the select drops the
candidates in the user's list (a CSR keyed by user id) and verifies the rest against the collect
threshold; a user whose seen items reach into the top k is re-run from a threshold that leaves
k unseen items at or above it (``_TopKRun.redo_excluded``).

``score_rank`` is the evaluation side of the same scorer: the exact 0-based place of one held-out
item per user among the items the user has not seen, by the top-k order, from one fp32 MFMA scan
that counts instead of collecting (csrc/rank.hip; no k, no thresholds, no re-runs).
"""
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ptr
from .engine import LN_EPS

K_MF_U = "mf_embedding_collection.embedding_bags.user_id.weight"
K_MF_I = "mf_embedding_collection.embedding_bags.product_id.weight"
QD = 64   # the scan's row width (ncf_score_queries pads narrower rows to it)


class ItemIndex:
    """Item-side factors of the factorised scorer for one model state."""

    def __init__(self, model, chunk: int = 65536, items: Optional[torch.Tensor] = None, *,
                 projection=None):
        """``items``: the global item ids this index covers (default: the whole catalogue).
        ``projection``: the ``nn.Linear(T, D)`` (or ``(weight, bias)``) of the hour path, as
        ``ops.forward_simple_hour`` takes it; needed to score at an hour when ``temporal_dim !=
        mf_embedding_dim``, unused otherwise."""
        eng = model._engine
        eng.sync_tables()
        self.model = model
        self.projection = projection
        self.chunk = chunk
        self.scale = None        # [24, D] s_h = 1 + 0.3 tp_h (hour_table)
        self._hour_bias = {}     # hour -> bias_{h, .} over this index's items
        dev = model.mf_norm.weight.device
        if dev.type != "cuda":
            raise RuntimeError("ncf_amd scoring runs on the MI355X only (no CPU fallback)")
        I = model.num_products
        D = model.mf_embedding_dim
        if D not in (16, 32, 64, 128):
            # (the scan kernels are 64 deep: narrower rows are zero-padded to 64, which leaves
            # every dot product the D-term one; D = 128 — the C4 model — takes the fp32 scan's
            # 128-deep form, k_collect<128>, with the fp32 threshold sample)
            raise NotImplementedError("the scoring kernels take D = 16, 32, 64 or 128")
        qd = max(QD, D)
        st = _lib.stream_ptr(dev)
        if items is None:
            ids = torch.arange(I, dtype=torch.int64, device=dev)
            self.ids = None
        else:
            ids = items.to(device=dev, dtype=torch.int64).contiguous()
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= I):
                raise IndexError("ItemIndex: item id out of range of the embedding table")
            self.ids = ids
            I = ids.numel()
        table = model.mf_embedding_collection.embedding_bags["product_id"].weight
        self.dim = D
        self._item_ids = ids
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        pD = torch.empty(I, D, device=dev)
        _lib.call("ncf_gather_rows", ptr(ids), I, ptr(table), model.num_products, D,
                  ptr(model.mf_norm.weight),
                  ptr(model.mf_norm.bias), LN_EPS, ptr(pD), ptr(err), st)
        if D == qd:
            self.p = pD
        else:   # zero-padded to the scan's 64-deep rows (the queries are padded alike)
            self.p = torch.zeros(I, qd, device=dev)
            self.p[:, :D].copy_(pD)
            del pD
        # mlp_item(i): the eval forward's MLP prediction depends on the item only (M = 1)
        mlp_item = torch.empty(I, device=dev)
        zeros = torch.zeros(max(1, min(I, chunk)), dtype=torch.int64, device=dev)
        with torch.no_grad():
            for c0 in range(0, I, chunk):
                c1 = min(I, c0 + chunk)
                w = eng.forward(zeros[:c1 - c0], ids[c0:c1], 1, False, 0.0, 0)
                mlp_item[c0:c1].copy_(w.mlp_pred)
        self.bias = torch.empty(I, device=dev)
        _lib.call("ncf_score_item_bias", ptr(mlp_item), I, ptr(model.final[0].weight),
                  ptr(model.final[0].bias), ptr(model.mf_output.bias), ptr(self.bias), st)
        # the item rows as three bf16 planes for the split-operand MFMA scan (fp32 accuracy)
        self.p3 = None
        self.pmax = None   # max_i |p_i| (float bits) for the 1/2-term scan's threshold margin
        self.terms = SPLIT_TERMS   # operand terms of the split scan (with pmax; else 3)
        if SPLIT_SCAN and qd == QD:    # (the split planes and their scan are 64 deep)
            self.p3 = torch.empty(3, I, QD, dtype=torch.int16, device=dev)
            _lib.call("ncf_score_split_items", ptr(self.p), I, QD, ptr(self.p3), st)
            if SPLIT_TERMS < 3:
                self.pmax = torch.empty(1, dtype=torch.int32, device=dev)
                _lib.call("ncf_score_item_norm_max", ptr(self.p), I, QD, ptr(self.pmax), st)
        self.version = _param_version(model) + self._projection_version()

    def valid_for(self, model) -> bool:
        return model is self.model and \
            self.version == _param_version(model) + self._projection_version()

    def _projection_tensors(self):
        pr = self.projection
        if pr is None:
            return ()
        return tuple(pr) if isinstance(pr, (tuple, list)) else (pr.weight, pr.bias)

    def _projection_version(self):
        # (in-place changes of the projection's tensors make the hour biases stale as well)
        return tuple(t._version for t in self._projection_tensors())

    def owns_projection(self, projection) -> bool:
        """Whether ``projection`` is this index's own (the same module, or the same tensors)."""
        if projection is self.projection:
            return True
        if projection is None or self.projection is None:
            return False
        mine = self._projection_tensors()
        theirs = tuple(projection) if isinstance(projection, (tuple, list)) else \
            (projection.weight, projection.bias)
        return len(mine) == len(theirs) and all(a is b for a, b in zip(mine, theirs))

    def hour_table(self) -> torch.Tensor:
        """The 24 query scales s_h = 1 + 0.3 tp_h, fp32 ``[24, D]`` (built once): tp_h is
        ``hour_E[h]``, projected to D columns when ``temporal_dim != mf_embedding_dim``
        (architecture.py:434-444), by the kernels ``forward_simple_hour`` uses."""
        if self.scale is not None:
            return self.scale
        from .sparse import gather_rows
        m = self.model
        D, T = m.mf_embedding_dim, m.temporal_dim
        if D != m.mlp_embedding_dim:
            # (as forward_simple(hour): the reference scales the MLP item rows by a vector of
            # the MF width, architecture.py:436-456, a broadcast error unless the widths agree)
            raise RuntimeError(f"forward_simple(hour): the temporal scale has {D} columns, the "
                               f"MLP item rows {m.mlp_embedding_dim}")
        dev = self.p.device
        if T != D and self.projection is None:
            raise ValueError(
                f"scoring at an hour with temporal_dim {T} != mf_embedding_dim {D} needs "
                "ItemIndex(..., projection=nn.Linear(T, D)): the reference draws a fresh random "
                "projection on every call (architecture.py:437-442), and a ranking needs one "
                "fixed projection")
        te = gather_rows(m.temporal_encoding.hour_embed.weight,
                         torch.arange(24, dtype=torch.int64, device=dev))
        if T != D:
            w_p, b_p = self._projection_tensors()
            w_p = w_p.detach().to(device=dev, dtype=torch.float32).contiguous()
            b_p = b_p.detach().to(device=dev, dtype=torch.float32).contiguous()
            tp = torch.empty(24, D, device=dev)
            _lib.call("ncf_gemm_f32", 24, D, T, ptr(te), T, 0, ptr(w_p), T, 1, ptr(tp), D,
                      ptr(b_p), 0, _lib.stream_ptr(dev))
        else:
            tp = te
        self._te, self._tp = te, tp
        self.scale = (1.0 + 0.3 * tp).contiguous()
        return self.scale

    def hour_bias(self, hour: int) -> torch.Tensor:
        """bias_{h, i} = w1 * mlp_item(i, h) + w0 * b_mf + b_final over this index's items, built
        on first use (the chunked eval forward of ``__init__`` with the hour's ``temporal=``) and
        kept while the index is valid."""
        hour = int(hour)
        if not 0 <= hour < 24:
            raise IndexError(f"hour {hour} is outside [0, 24)")
        b = self._hour_bias.get(hour)
        if b is not None:
            return b
        self.hour_table()
        model, ids = self.model, self._item_ids
        eng = model._engine
        dev = self.p.device
        I = ids.numel()
        cn = max(1, min(I, self.chunk))
        tp_rows = self._tp[hour].expand(cn, -1).contiguous()
        te_rows = self._te[hour].expand(cn, -1).contiguous()
        zeros = torch.zeros(cn, dtype=torch.int64, device=dev)
        mlp_item = torch.empty(I, device=dev)
        with torch.no_grad():
            for c0 in range(0, I, cn):
                c1 = min(I, c0 + cn)
                w = eng.forward(zeros[:c1 - c0], ids[c0:c1], 1, False, 0.0, 0,
                                temporal=(tp_rows[:c1 - c0], 0.3, te_rows[:c1 - c0]))
                mlp_item[c0:c1].copy_(w.mlp_pred)
        b = torch.empty(I, device=dev)
        _lib.call("ncf_score_item_bias", ptr(mlp_item), I, ptr(model.final[0].weight),
                  ptr(model.final[0].bias), ptr(model.mf_output.bias), ptr(b),
                  _lib.stream_ptr(dev))
        self._hour_bias[hour] = b
        return b

    def at_hour(self, hour: int, bias: Optional[torch.Tensor] = None) -> "HourView":
        """This index as the pipeline sees it at ``hour``: the same item rows with that hour's
        bias (``bias``: a buffer to use in its place, the graphed scorer's static one)."""
        scale = self.hour_table()
        return HourView(self, scale, self.hour_bias(hour) if bias is None else bias)


class HourView:
    """An ``ItemIndex`` at one hour of day: its ``p`` / ``p3`` / ``pmax`` / ``terms`` / ``ids`` /
    ``dim`` (the item rows do not depend on the hour), the hour's ``bias`` and the query scale
    table.  The collect, select and re-run code reads it like an index."""

    def __init__(self, base: ItemIndex, scale: torch.Tensor, bias: torch.Tensor):
        self.base, self.scale, self.bias = base, scale, bias
        self.p, self.p3, self.pmax, self.terms = base.p, base.p3, base.pmax, base.terms
        self.ids, self.dim = base.ids, base.dim


def _param_version(model):
    # torch's _version sees optimizer steps through torch; engine.updates the HIP kernels' writes
    return (model._engine.updates,) + tuple(p._version for p in model.parameters())


def _resolve_index(model, index, projection, caller: str, items=None) -> "ItemIndex":
    """The index a call scores over: ``index`` when it is valid for the model's parameters, a
    rebuilt one over the same items and projection when they changed since, a new one when none
    was given (``items``: a function returning the ids a new or rebuilt index covers; default
    the whole catalogue, or the stale index's own).  A ``projection`` beside an index must be the
    index's own."""
    if index is None:
        return ItemIndex(model, items=items and items(), projection=projection)
    if projection is not None and not index.owns_projection(projection):
        raise ValueError(f"{caller}: index was built with another projection; pass the "
                         "projection to ItemIndex and leave it out here")
    if not index.valid_for(model):   # parameters changed since the index was built
        index = ItemIndex(model, items=items() if items else index.ids,
                          projection=index.projection)
    return index


def _queries(model, uid, n, q, err, st, hours=None, scale=None):
    """The query rows of ``uid[:n]`` into ``q`` on stream ``st`` (ncf_score_queries; with
    ``hours``: ncf_score_queries_hour, row r times ``scale[hours[r]]``).  The kernel ORs 1 into
    ``err`` for a user id, 2 for an hour out of range."""
    table = model.mf_embedding_collection.embedding_bags["user_id"].weight
    rows = (ptr(table), model.num_users, model.mf_embedding_dim, ptr(model.mf_norm.weight),
            ptr(model.mf_norm.bias), LN_EPS, ptr(model.mf_output.weight),
            ptr(model.final[0].weight))
    if hours is None:
        _lib.call("ncf_score_queries", ptr(uid), n, *rows, ptr(q), ptr(err), st)
    else:
        _lib.call("ncf_score_queries_hour", ptr(uid), ptr(hours), n, *rows, ptr(scale), ptr(q),
                  ptr(err), st)


def _raise_flags(flags: int, caller: str):
    """The kernels' error word (1: user id, 2: hour, 4: item id out of range) as an IndexError."""
    if flags & 1:
        raise IndexError(f"{caller}: user id out of range of the embedding table")
    if flags & 2:
        raise IndexError(f"{caller}: hour outside [0, 24)")
    if flags & 4:
        raise IndexError(f"{caller}: item id out of range of the catalogue")


class SeenItems:
    """Every user's already-seen items, as a CSR over the whole user table: ``offsets`` int64
    ``[num_users + 1]``, ``items`` int32 global item ids, sorted ascending and unique within a
    user.  Passed as ``exclude=`` to ``score_topk`` / ``GraphedScorer`` / ``sharded_score_topk``,
    which then rank the other items only.  Keyed by user id, not by position in a call."""

    def __init__(self, users, products, num_users: int, num_products: int):
        """From an interactions table (one ``(user, product)`` pair per row; duplicates and users
        without a row are fine): the ``unique(u * I + p)`` construction of
        ``DeviceNegativeSampler``.  Runs on the tensors' device (CPU tensors: no GPU needed)."""
        users = torch.as_tensor(users).to(torch.int64).reshape(-1)
        products = torch.as_tensor(products).to(torch.int64).reshape(-1)
        if users.numel() != products.numel():
            raise ValueError("users and products must have the same length")
        if users.numel() and (int(users.min()) < 0 or int(users.max()) >= num_users or
                              int(products.min()) < 0 or int(products.max()) >= num_products):
            raise IndexError("interaction ids out of range")
        key = torch.unique(users * num_products + products.to(users.device))
        hu, hi = key // num_products, key % num_products
        offsets = torch.zeros(num_users + 1, dtype=torch.int64, device=key.device)
        offsets[1:] = torch.cumsum(torch.bincount(hu, minlength=num_users), 0)
        self._set(offsets, hi.to(torch.int32), num_products)

    def _set(self, offsets, items, num_products):
        if not 0 < num_products < 2 ** 31:
            raise ValueError("num_products must be in [1, 2^31)")
        self.offsets, self.items, self.num_products = offsets, items, int(num_products)
        self._lengths = None

    @classmethod
    def from_csr(cls, offsets, items, num_products: int) -> "SeenItems":
        """From a ready CSR (validated: monotone offsets from 0 to ``len(items)``, item ids in
        range, every user's slice sorted ascending without repeats)."""
        offsets = torch.as_tensor(offsets).to(torch.int64).reshape(-1).contiguous()
        items = torch.as_tensor(items).reshape(-1)
        if offsets.numel() < 1 or int(offsets[0]) != 0 or int(offsets[-1]) != items.numel() or \
                bool((offsets[1:] < offsets[:-1]).any()):
            raise ValueError("SeenItems: offsets must rise from 0 to len(items)")
        if items.numel():
            if items.is_floating_point() or int(items.min()) < 0 or \
                    int(items.max()) >= num_products:
                raise ValueError("SeenItems: item id out of range")
            # within a user (no offset between two neighbours) the ids strictly increase
            start = torch.zeros(items.numel() + 1, dtype=torch.bool, device=offsets.device)
            start[offsets] = True
            if bool(((items[1:] <= items[:-1]).to(offsets.device) & ~start[1:-1]).any()):
                raise ValueError("SeenItems: every user's items must be sorted and unique")
        self = cls.__new__(cls)
        self._set(offsets, items.to(device=offsets.device, dtype=torch.int32).contiguous(),
                  num_products)
        return self

    @classmethod
    def _shared(cls, offsets, items, num_products):
        """Around tensors that already hold a valid CSR, without a copy."""
        self = cls.__new__(cls)
        self._set(offsets, items, num_products)
        return self

    @property
    def num_users(self) -> int:
        return self.offsets.numel() - 1

    @property
    def device(self):
        return self.offsets.device

    @property
    def lengths(self) -> torch.Tensor:
        """Seen items per user, int64 ``[num_users]``."""
        if self._lengths is None:
            self._lengths = self.offsets[1:] - self.offsets[:-1]
        return self._lengths

    def to(self, device) -> "SeenItems":
        return SeenItems._shared(self.offsets.to(device), self.items.to(device), self.num_products)

    def contains(self, users: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
        """Per pair, whether ``items[j]`` is in ``users[j]``'s list (torch ops on ``device``)."""
        u = users.to(device=self.device, dtype=torch.int64).reshape(-1)
        it = items.to(device=self.device, dtype=torch.int64).reshape(-1)
        if self.items.numel() == 0:
            return torch.zeros_like(u, dtype=torch.bool)
        owner = torch.repeat_interleave(torch.arange(self.num_users, device=self.device),
                                        self.lengths)
        keys = owner * self.num_products + self.items.to(torch.int64)   # sorted ascending
        want = u * self.num_products + it
        pos = torch.searchsorted(keys, want).clamp_max(keys.numel() - 1)
        return keys[pos] == want


def _check_exclude(exclude, num_users: int, num_products: int, device=None):
    """The ``exclude=`` argument against the model it is used with (before any launch)."""
    if exclude is None:
        return
    if not isinstance(exclude, SeenItems):
        raise TypeError("exclude must be a SeenItems")
    if exclude.num_users != num_users:
        raise ValueError(f"exclude covers {exclude.num_users} users, the model has {num_users}")
    if exclude.num_products != num_products:
        raise ValueError(f"exclude is over {exclude.num_products} items, the model has "
                         f"{num_products}")
    if device is not None and exclude.device != device:
        raise ValueError(f"exclude is on {exclude.device}, the index on {device}: "
                         "move it with exclude.to(device)")


# the candidate scan on bf16 matrix cores with split operands (fp32 accuracy, same candidate
# sets; an index without the planes, p3 = None, takes the fp32 MFMA scan)
SPLIT_SCAN = True
# terms per operand of the split scan: 1 (one bf16 product per pair) or 2 (three products) — the
# thresholds lowered by the scan's error bound, the candidates near the K-th re-scored in fp32, so
# the top-k are the same bits either way (tested) — or 3 (six products, fp32-accurate logits
# straight from the scan).  Measured (10K users x 1M items, ms, top-10 / top-100): 1 term
# 2.85 / 4.29 (scan 2.06 / 2.42), 2 terms 4.75 / 5.76 (scan 3.67 / 3.82), 3 terms 6.8 / 8.5
SPLIT_TERMS = 1
# >= the scan's |logit error| / (|q|_2 max_i |p_i|_2) (Cauchy-Schwarz over the per-term errors),
# with the fp32 accumulation and the fp32 re-scoring's own rounding: two terms (the dropped
# products ~2^-16 relative): ~6.1e-5; one term (bf16 keeps 8 significant bits: each operand
# rounded within 2^-8 of itself, |a0 b0 - a b| <= (2^-7 + 2^-16) |a| |b|): 7.83e-3 + 2 x 64 x
# 2^-24 = 7.84e-3
MARGIN_C = {1: 8e-3, 2: 1e-4}


def _terms(idx):
    return idx.terms if idx.pmax is not None else 3


def _collect(idx, q, rows, n, thr, cap, count, cand, st, expected=0, terms=None):
    """ncf_score_collect(_split) of n queried users over the index's items (``expected``: the
    candidates per user the thresholds aim at, which sizes the split scan's item split;
    ``terms``: the split scan's operand terms, default the index's)."""
    I, D = idx.p.shape
    if idx.p3 is not None:
        terms = terms or _terms(idx)
        if terms < 3:   # lower the thresholds by the scan's error bound first
            _lib.call("ncf_score_margin", q, rows, n, D, ptr(idx.pmax), MARGIN_C[terms], thr, st)
        _lib.call("ncf_score_collect_split", q, rows, n, ptr(idx.p3), ptr(idx.bias), I, D, thr,
                  cap, count, cand, terms, int(expected), st)
    else:
        _lib.call("ncf_score_collect", q, rows, n, ptr(idx.p), ptr(idx.bias), I, D, thr, cap,
                  count, cand, st)


# Expected candidates per user the threshold sample aims at: 512 (a bigger sample costs a
# longer sample GEMM and k-th select, a smaller one more scan hits and select work; round 1,
# fp32 scan: 1024 -> 7.5 ms, 2048 -> 7.7, cap / 2 = 4096 -> 8.3 at top-10 over 1M items), with the sample
# kept within the k-th kernel's LDS-resident size (top-100: ~2570; a 30720-logit cap: 6.26 ms,
# 38912: 5.90 ms), and never above cap / 2.
# (round 4, 10K x 1M eager, 2-4 interleaved runs: top-10 2.61-2.64 ms at 512 (scan 1.78-1.80,
# sample + k-th 0.42) against 2.64-2.82 at 1024 (scan 1.99-2.04, sample + k-th 0.21) and
# 2.99-3.16 at 2048; top-100 takes the rank-j plan, unaffected)
SAMPLE_CANDS = 512
# the collect scans its users in threshold order (see _TopKRun.launch).  Off: measured slower
# (graphed top-10 2.21 / 2.23 against 2.15 / 2.16 ms, r5zk: the scan no faster — the thresholds
# of a user block are already close — and the sort on top)
SORT_USERS = False
# the split scan's item split raised from the expected candidates per user (the launch's
# expected_per_user: fewer per-wave LDS slice overflows; tested invisible in the results)
SIZED_SPLIT = True
KTH_LDS_MAX = _lib.DEFINES["NCF_SCORE_KTH_LDS_MAX"]   # score.hip kKthLdsMax
# score.hip kSelectMax: the longest candidate list the select takes
SELECT_MAX = _lib.DEFINES["NCF_SCORE_SELECT_MAX"]
# the threshold sample on bf16 matrix cores, fp16 logits rounded down (ncf_score_sample_split16 +
# ncf_score_kth16, its k-th lowered by the two-term bound) instead of the fp32 sample GEMM +
# fp32 k-th (measured, 10K x 1M eager: top-100 4.25 -> 3.73 ms, top-10 2.78 -> 2.70); needs the
# split index (p3, pmax); tests compare both
SAMPLE16 = True
# the fp16 sample keeps only the maximum of every SAMPLE_GROUP consecutive sample items (the k-th
# largest group maximum bounds the k-th largest logit from below as well), where the sample
# holds >= 8 j group maxima: 8x fewer bytes written and selected over; 1 = every logit
SAMPLE_GROUP = 8


def _select(idx, rows, n, run, k, out_s, out_i, overflow, st, terms=None, check=None,
            exclude=None):
    """ncf_score_select of n users' candidate lists (with its re-scoring group after a one- or
    two-term scan, fp32; ``terms`` as the scan's; ``check``: the rank-j thresholds to verify the
    selection against, flag 2 where it is not provably the top k; ``exclude``: the users' seen
    items, looked up by ``run.uid`` and dropped from the lists first, its exclusion group)."""
    rescore = (None, None, None, 0, None, 0.0) if idx.pmax is None else \
        (ptr(run.q), ptr(idx.p), ptr(idx.bias), idx.p.shape[1], ptr(idx.pmax),
         MARGIN_C[terms or _terms(idx)])
    seen = (None, 0, None, None, None) if exclude is None else \
        (ptr(run.uid), exclude.num_users, ptr(exclude.offsets), ptr(exclude.items), ptr(idx.ids))
    _lib.call("ncf_score_select", rows, n, ptr(run.count), ptr(run.cand), run.cap, k, *rescore,
              out_s, out_i, ptr(run.thr), overflow, check, *seen, st)


# Rank-j thresholds (the fp16 sample path, k > RANK_J): the threshold is the sample's j-th
# largest logit (j = RANK_J) instead of its k-th, over a sample k / j times smaller, aimed at
# RANK_J * k expected candidates per user.  It is not a guaranteed bound of the k-th logit, so the
# select verifies each user's result against it (every item at or above it was collected; the
# k chosen are exact iff k were found and the k-th is at or above it) and flags the rest, which
# are re-run from the sample's k-th (guaranteed).  The number of items at or above the j-th of a
# sample of S ~ n_items / k is ~ Gamma(j) * k: below k with probability P(Gamma(16) < 1) ~ 1e-14
# per user on exchangeable scores.  RANK_J = 0: the k-th always.
RANK_J = 16
SAMPLE_MIN = 4096   # items in the smallest threshold sample
# Rank-j sample size factor f: S ~ f n_items / k, so ~RANK_J k / f candidates per user are
# expected and a user needs the guaranteed re-run with probability P(Gamma(RANK_J) < f)
# (f = 2: ~4e-10 per user).  Measured at top-100 (10K x 1M, graphed): f = 1 2.62 / 2.68 ms, f = 2
# 3.29 / 3.33, f = 3 3.28 / 3.41 (r5zl: the larger samples' scans were slower, not faster)
RANK_SAMPLE_F = 1


def _threshold_rank(k: int, cap: int, s16: bool) -> int:
    """The sample rank whose logit is the collect threshold: k, or RANK_J (see above)."""
    if s16 and RANK_J > 0 and k > RANK_J and RANK_J * k <= cap // 2:
        return RANK_J
    return k


def _sample_size(n_items: int, k: int, cap: int, j: int = 0) -> int:
    """Items in the threshold sample S: expected candidates ~ j * n_items / S (j = k by
    default; j < k: the rank-j plan, S ~ n_items / k, RANK_J * k candidates expected)."""
    j = j or k
    if j < k:
        s = max(SAMPLE_MIN, -(-j * n_items * RANK_SAMPLE_F // (RANK_J * k)))
    else:
        s = max(SAMPLE_MIN, -(-k * n_items // max(1, SAMPLE_CANDS)))
    s = max(min(s, KTH_LDS_MAX), -(-2 * j * n_items // cap))
    s = -(-s // 256) * 256
    return min(n_items, s)


class _TopKRun:
    """Buffers and launch sequence of one top-k pipeline for ``n`` users (shared by the eager
    ``score_topk`` and the captured ``GraphedScorer``)."""

    def __init__(self, index: "ItemIndex", n: int, k: int, cap: int,
                 exclude: Optional[SeenItems] = None):
        p = index.p
        dev = p.device
        I, D = p.shape
        if not 1 <= k <= min(I, cap):
            raise ValueError(f"k must be in [1, {min(I, cap)}]")
        self.index, self.n, self.k, self.cap = index, n, k, cap
        self.exclude = exclude
        s16 = SAMPLE16 and index.p3 is not None and index.pmax is not None
        self.j = _threshold_rank(k, cap, s16)
        self.S = _sample_size(I, k, cap, self.j)
        self.stride = I // self.S
        # the sample's item biases, contiguous: added in the sample GEMM's epilogue
        self.sbias = index.bias[::self.stride][:self.S].contiguous()
        e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)  # noqa: E731
        self.uid = e(max(n, 1), dt=torch.int64)
        # an index at an hour (HourView): the users' hours, read by ncf_score_queries_hour
        self.hours = torch.zeros(max(n, 1), dtype=torch.int64, device=dev) \
            if isinstance(index, HourView) else None
        self.s16 = s16 and self.S <= KTH_LDS_MAX
        # (rank j only where the sample leaves >= 8 k candidates expected: a small catalogue's
        # sample floor of 4096 items would otherwise put the j-th near the k-th item overall)
        if self.j < k and (not self.s16 or self.j * I < 8 * k * self.S):
            self.j = k
            self.S = _sample_size(I, k, cap)
            self.stride = I // self.S
            self.sbias = index.bias[::self.stride][:self.S].contiguous()
        # sample group maxima (fp16 path): rows of Sg = ceil(S / G)
        self.G = SAMPLE_GROUP if self.s16 and SAMPLE_GROUP > 1 and \
            self.S // SAMPLE_GROUP >= 8 * self.j else 1
        self.Sg = -(-self.S // self.G)
        self.q, self.thr = e(max(n, 1), D), e(max(n, 1))
        # the rank-j thresholds before the margins (the select's check).  With exclusion every
        # threshold is checked: it bounds the k-th logit of the catalogue, not of the unseen
        # items (there: the guaranteed thresholds, after the sample's own margin)
        self.thr_chk = e(max(n, 1)) if self.j < k or exclude is not None else None
        self.sample = (torch.empty(max(n, 1), self.Sg, dtype=torch.int16, device=dev) if self.s16
                       else e(max(n, 1), self.S))
        self.count = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        # (logit f32, item i32) records, ncf_score_cand: one 8-byte store per candidate
        self.cand = e(max(n, 1), cap, 2, dt=torch.int32)
        self.overflow = e(max(n, 1), dt=torch.int32)
        self.scores, self.items = e(n, k), e(n, k, dt=torch.int64)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(self, model, st):
        """queries -> threshold sample (MFMA GEMM over strided item rows) -> k-th threshold ->
        MFMA collect -> select, on stream ``st``; reads self.uid[:n]."""
        idx, n, k, cap = self.index, self.n, self.k, self.cap
        p, bias = idx.p, idx.bias
        I, D = p.shape
        # (an index at an hour: q_u (.) s_h, h = self.hours[u's row])
        _queries(model, self.uid, n, self.q, self.err, st, self.hours,
                 idx.scale if self.hours is not None else None)
        if self.s16:
            _lib.call("ncf_score_sample_split16", ptr(self.q), n, ptr(idx.p3), I, D, self.stride,
                      ptr(self.sbias), self.S, self.G, ptr(self.sample), st)
            _lib.call("ncf_score_kth16", ptr(self.sample), n, self.Sg, self.j, ptr(self.thr), st)
            if self.thr_chk is not None and self.exclude is None:
                self.thr_chk.copy_(self.thr)
            # (the k-th of the fp16 sample is a bound after the two-term error is taken off)
            _lib.call("ncf_score_margin", ptr(self.q), None, n, D, ptr(idx.pmax), MARGIN_C[2],
                      ptr(self.thr), st)
            if self.exclude is not None:
                self.thr_chk.copy_(self.thr)
        else:
            _lib.call("ncf_gemm_f32", n, self.S, D, ptr(self.q), D, 0, ptr(p), D * self.stride, 1,
                      ptr(self.sample), self.S, ptr(self.sbias), 0, st)
            _lib.call("ncf_score_kth", ptr(self.sample), n, self.S, k, None, self.stride,
                      ptr(self.thr), st)
            if self.thr_chk is not None:   # (exclusion only: this plan's rank is k)
                self.thr_chk.copy_(self.thr)
        self.count.zero_()
        # the scan's users in threshold order (SORT_USERS): its 32-user blocks then hold users of
        # near-equal thresholds, so its first reject (a lane's best logit against the smallest
        # of its 16 users' thresholds) is nearly as tight as the per-user test
        rows = None
        if SORT_USERS and n >= 64:
            self.order = torch.argsort(self.thr[:n]).to(torch.int32)
            rows = ptr(self.order)
        # expected candidates per user: k x I / S (the threshold sample's k-th over S items)
        _collect(idx, ptr(self.q), rows, n, ptr(self.thr), cap, ptr(self.count), ptr(self.cand),
                 st, expected=-(-self.j * I // self.S) if SIZED_SPLIT else 0)
        _select(idx, None, n, self, k, ptr(self.scores), ptr(self.items), ptr(self.overflow), st,
                check=None if self.thr_chk is None else ptr(self.thr_chk), exclude=self.exclude)

    def safe_thresholds(self, redo, st, rank=None, cap=None):
        """Users flagged by the rank-j check: their threshold from the sample's k-th instead (the
        fp32 sample GEMM over the same strided items, its k-th: k sample items at or above it, a
        guaranteed bound; the re-run's collect lowers it by the scan's margin).  ``rank``: the
        sample rank to take instead of k (exclusion: k + the longest list of these users, so k
        unseen items are at or above it; -inf where the sample is smaller than that), for
        candidate lists of ``cap``."""
        idx, k = self.index, rank or self.k
        cap = cap or self.cap
        p = idx.p
        I, D = p.shape
        if k > _sample_size(I, k, cap):
            self.thr[redo] = float("-inf")
            return
        q = self.q[redo].contiguous()
        nr = q.shape[0]
        # (a sample sized for the k-th itself, ~k I / S candidates within cap: the rank-j
        # sample's S ~ I / k would expect ~k^2 of them, over the cap at k = 100, and cost every
        # flagged user a further overflow round)
        S = _sample_size(I, k, cap)
        stride = I // S
        sbias = idx.bias[::stride][:S].contiguous()
        sample = torch.empty(nr, S, device=p.device)
        thr = torch.empty(nr, device=p.device)
        _lib.call("ncf_gemm_f32", nr, S, D, ptr(q), D, 0, ptr(p), D * stride, 1,
                  ptr(sample), S, ptr(sbias), 0, st)
        _lib.call("ncf_score_kth", ptr(sample), nr, S, k, None, stride, ptr(thr), st)
        self.thr[redo] = thr

    def redo_overflow(self, st):
        """Re-run the users whose candidate list overflowed (flag 1) or whose rank-j result was
        not provably exact (flag 2) (eager; rare: the threshold sample targets cap / 2
        candidates at most, and a rank-j shortfall has probability ~1e-14 per user)."""
        if self.exclude is not None:
            return self.redo_excluded(st)
        idx, k, cap = self.index, self.k, self.cap
        p, bias = idx.p, idx.bias
        I, D = p.shape
        dev = p.device
        overflow = self.overflow[:self.n]
        # the re-runs scan with at least two terms: their thresholds (the K-th re-scored logit
        # seen) sit just below the K-th, and the one-term scan's margin (~8e-3 |q| max|p|) could
        # keep more than cap items above the lowered threshold
        terms = max(2, _terms(idx))
        for _ in range(32):
            redo = torch.nonzero(overflow).flatten()
            if redo.numel() == 0:
                return
            short = redo[overflow[redo] == 2]
            if short.numel():
                self.safe_thresholds(short, st)
            rows = redo.to(torch.int32)
            self.count[redo] = 0
            sub_s = torch.empty(rows.numel(), k, device=dev)
            sub_i = torch.empty(rows.numel(), k, dtype=torch.int64, device=dev)
            sub_o = torch.empty(rows.numel(), dtype=torch.int32, device=dev)
            _collect(idx, ptr(self.q), ptr(rows), rows.numel(), ptr(self.thr), cap,
                     ptr(self.count), ptr(self.cand), st, terms=terms)
            _select(idx, ptr(rows), rows.numel(), self, k, ptr(sub_s), ptr(sub_i), ptr(sub_o), st,
                    terms=terms)
            self.scores[redo] = sub_s
            self.items[redo] = sub_i
            overflow.zero_()
            overflow[redo] = sub_o
        raise RuntimeError("score_topk: candidate lists kept overflowing (degenerate scores?)")

    def redo_excluded(self, st):
        """redo_overflow with exclusion: the flagged users (1: the list overflowed; 2: fewer than
        k unseen candidates at or above the checked threshold) re-run in buffers of their own.
        Flag 2 takes the fp32 sample's rank k + e as the threshold, e the longest list among the
        flagged users: at least k + e items are at or above it and at most e of them are seen.
        The lists hold cap_r >= k + e candidates, so an overflowing list always shows the select k
        unseen ones and the threshold it returns (their k-th) rises every round."""
        idx, k, ex = self.index, self.k, self.exclude
        dev = idx.p.device
        overflow = self.overflow[:self.n]
        redo = torch.nonzero(overflow).flatten()
        if redo.numel() == 0:
            return
        uid = self.uid[redo]
        ok = (uid >= 0) & (uid < ex.num_users)   # (an id out of range raises after this)
        e = int((ex.lengths[uid.clamp(0, ex.num_users - 1)] * ok).max())
        if k + e > SELECT_MAX:
            raise ValueError(f"score_topk: k + the longest seen list ({k} + {e}) exceeds the "
                             f"select's {SELECT_MAX} candidates")
        cap_r = max(self.cap, min(SELECT_MAX, 2 * (k + e)))
        short = redo[overflow[redo] == 2]
        if short.numel():
            self.safe_thresholds(short, st, rank=k + e, cap=cap_r)
        nr = redo.numel()
        sub = SimpleNamespace(
            q=self.q[redo].contiguous(), uid=uid.contiguous(), thr=self.thr[redo].contiguous(),
            count=torch.zeros(nr, dtype=torch.int32, device=dev), cap=cap_r,
            cand=torch.empty(nr, cap_r, 2, dtype=torch.int32, device=dev))
        terms = max(2, _terms(idx))   # (as redo_overflow)
        rows = torch.arange(nr, dtype=torch.int32, device=dev)
        for _ in range(32):
            m = rows.numel()
            sub_s = torch.empty(m, k, device=dev)
            sub_i = torch.empty(m, k, dtype=torch.int64, device=dev)
            sub_o = torch.empty(m, dtype=torch.int32, device=dev)
            sub.count.zero_()
            _collect(idx, ptr(sub.q), ptr(rows), m, ptr(sub.thr), cap_r, ptr(sub.count),
                     ptr(sub.cand), st, terms=terms)
            _select(idx, ptr(rows), m, sub, k, ptr(sub_s), ptr(sub_i), ptr(sub_o), st,
                    terms=terms, exclude=ex)
            dst = redo[rows.long()]
            self.scores[dst] = sub_s
            self.items[dst] = sub_i
            rows = rows[sub_o != 0]
            if rows.numel() == 0:
                overflow.zero_()
                return
        raise RuntimeError("score_topk: candidate lists kept overflowing (degenerate scores?)")

    def result(self):
        items = self.items
        if self.index.ids is not None:   # shard-local positions -> global item ids
            if self.exclude is None:
                items = self.index.ids[items.clamp_min(0)]
            else:   # (a shard may run out of unseen items: its empty slots stay -1)
                items = torch.where(items < 0, items, self.index.ids[items.clamp_min(0)])
        return self.scores, items


def _check_hour(hour, n_users: int):
    """The ``hour=`` argument before any launch: None, an int in [0, 24) (IndexError outside), or
    an integer tensor with one hour per user (ValueError at another length), returned flat."""
    if hour is None:
        return None
    if isinstance(hour, torch.Tensor) and hour.dim() > 0:
        if hour.is_floating_point() or hour.dtype == torch.bool:
            raise TypeError("hour must be an int or an integer tensor")
        hour = hour.reshape(-1)
        if hour.numel() != n_users:
            raise ValueError(f"hour holds {hour.numel()} entries for {n_users} users "
                             "(one hour per user, or one int)")
        return hour
    if isinstance(hour, (bool, float)) or \
            (isinstance(hour, torch.Tensor) and hour.is_floating_point()):
        raise TypeError("hour must be an int or an integer tensor")
    hour = int(hour)
    if not 0 <= hour < 24:
        raise IndexError(f"hour {hour} is outside [0, 24)")
    return hour


def _one_hour(hour, n_users: int) -> int:
    """``_check_hour`` for the graphed scorer, whose replay runs at one hour."""
    hour = _check_hour(hour, n_users)
    if isinstance(hour, torch.Tensor):
        if hour.numel() == 0 or bool((hour != hour[0]).any()):
            raise ValueError("GraphedScorer replays one hour per call (an int); users at "
                             "several hours go through score_topk(hour=tensor)")
        hour = _check_hour(int(hour[0]), n_users)
    return hour


def group_by_hour(hours: torch.Tensor):
    """``[(hour, positions)]`` over the distinct values of a 1-D integer tensor, hours ascending,
    every group's positions (int64, on the tensor's device) in the caller's order."""
    hours = hours.reshape(-1)
    if hours.numel() == 0:
        return []
    order = torch.argsort(hours, stable=True)
    uniq, counts = torch.unique_consecutive(hours[order], return_counts=True)
    return list(zip(uniq.tolist(), torch.split(order, counts.tolist())))


def _topk_eager(model, uid, k, idx, cap, exclude, hours=None):
    """One eager pipeline run of ``uid`` over ``idx`` (an ItemIndex, or a HourView with the
    users' ``hours``: an int, or a tensor the kernel range-checks)."""
    n = uid.numel()
    run = _TopKRun(idx, n, k, cap, exclude=exclude)
    if n == 0:
        return run.result()
    st = _lib.stream_ptr(uid.device)
    run.uid[:n].copy_(uid)
    if run.hours is not None:
        if isinstance(hours, torch.Tensor):
            run.hours[:n].copy_(hours)
        else:
            run.hours.fill_(hours)
    run.launch(model, st)
    run.redo_overflow(st)
    _raise_flags(int(run.err.item()), "score_topk")
    return run.result()


def score_topk(model, user_ids: torch.Tensor, k: int = 10, index: Optional[ItemIndex] = None,
               cap: int = 8192, *,
               exclude: Optional[SeenItems] = None, hour=None,
               projection=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k (probability, item id) per user over all items, as
    ``forward_simple(user, all_items)`` + ``nlargest(k)`` would rank them.  Returns
    ``(scores [n, k] fp32, items [n, k] int64)``.  ``exclude``: every user's seen items
    (``SeenItems``, on the index's device): the top k of the others instead, exact by the same
    order; a user with fewer than k unseen items gets trailing ``(0.0, -1)`` slots.
    ``hour``: rank as ``forward_simple(user, all_items, hour)`` does, at one int hour or at one
    hour per user (an integer tensor: the users are grouped by hour, one run per distinct hour,
    the results back in the caller's order).  ``projection``: the hour path's ``nn.Linear(T, D)``
    or ``(weight, bias)`` for the index this call builds (an ``index`` brings its own)."""
    _check_exclude(exclude, model.num_users, model.num_products)
    hour = _check_hour(hour, user_ids.numel())
    index = _resolve_index(model, index, projection, "score_topk")
    dev = index.p.device
    _check_exclude(exclude, model.num_users, model.num_products, dev)
    uid = user_ids.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    n = uid.numel()
    if hour is None or n == 0:
        return _topk_eager(model, uid, k, index, cap, exclude)
    if not isinstance(hour, torch.Tensor):
        return _topk_eager(model, uid, k, index.at_hour(hour), cap, exclude, hour)
    hour = hour.to(device=dev, dtype=torch.int64)
    groups = group_by_hour(hour)
    # (an hour out of range: its group runs at hour 0 and the kernel flags it, which raises)
    view = lambda h: index.at_hour(h if 0 <= h < 24 else 0)   # noqa: E731
    if len(groups) == 1:
        return _topk_eager(model, uid, k, view(groups[0][0]), cap, exclude, hour)
    scores = torch.empty(n, k, device=dev)
    items = torch.empty(n, k, dtype=torch.int64, device=dev)
    for h, pos in groups:
        s, i = _topk_eager(model, uid[pos], k, view(h), cap, exclude, hour[pos])
        scores[pos] = s
        items[pos] = i
    return scores, items


def _check_rank(user_ids, item_ids, num_products: int, exclude=None, index=None):
    """``score_rank``'s arguments before any launch (torch ops on the tensors' own devices: no
    GPU needed): one held-out item per user (ValueError), item ids inside the catalogue
    (IndexError), no held-out item inside its user's history (ValueError, the rule of
    ``full_ranking_metrics``), and an index over the whole catalogue (ValueError for a subset
    index: a place among a shard's items is not the place in the catalogue)."""
    if user_ids.numel() != item_ids.numel():
        raise ValueError(f"score_rank: {user_ids.numel()} users for {item_ids.numel()} held-out "
                         "items (one held-out item per user)")
    if item_ids.is_floating_point() or item_ids.dtype == torch.bool:
        raise TypeError("score_rank: item ids must be integers")
    if index is not None and index.ids is not None:
        raise ValueError("score_rank: the index covers a subset of the catalogue; the place of "
                         "an item is counted over all of it")
    if item_ids.numel() and (int(item_ids.min()) < 0 or int(item_ids.max()) >= num_products):
        raise IndexError("score_rank: item id out of range of the catalogue")
    if exclude is not None and item_ids.numel() and \
            bool(exclude.contains(user_ids, item_ids).any()):
        raise ValueError("score_rank: a held-out item is in its user's history")


def _rank_places(q, p, bias, held, *, seen: Optional[SeenItems] = None, users=None,
                 items_per_block: int = 0, err=None) -> torch.Tensor:
    """The rank kernels (csrc/rank.hip) on raw device tensors: ``q [n, qd]`` query rows,
    ``p [I, qd]`` item rows, ``bias [I]``, ``held [n]`` item ids -> int64 ``[n]``, the number of
    items that beat each row's held-out item, without those in ``seen`` of ``users[r]``.
    ``items_per_block``: the scan's item split (0: chosen by the kernel's entry point).  ``err``:
    the int32 flag word the kernels OR 4 into for an id outside ``[0, I)``.  No host sync."""
    n, qd = q.shape
    I = p.shape[0]
    dev = q.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    if (seen is None) != (users is None):
        raise ValueError("_rank_places: seen and users go together")
    q, p, bias = q.contiguous(), p.contiguous(), bias.contiguous()
    held32 = held.to(device=dev, dtype=torch.int32).contiguous()
    target = torch.empty(n, device=dev)
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    _lib.call("ncf_rank_pair_logits", ptr(q), n, None, ptr(held32), n, ptr(p), ptr(bias), I, qd,
              ptr(target), ptr(err), st)
    _lib.call("ncf_rank_scan", ptr(q), n, ptr(p), ptr(bias), I, qd, ptr(target), ptr(held32),
              int(items_per_block), ptr(count), st)
    if seen is not None:
        uid = users.to(device=dev, dtype=torch.int64).contiguous()
        _lib.call("ncf_rank_seen_correct", ptr(q), n, ptr(held32), ptr(target), ptr(uid),
                  seen.num_users, ptr(seen.offsets), ptr(seen.items), ptr(p), ptr(bias), I, qd,
                  ptr(count), ptr(err), st)
    return count.to(torch.int64)


def score_rank(model, user_ids: torch.Tensor, item_ids: torch.Tensor,
               index: Optional[ItemIndex] = None, *, exclude: Optional[SeenItems] = None,
               hour=None, projection=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact place of one held-out item per user among everything the user has not seen:
    ``place[r] = #{j not in seen(u_r): beats(j)}``, 0-based (``place < k``: in the top k), where
    ``beats(j) = (s_j > s_h and j != h) or (s_j == s_h and j < h)`` is ``score_topk``'s order
    (score desc, item id asc) on the fp32 logits of its factorised scorer.  Returns ``(place
    int64 [n], candidates int64 [n])``, ``candidates = I - len(seen(u_r))``.  One MFMA scan of the
    catalogue that counts (csrc/rank.hip): no k, no candidate lists, no re-runs; HR / NDCG / MRR
    at any k, mean rank and AUC follow from ``place`` (``metrics.ranking_report``).  ``index``,
    ``exclude``, ``hour`` and ``projection`` as in ``score_topk``; the index must cover the whole
    catalogue, and a held-out item inside its user's history is refused."""
    user_ids, item_ids = user_ids.reshape(-1), item_ids.reshape(-1)
    _check_exclude(exclude, model.num_users, model.num_products)
    hour = _check_hour(hour, user_ids.numel())
    _check_rank(user_ids, item_ids, model.num_products, exclude, index)
    index = _resolve_index(model, index, projection, "score_rank")
    dev = index.p.device
    _check_exclude(exclude, model.num_users, model.num_products, dev)
    uid = user_ids.to(device=dev, dtype=torch.int64).contiguous()
    held = item_ids.to(device=dev, dtype=torch.int64).contiguous()
    n = uid.numel()
    if n == 0:
        return (torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    I, qd = index.p.shape
    st = _lib.stream_ptr(dev)
    q = torch.empty(n, qd, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    seen = dict(seen=exclude, users=uid) if exclude is not None else {}
    if hour is None:
        _queries(model, uid, n, q, err, st)
        place = _rank_places(q, index.p, index.bias, held, err=err, **seen)
    else:
        # one query launch for every row (the kernel scales row r by its own hour's s_h); the
        # item bias is per hour, so the rows are ranked in groups of one hour
        hours = hour.to(device=dev, dtype=torch.int64).contiguous() \
            if isinstance(hour, torch.Tensor) else torch.full((n,), hour, dtype=torch.int64,
                                                              device=dev)
        _queries(model, uid, n, q, err, st, hours, index.hour_table())
        groups = group_by_hour(hours)
        place = torch.empty(n, dtype=torch.int64, device=dev)
        for h, pos in groups:
            # (an hour out of range: ranked at hour 0 and flagged by the kernel, which raises)
            bias_h = index.hour_bias(h if 0 <= h < 24 else 0)
            if len(groups) == 1:
                place = _rank_places(q, index.p, bias_h, held, err=err, **seen)
            else:
                sub = dict(seen=exclude, users=uid[pos]) if exclude is not None else {}
                place[pos] = _rank_places(q[pos], index.p, bias_h, held[pos], err=err, **sub)
    _raise_flags(int(err.item()), "score_rank")
    candidates = torch.full((n,), I, dtype=torch.int64, device=dev)
    if exclude is not None:
        candidates -= exclude.lengths[uid]
    return place, candidates


class GraphedScorer:
    """C5 as a captured hipGraph (BASELINE configs[4]): the whole top-k pipeline for a fixed
    number of users (queries, threshold sample GEMM, k-th threshold, MFMA collect, select, and
    the overflow / id-error flags) recorded once with ``torch.cuda.CUDAGraph`` and replayed per
    call, so a call costs one graph launch and one 8-byte flag read instead of the per-launch
    host work.  Users whose candidate list overflowed are re-run eagerly (same results as
    ``score_topk``); a parameter change since capture rebuilds the index and re-captures.

        scorer = GraphedScorer(model, n_users=10_000, k=10)
        scores, items = scorer(user_ids)        # [n, k] each, like score_topk

    The graph writes into static output tensors.  By default a call returns fresh copies of
    them (like ``score_topk``); ``scorer(user_ids, copy=False)`` returns the static tensors
    themselves, which the NEXT call overwrites in place.

    ``exclude`` (``SeenItems``) as in ``score_topk``.  The lists are looked up by user id inside
    the graph, so it holds the CSR's two pointers only and any users can be replayed; users whose
    seen items reach into their top k take the eager re-run after the replay.

    ``hour`` (an int) captures the hour pipeline of ``score_topk(hour=)``; a call then takes
    ``scorer(user_ids, hour=h)``, one int hour per call (default: the last one).  Another hour
    overwrites the scorer's bias buffers in place and replays the same graph.  ``projection``
    as in ``score_topk``.
    """

    def __init__(self, model, n_users: int, k: int = 10, index: Optional[ItemIndex] = None,
                 cap: int = 8192, *, exclude: Optional[SeenItems] = None, hour=None,
                 projection=None):
        self.model, self.n, self.k, self.cap = model, int(n_users), int(k), cap
        if self.n < 1:
            raise ValueError("GraphedScorer needs n_users >= 1")
        _check_exclude(exclude, model.num_users, model.num_products)
        self.exclude = exclude
        # the hour the static buffers hold (None: the hour=None pipeline, captured without them)
        self.hour = None if hour is None else _one_hour(hour, self.n)
        self.index = _resolve_index(model, index, projection, "GraphedScorer")
        self._capture()

    def _capture(self):
        idx = self.index
        dev = idx.p.device
        _check_exclude(self.exclude, self.model.num_users, self.model.num_products, dev)
        if self.hour is not None:
            # the captured kernels read a bias buffer of the scorer's own (and the run's sbias,
            # its sample's rows): _set_hour overwrites both in place, no re-capture per hour
            idx = idx.at_hour(self.hour, bias=idx.hour_bias(self.hour).clone())
        self.run = run = _TopKRun(idx, self.n, self.k, self.cap, exclude=self.exclude)
        run.uid.zero_()
        if self.hour is not None:
            run.hours.fill_(self.hour)
        st = _lib.stream_ptr(dev)
        run.launch(self.model, st)           # warm-up: kernel attributes, lazy module loads
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: other threads' HIP calls (e.g. a process group's watchdog polling its
        # events) stay legal while this thread captures
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            run.launch(self.model, _lib.stream_ptr(dev))
            self.flags = torch.stack([run.overflow[:self.n].amax(), run.err[0]])
            self.out = run.result()
        self.version = self.index.version

    def _set_hour(self, hour: int):
        """Point the captured pipeline at ``hour``: the index's cached bias of that hour into
        the static bias buffer and its sample rows into the run's sbias, the hour into the
        per-user hour buffer (all in place)."""
        run = self.run
        view = run.index
        view.bias.copy_(self.index.hour_bias(hour))
        run.sbias.copy_(view.bias[::run.stride][:run.S])
        run.hours.fill_(hour)
        self.hour = hour

    def __call__(self, user_ids: torch.Tensor, copy: bool = True, *,
                 hour=None) -> Tuple[torch.Tensor, torch.Tensor]:
        uid = user_ids.reshape(-1)
        if hour is not None:
            if self.hour is None:
                raise ValueError("this GraphedScorer was captured for hour=None; build it with "
                                 "hour= to score at an hour")
            hour = _one_hour(hour, uid.numel())
        index = _resolve_index(self.model, self.index, None, "GraphedScorer")
        if index is not self.index:   # rebuilt: the parameters changed since the capture
            self.index = index
            if hour is not None:
                self.hour = hour
            self._capture()
        run = self.run
        if uid.numel() != self.n:
            raise ValueError(f"GraphedScorer was captured for {self.n} users, got {uid.numel()}")
        if hour is not None and hour != self.hour:
            self._set_hour(hour)
        run.uid.copy_(uid)
        run.err.zero_()
        self.graph.replay()
        over, err = self.flags.tolist()
        _raise_flags(err, "score_topk")
        if over:
            run.redo_overflow(_lib.stream_ptr(run.uid.device))
            out = run.result()
        else:
            out = self.out
        return (out[0].clone(), out[1].clone()) if copy else out


def shard_items(num_items: int, world: int, rank: int) -> torch.Tensor:
    """Global item ids of ``rank``'s scoring shard: a contiguous block of the catalogue."""
    per = -(-num_items // world)
    return torch.arange(min(num_items, rank * per), min(num_items, (rank + 1) * per),
                        dtype=torch.int64)


def merge_topk(cand_scores: torch.Tensor, cand_items: torch.Tensor, k: int):
    """Per-user top-k of ``[n, L]`` candidate (score, global item id) lists, ordered by score
    desc then item id asc (empty slots: id < 0).  HIP (ncf_score_merge); GPU only."""
    if cand_scores.device.type != "cuda":
        raise RuntimeError("ncf_amd scoring runs on the MI355X only (no CPU fallback)")
    n, L = cand_scores.shape
    s = cand_scores.to(torch.float32).contiguous()
    it = cand_items.to(torch.int64).contiguous()
    out_s = torch.empty(n, k, device=s.device)
    out_i = torch.empty(n, k, dtype=torch.int64, device=s.device)
    _lib.call("ncf_score_merge", ptr(s), ptr(it), n, L, k, ptr(out_s), ptr(out_i),
              _lib.stream_ptr(s.device))
    return out_s, out_i


def sharded_score_topk(model, user_ids: torch.Tensor, k: int = 10,
                       index: Optional[ItemIndex] = None, group=None, cap: int = 8192,
                       local_topk=None, merge=None, graph: bool = False, *,
                       exclude: Optional[SeenItems] = None, hour=None, projection=None):
    """Item-sharded C5 scoring over ``torch.distributed``: rank r scores every
    queried user against ``shard_items(I, W, r)``, the ``[n, k]`` local lists are all-gathered
    (8 B per entry + id widening) and merged per user.  Every rank returns the global top-k.
    ``local_topk(user_ids, k) -> (scores, global ids)`` and ``merge`` default to the HIP path
    (they are parameters so the collective layout can be exercised on CPU ranks).  ``exclude``
    (``SeenItems``, global item ids, the same on every rank) as in ``score_topk``: each shard
    leaves out the seen items it holds.  ``hour`` / ``projection`` as in ``score_topk`` (with
    ``graph``: one int hour per call); each shard builds the hour's bias over its own items."""
    import torch.distributed as dist
    W = dist.get_world_size(group) if dist.is_initialized() else 1
    r = dist.get_rank(group) if dist.is_initialized() else 0
    if local_topk is None:
        hour = _check_hour(hour, user_ids.numel())
        index = _resolve_index(model, index, projection, "sharded_score_topk",
                               items=lambda: shard_items(model.num_products, W, r))
        kk = min(k, index.p.shape[0])

        def local_topk(u, _k):
            if graph:   # the shard's pipeline as a captured hipGraph (cached on the index)
                gs = index.__dict__.setdefault("_graphed", {})
                # (a scorer keeps its SeenItems alive, so the id in the key stays its own; an
                # hour scorer replays any hour, so the key holds only whether it is one)
                key = (u.numel(), kk, cap) + (() if exclude is None else (id(exclude),)) + \
                    (() if hour is None else ("hour",))
                sc = gs.get(key)
                if sc is None:
                    sc = gs[key] = GraphedScorer(model, u.numel(), kk, index, cap,
                                                 exclude=exclude, hour=hour)
                s, i = sc(u) if hour is None else sc(u, hour=hour)
            else:
                s, i = score_topk(model, u, kk, index, cap, exclude=exclude, hour=hour)
            if kk < _k:   # a shard smaller than k: pad with empty slots
                s = torch.cat([s, s.new_zeros(s.shape[0], _k - kk)], 1)
                i = torch.cat([i, i.new_full((i.shape[0], _k - kk), -1)], 1)
            return s, i
    merge = merge or merge_topk
    s, i = local_topk(user_ids, k)
    if W == 1:
        return s, i      # already the (score desc, item id asc) top-k of the whole catalogue
    gs = [torch.empty_like(s) for _ in range(W)]
    gi = [torch.empty_like(i) for _ in range(W)]
    dist.all_gather(gs, s.contiguous(), group=group)
    dist.all_gather(gi, i.contiguous(), group=group)
    return merge(torch.cat(gs, 1), torch.cat(gi, 1), k)
