"""Exact nearest-product search over the exported embeddings.

The reference's production API ranks by vector search: ``get_user_embedding(features)`` and
``product_search.find_neighbors(user_embedding, k, category_filter)`` (src/inference/api.py:63-73)
against a Vertex Tree-AH index built with ``COSINE_DISTANCE`` over the L2-normalised ``"mlp"``
product vectors (setup_tree_ah_endpoint.py:25-32, generate_embeddings.py:193-221).  ``export.py``
writes that index's input; ``ProductSearch`` answers the query itself, exactly instead of
approximately: cosine top-k with the API's category filter, from one HIP scan of the matrix
(csrc/neighbors.hip, ``ncf_nn_scan``) and the per-slab lists merged by ``ncf_score_merge``.

It is named after the reference's ``src.inference.vector_search.ProductSearch``, which api.py
imports and the reference tree does not contain.  GPU only; no CPU fallback.

Slab plan (``plan``): the catalogue is cut into contiguous slabs, one workgroup per slab and block
of 32 queries, each writing its slab's exact top k per query; at least two workgroups per CU where
the catalogue allows, no slab below 1024 items.  The lists are merged in one ``ncf_score_merge``
when ``n_slabs * k <= 8192``, else in two levels (groups of ``g2`` slabs, then the ``g1`` groups).
A similarity is the same bits whatever the plan: the kernel's accumulation order is fixed.
"""
from collections import namedtuple
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ptr
from .engine import LN_EPS

K_MAX = 128            # ncf_nn_scan keeps up to 128 keys per query and slab
DIMS = (16, 32, 64, 128)
QUERY_BLOCK = 32       # queries per workgroup (the MFMA's 32 rows)
NUM_CUS = 256
MIN_SLAB = 1024
MERGE_MAX = _lib.DEFINES["NCF_SCORE_SELECT_MAX"]   # ncf_score_merge's longest candidate list

Plan = namedtuple("Plan", "slab_items n_slabs g1 g2")
Plan.__doc__ = """``n_slabs`` slabs of ``slab_items`` items cover the catalogue (the last one may be
short); the kernel is launched over ``g1 * g2 >= n_slabs`` slabs, the ones past the catalogue
empty, and merged as ``g1`` groups of ``g2`` (``g1 == 1``: one level)."""


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def plan(n_items: int, k: int, slab_items: Optional[int] = None, query_blocks: int = 1) -> Plan:
    """Host arithmetic only.  ``slab_items`` forces the slab size (tests); ``query_blocks`` (blocks
    of 32 queries in the call) counts towards the two workgroups per CU, so a large batch takes
    fewer, longer slabs and shorter merges."""
    _check_k(k)
    n_items, query_blocks = int(n_items), max(1, int(query_blocks))
    if n_items < 1:
        raise ValueError("plan: the catalogue is empty")
    lists = MERGE_MAX // k             # lists of k one merge level takes (>= 64)
    if slab_items is None:
        want = _cdiv(2 * NUM_CUS, query_blocks)
        slab = max(MIN_SLAB, _cdiv(n_items, want), _cdiv(n_items, lists * lists))
    else:
        slab = int(slab_items)
        if slab < 1:
            raise ValueError("slab_items must be >= 1")
        if _cdiv(n_items, slab) > lists * lists:
            raise ValueError(f"slab_items={slab} gives {_cdiv(n_items, slab)} slabs, more than "
                             f"two merge levels take at k={k} ({lists * lists})")
    n_slabs = _cdiv(n_items, slab)
    g1 = _cdiv(n_slabs, lists)
    g2 = _cdiv(n_slabs, g1)
    return Plan(slab, n_slabs, g1, g2)


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("k must be an int")
    if not 1 <= k <= K_MAX:
        raise ValueError(f"k={k} is outside [1, {K_MAX}]")
    return k


def _check_dim(dim: int) -> int:
    if dim not in DIMS:
        raise ValueError(f"the search kernel takes D = 16, 32, 64 or 128, not {dim}")
    return dim


def _int_tensor(name: str, t, n: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or \
            t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor")
    t = t.reshape(-1)
    if t.numel() != n:
        raise ValueError(f"{name} holds {t.numel()} entries for {n} {what}")
    return t


def _check_categories(categories, n_items: int):
    """``categories=`` of an index: None, or one integer >= 0 per indexed product."""
    if categories is None:
        return None
    cat = _int_tensor("categories", categories, n_items, "indexed products")
    if cat.numel() and (int(cat.min()) < 0 or int(cat.max()) >= 2 ** 31):
        raise ValueError("categories must lie in [0, 2^31)")
    return cat


def _check_filter(category_filter, n: int, has_categories: bool):
    """``category_filter=``: None, an int (negative: no filter) or an integer tensor with one
    entry per query (-1 = no filter); returned as None, an int, or the flat tensor."""
    if category_filter is None:
        return None
    if not has_categories:
        raise ValueError("category_filter needs an index built with categories=")
    if isinstance(category_filter, torch.Tensor) and category_filter.dim() > 0:
        return _int_tensor("category_filter", category_filter, n, "queries")
    if isinstance(category_filter, (bool, float)) or \
            (isinstance(category_filter, torch.Tensor) and
             (category_filter.is_floating_point() or category_filter.dtype == torch.bool)):
        raise TypeError("category_filter must be an int or an integer tensor")
    c = int(category_filter)
    if c >= 2 ** 31:
        raise ValueError("category_filter must lie below 2^31")
    return c


def _check_skip(skip, n: int):
    """``skip=``: None, or an integer tensor of global item ids, one per query (-1 = none)."""
    if skip is None:
        return None
    return _int_tensor("skip", skip, n, "queries")


def _check_queries(queries, dim: int) -> torch.Tensor:
    if not isinstance(queries, torch.Tensor) or not queries.is_floating_point():
        raise TypeError("queries must be a floating-point tensor")
    if queries.dim() == 1:
        queries = queries.unsqueeze(0)
    if queries.dim() != 2 or queries.shape[1] != dim:
        raise ValueError(f"queries must be [n, {dim}] or [{dim}], not {tuple(queries.shape)}")
    return queries


def _no_cpu(device, what: str):
    if device.type != "cuda":
        raise RuntimeError(f"ncf_amd {what} runs on the MI355X only (no CPU fallback)")


class ProductSearch:
    """Exact cosine search over one set of L2-normalised product vectors.

    ``ProductSearch(model, ...)`` indexes the model's ``"mlp"`` (or ``table="mf"``) product
    vectors, the rows ``export.product_embeddings(model, ids, normalize=True)`` returns, for the
    model's current parameters (``valid_for``); ``from_vectors`` indexes any ``[I, D]`` matrix,
    for example one read back with ``export.read_embeddings_jsonl``."""

    def __init__(self, model, categories: Optional[torch.Tensor] = None,
                 items: Optional[torch.Tensor] = None, table: str = "mlp"):
        """``items``: the global product ids to index (default: the whole catalogue).
        ``categories``: one integer >= 0 per indexed product, for ``category_filter=``."""
        from .export import product_embeddings
        from .scoring import _param_version
        if table not in ("mlp", "mf"):
            raise ValueError("table must be 'mlp' or 'mf'")
        dev = model.mlp_norm.weight.device
        _no_cpu(dev, "product search")
        I = model.num_products
        if items is None:
            ids, own = torch.arange(I, dtype=torch.int64, device=dev), None
        else:
            ids = _int_tensor("items", items, items.numel() if isinstance(items, torch.Tensor)
                              else 0, "items").to(
                device=dev, dtype=torch.int64).contiguous()
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= I):
                raise IndexError("ProductSearch: item id out of range of the embedding table")
            own = ids
        if ids.numel() == 0:
            raise ValueError("ProductSearch: nothing to index")
        cat = _check_categories(categories, ids.numel())
        width = (model.mlp_embedding_collection if table == "mlp" else
                 model.mf_embedding_collection).embedding_bags["product_id"].weight.shape[1]
        _check_dim(width)
        self._set(product_embeddings(model, ids, normalize=True, table=table), own, cat)
        self.model = model
        self.table = table
        self.version = _param_version(model)

    def _set(self, vectors, ids, categories):
        self.vectors = vectors                 # [I, D] fp32 unit rows, on the device
        self.dim = vectors.shape[1]
        self.ids = ids                         # global ids of the rows (None: the positions)
        self.categories = None if categories is None else \
            categories.to(device=vectors.device, dtype=torch.int32).contiguous()
        self.model = None
        self.version = None
        self._pos = None                       # global id -> position (built on first use)

    @classmethod
    def from_vectors(cls, vectors: torch.Tensor, ids: Optional[torch.Tensor] = None,
                     categories: Optional[torch.Tensor] = None) -> "ProductSearch":
        """Index the rows of an ``[I, D]`` matrix.  The rows are L2-normalised on load (a zero
        row stays zero: similarity 0 to every query); a non-finite row raises ``ValueError``.
        ``ids``: the rows' global item ids (distinct, >= 0), default their positions."""
        if not isinstance(vectors, torch.Tensor) or not vectors.is_floating_point():
            raise TypeError("vectors must be a floating-point tensor")
        if vectors.dim() != 2 or vectors.shape[0] < 1:
            raise ValueError("vectors must be a non-empty [I, D] matrix")
        I, D = vectors.shape
        _check_dim(D)
        cat = _check_categories(categories, I)
        if ids is not None:
            ids = _int_tensor("ids", ids, I, "rows")
        _no_cpu(vectors.device, "product search")
        dev = vectors.device
        v = vectors.detach().to(torch.float32).contiguous()
        if not bool(torch.isfinite(v).all()):
            raise ValueError("vectors holds a non-finite row")
        if ids is not None:
            ids = ids.to(device=dev, dtype=torch.int64).contiguous()
            if int(ids.min()) < 0 or ids.unique().numel() != I:
                raise ValueError("ids must be distinct and >= 0")
        rows = torch.arange(I, dtype=torch.int64, device=dev)
        out = torch.empty_like(v)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("ncf_embedding_export", ptr(rows), I, ptr(v), I, D, None, None, LN_EPS, 1,
                  ptr(out), ptr(err), _lib.stream_ptr(dev))
        out = torch.where((v != 0).any(dim=1, keepdim=True), out, v)   # (0 / 0: the zero rows)
        self = cls.__new__(cls)
        self._set(out, ids, cat)
        return self

    def valid_for(self, model) -> bool:
        """Whether the index still holds ``model``'s vectors (no parameter changed since)."""
        from .scoring import _param_version
        return self.model is not None and model is self.model and \
            self.version == _param_version(model)

    @property
    def num_items(self) -> int:
        return self.vectors.shape[0]

    def _positions(self, item_ids: torch.Tensor) -> torch.Tensor:
        """Index positions of global item ids (-1: not in the index)."""
        ids = item_ids.to(device=self.vectors.device, dtype=torch.int64)
        I = self.num_items
        if self.ids is None:
            return torch.where((ids >= 0) & (ids < I), ids, torch.full_like(ids, -1))
        if self._pos is None:
            pos = torch.full((int(self.ids.max()) + 1,), -1, dtype=torch.int64,
                             device=self.ids.device)
            pos[self.ids] = torch.arange(I, dtype=torch.int64, device=self.ids.device)
            self._pos = pos
        inside = (ids >= 0) & (ids < self._pos.numel())
        return torch.where(inside, self._pos[ids.clamp(0, self._pos.numel() - 1)],
                           torch.full_like(ids, -1))

    def find_neighbors(self, queries: torch.Tensor, k: int = 10, category_filter=None,
                       skip: Optional[torch.Tensor] = None, *,
                       slab_items: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``k`` products most similar to each query: ``(similarity [n, k] fp32, items
        [n, k] int64)``, ordered by similarity desc then item id asc, global ids.

        ``queries``: ``[n, D]`` or ``[D]`` fp32, normalised on the device (a zero query stays
        zero).  The similarity is the cosine; the index's cosine *distance* is ``1 -
        similarity`` and is not returned.  ``category_filter``: None, an int, or an integer
        tensor with one entry per query (-1 = no filter): only products of that category.
        ``skip``: an integer tensor of global item ids to leave out, one per query (-1 = none).
        A query with fewer than ``k`` matches gets trailing ``(0.0, -1)`` slots, as in
        ``score_topk``; so does every slot of a query holding a NaN.  ``slab_items`` forces the
        slab size (tests)."""
        k = _check_k(k)
        q = _check_queries(queries, self.dim)
        n = q.shape[0]
        cf = _check_filter(category_filter, n, self.categories is not None)
        sk = _check_skip(skip, n)
        dev = self.vectors.device
        _no_cpu(dev, "product search")
        _no_cpu(q.device, "product search")
        if q.device != dev:
            raise ValueError(f"queries are on {q.device}, the index on {dev}")
        pl = plan(self.num_items, k, slab_items, _cdiv(max(n, 1), QUERY_BLOCK))
        out_s = torch.empty(n, k, device=dev)
        out_i = torch.empty(n, k, dtype=torch.int64, device=dev)
        if n == 0:
            return out_s, out_i
        q = q.detach().to(torch.float32).contiguous()
        qcat = None
        if isinstance(cf, int):
            if cf >= 0:     # (a negative int: no filter)
                qcat = torch.full((n,), cf, dtype=torch.int32, device=dev)
        elif cf is not None:
            qcat = cf.to(device=dev, dtype=torch.int64).clamp(-1, 2 ** 31 - 1).to(
                torch.int32).contiguous()
        qskip = None if sk is None else self._positions(sk).contiguous()
        st = _lib.stream_ptr(dev)
        slabs = pl.g1 * pl.g2
        part_s = torch.empty(n, slabs, k, device=dev)
        part_i = torch.empty(n, slabs, k, dtype=torch.int64, device=dev)
        _lib.call("ncf_nn_scan", ptr(q), n, 1, ptr(self.vectors), self.num_items, self.dim,
                  ptr(self.categories) if qcat is not None else None, ptr(qcat), ptr(qskip),
                  pl.slab_items, slabs, k, ptr(part_s), ptr(part_i), st)
        if pl.g1 > 1:     # groups of g2 slabs first: (query, group) is the merge's "user"
            mid_s = torch.empty(n, pl.g1, k, device=dev)
            mid_i = torch.empty(n, pl.g1, k, dtype=torch.int64, device=dev)
            _lib.call("ncf_score_merge", ptr(part_s), ptr(part_i), n * pl.g1, pl.g2 * k, k,
                      ptr(mid_s), ptr(mid_i), st)
            part_s, part_i, slabs = mid_s, mid_i, pl.g1
        _lib.call("ncf_score_merge", ptr(part_s), ptr(part_i), n, slabs * k, k, ptr(out_s),
                  ptr(out_i), st)
        if self.ids is not None:
            out_i = torch.where(out_i < 0, out_i, self.ids[out_i.clamp_min(0)])
        return out_s, out_i

    def find_neighbors_of_users(self, user_ids: torch.Tensor, k: int = 10, category_filter=None):
        """``find_neighbors`` of the users' LayerNorm'd embedding rows (the ``"mlp"`` vectors
        ``model.get_user_embeddings`` returns, or ``"mf"`` for a ``table="mf"`` index); a user
        id out of range raises ``IndexError``."""
        from .sparse import gather_rows
        if self.model is None:
            raise ValueError("find_neighbors_of_users needs an index built from a model")
        m = self.model
        k = _check_k(k)
        uid = _int_tensor("user_ids", user_ids, user_ids.numel()
                          if isinstance(user_ids, torch.Tensor) else 0, "users")
        cf = _check_filter(category_filter, uid.numel(), self.categories is not None)
        m._engine.sync_tables()
        coll, ln = ((m.mlp_embedding_collection, m.mlp_norm) if self.table == "mlp" else
                    (m.mf_embedding_collection, m.mf_norm))
        q = gather_rows(coll.embedding_bags["user_id"].weight, uid, ln.weight, ln.bias, LN_EPS)
        return self.find_neighbors(q, k, cf)

    def similar_products(self, product_ids: torch.Tensor, k: int = 10, category_filter=None):
        """The ``k`` nearest products of each of ``product_ids`` (global ids), the product itself
        left out; a product that is not in the index raises ``IndexError``."""
        k = _check_k(k)
        pid = _int_tensor("product_ids", product_ids, product_ids.numel()
                          if isinstance(product_ids, torch.Tensor) else 0, "products")
        cf = _check_filter(category_filter, pid.numel(), self.categories is not None)
        pid = pid.to(device=self.vectors.device, dtype=torch.int64)
        pos = self._positions(pid)
        if bool((pos < 0).any()):
            raise IndexError("similar_products: a product is not in the index")
        return self.find_neighbors(self.vectors[pos], k, cf, skip=pid)
