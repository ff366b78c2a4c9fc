"""torchrec-compatible sparse input types and the EmbeddingBagCollection used by AdvancedNCF.

The reference imports ``EmbeddingBagCollection, EmbeddingBagConfig, PoolingType`` from torchrec
and ``KeyedJaggedTensor`` from ``torchrec.sparse.jagged_tensor`` (src/model/architecture.py:5-12,
src/model/data_prep.py:5, src/inference/*).  torchrec (0.8.0, Dockerfile:23-25) is not part of
this framework: these classes provide the surface those call sites use —
``KeyedJaggedTensor(keys, values, lengths=None, offsets=None)``, ``.from_lengths_sync``,
``keys() / values() / lengths() / offsets() / to() / to_dict() / __getitem__`` — and an EBC whose
parameters are named ``embedding_bags.<table>.weight`` (the reference state_dict keys).

The EBC forward is the HIP row gather for single-id bags (one row per bag, which is how every
reference call site builds its KJTs: lengths == 1, data_prep.py:273-283, architecture.py:418-422)
and the HIP segmented gather-sum (``pool_rows``, csrc/bag_pool.hip) for every other KJT: bags of
any length, empty ones included, pooled by the table's SUM or MEAN, with per-id weights when the
collection is weighted — what torchrec's EBC does with a jagged feature such as the reference's
purchase history (up to 50 items per customer, src/data/training_data.py:72-81).

Out of scope, and refused loudly: pooled bags through ``AdvancedNCF.forward`` /
``forward_simple`` / ``get_user_embeddings`` / ``get_product_embeddings`` (the reference's forward
takes its batch size from ``values.size(0)``, architecture.py:274-276, and cannot take them
either), bf16 tables, a fused LayerNorm, row-sharded pooled lookups.

``sparse=True`` (``pool_rows`` and a free-standing collection) gives the table a coalesced sparse
(COO) gradient of its touched rows, as ``nn.EmbeddingBag(sparse=True)`` does, for
``ncf_amd.SparseAdam`` (optim.py) or ``torch.optim.SparseAdam``; the default stays dense.
"""
import enum
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib


class PoolingType(enum.Enum):
    SUM = "SUM"
    MEAN = "MEAN"
    NONE = "NONE"


@dataclass
class EmbeddingBagConfig:
    num_embeddings: int
    embedding_dim: int
    name: str = ""
    feature_names: List[str] = field(default_factory=list)
    pooling: PoolingType = PoolingType.SUM
    weight_init_max: Optional[float] = None
    weight_init_min: Optional[float] = None


class JaggedTensor:
    def __init__(self, values: torch.Tensor, lengths: torch.Tensor):
        self._values = values
        self._lengths = lengths

    def values(self):
        return self._values

    def lengths(self):
        return self._lengths

    def offsets(self):
        z = torch.zeros(1, dtype=self._lengths.dtype, device=self._lengths.device)
        return torch.cat([z, torch.cumsum(self._lengths, 0)])


class KeyedJaggedTensor:
    """Keyed jagged ids: ``values`` = concatenation over keys; ``lengths`` has
    ``len(keys) * stride`` entries (per key, one length per bag)."""

    def __init__(self, keys: List[str], values: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                 offsets: Optional[torch.Tensor] = None, weights=None, stride: Optional[int] = None,
                 **kwargs):
        self._keys = list(keys)
        self._values = values
        if lengths is None:
            if offsets is None:
                raise ValueError("KeyedJaggedTensor needs lengths or offsets")
            lengths = offsets[1:] - offsets[:-1]
        self._lengths = lengths
        self._weights = weights
        if stride is None:
            stride = lengths.numel() // max(1, len(self._keys))
        self._stride = stride
        self._length_per_key = None
        self._offset_per_key = None

    @staticmethod
    def from_lengths_sync(keys, values, lengths, weights=None, stride=None):
        return KeyedJaggedTensor(keys, values, lengths=lengths, weights=weights, stride=stride)

    @staticmethod
    def from_offsets_sync(keys, values, offsets, weights=None, stride=None):
        return KeyedJaggedTensor(keys, values, offsets=offsets, weights=weights, stride=stride)

    def keys(self) -> List[str]:
        return self._keys

    def values(self) -> torch.Tensor:
        return self._values

    def lengths(self) -> torch.Tensor:
        return self._lengths

    def offsets(self) -> torch.Tensor:
        z = torch.zeros(1, dtype=self._lengths.dtype, device=self._lengths.device)
        return torch.cat([z, torch.cumsum(self._lengths, 0)])

    def weights_or_none(self):
        return self._weights

    def weights(self) -> torch.Tensor:
        """The per-id weights; raises when the KJT has none (as torchrec does)."""
        if self._weights is None:
            raise ValueError("KeyedJaggedTensor has no weights (weights_or_none() returns None)")
        return self._weights

    def length_per_key(self) -> List[int]:
        """Ids per key (torchrec's name).  Computed once per object; one host read when the
        lengths are on the device (the "sync" of ``from_lengths_sync``)."""
        if self._length_per_key is None:
            k = len(self._keys)
            per = self._lengths.reshape(k, -1).sum(dim=1) if k and self._lengths.numel() else None
            self._length_per_key = [0] * k if per is None else [int(x) for x in per.tolist()]
        return self._length_per_key

    def offset_per_key(self) -> List[int]:
        """Running sum of ``length_per_key()`` with a leading 0: key i owns
        ``values[offset_per_key()[i]:offset_per_key()[i + 1]]`` (torchrec's name)."""
        if self._offset_per_key is None:
            run, out = 0, [0]
            for n in self.length_per_key():
                run += n
                out.append(run)
            self._offset_per_key = out
        return self._offset_per_key

    def is_single_id(self) -> bool:
        """Whether every bag holds exactly one id (the layout ``single_id_split`` takes), checked
        wherever the lengths live: one host read when they are on the device."""
        n = len(self._keys) * self._stride
        if self._values.numel() != n or self._lengths.numel() != n:
            return False
        return n == 0 or bool((self._lengths == 1).all())

    def stride(self) -> int:
        return self._stride

    @property
    def device(self):
        return self._values.device

    def to(self, device, non_blocking: bool = False) -> "KeyedJaggedTensor":
        w = self._weights
        if w is not None:
            w = w.to(device, non_blocking=non_blocking)
        out = KeyedJaggedTensor(self._keys, self._values.to(device, non_blocking=non_blocking),
                                lengths=self._lengths.to(device, non_blocking=non_blocking),
                                weights=w, stride=self._stride)
        out._length_per_key, out._offset_per_key = self._length_per_key, self._offset_per_key
        return out

    def pin_memory(self):
        w = self._weights
        out = KeyedJaggedTensor(self._keys, self._values.pin_memory(),
                                lengths=self._lengths.pin_memory(),
                                weights=None if w is None else w.pin_memory(), stride=self._stride)
        out._length_per_key, out._offset_per_key = self._length_per_key, self._offset_per_key
        return out

    def single_id_split(self) -> Dict[str, torch.Tensor]:
        """{key: ids} for the single-id-bag layout (every length == 1): key k owns
        values[k*stride:(k+1)*stride].  Raises NotImplementedError for pooled bags."""
        n = len(self._keys) * self._stride
        if self._values.numel() != n or self._lengths.numel() != n:
            raise NotImplementedError("AdvancedNCF path supports single-id bags (lengths == 1) only")
        if self._lengths.device.type == "cpu" and n and not bool((self._lengths == 1).all()):
            raise NotImplementedError("AdvancedNCF path supports single-id bags (lengths == 1) only")
        s = self._stride
        return {k: self._values[i * s:(i + 1) * s] for i, k in enumerate(self._keys)}

    def to_dict(self) -> Dict[str, JaggedTensor]:
        out, pos = {}, 0
        cum = torch.cumsum(self._lengths, 0).tolist() if self._lengths.numel() else []
        for i, k in enumerate(self._keys):
            a = i * self._stride
            b = (i + 1) * self._stride
            end = cum[b - 1] if b > 0 and cum else 0
            out[k] = JaggedTensor(self._values[pos:end], self._lengths[a:b])
            pos = end
        return out

    def __getitem__(self, key: str) -> JaggedTensor:
        return self.to_dict()[key]

    def __repr__(self):
        return (f"KeyedJaggedTensor(keys={self._keys}, values={tuple(self._values.shape)}, "
                f"stride={self._stride})")


class _Bag(nn.Module):
    """Holds one table; the parameter is named ``weight`` like nn.EmbeddingBag.

    A deferred dense-exact optimizer (deferred.py) may hold rows of the table behind the step
    count; every read of the table through this module — ``bag.weight``, ``state_dict()`` of
    the bag or of any module above it, the collection's forward — first brings them current
    (``_sync``, installed by the owning AdvancedNCF).  The kernels use ``raw_weight()``."""

    def __init__(self, num_embeddings: int, embedding_dim: int):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self._sync = None
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        self.register_state_dict_pre_hook(_bag_state_dict_pre)

    @property
    def weight(self):
        p = self.__dict__["_parameters"].get("weight")
        if p is None:
            raise AttributeError("weight")
        s = self.__dict__.get("_sync")
        if s is not None:
            s()
        return p

    def raw_weight(self) -> nn.Parameter:
        """The parameter itself, without bringing lagging rows current (kernel plumbing)."""
        return self._parameters["weight"]


def _bag_state_dict_pre(module, prefix, keep_vars):
    s = module.__dict__.get("_sync")
    if s is not None:
        s()


class EmbeddingBagCollection(nn.Module):
    """Drop-in for torchrec.EmbeddingBagCollection.

    ``forward(kjt)`` returns ``{feature: [stride, dim]}``.  A KJT in the single-id layout (every
    length 1: the AdvancedNCF path) is the plain row gather.  Any other KJT is pooled per bag by
    ``pool_rows`` with the table's pooling (SUM or MEAN); empty bags give zero rows; several
    features may share one table.  ``is_weighted=True`` multiplies every row by its id's weight
    (``kjt.weights()``, SUM tables only; ValueError when the KJT has none); a collection that is
    not weighted ignores the KJT's weights, as torchrec does.

    The pooled path is differentiable (dense table gradient, and the weights' gradient) for a
    free-standing collection.  A collection owned by an AdvancedNCF (one with ``set_sync``
    installed) returns tensors without ``grad_fn``, as its single-id forward does: the fused
    optimizer binding owns those tables' gradients.  The model's own forward keeps refusing
    pooled bags.  ``sparse=True``: the pooled path of a free-standing collection gives every
    table a sparse (COO) gradient (``pool_rows(sparse=True)``); two features sharing a table add
    two of them, and autograd's sum may be uncoalesced, as torch's own is.  The single-id gather
    has no gradient and a model-owned collection produces none, so both ignore the flag.  Not
    provided: bf16 tables, a fused LayerNorm, row-sharded pooled lookups."""

    def __init__(self, tables: List[EmbeddingBagConfig], device=None, is_weighted: bool = False,
                 sparse: bool = False):
        super().__init__()
        self._is_weighted = bool(is_weighted)
        self._sparse = bool(sparse)
        self._embedding_bag_configs = list(tables)
        self.embedding_bags = nn.ModuleDict()
        for t in self._embedding_bag_configs:
            if t.pooling not in (PoolingType.SUM, PoolingType.MEAN):
                raise ValueError("EmbeddingBagCollection supports SUM/MEAN pooling")
            bag = _Bag(t.num_embeddings, t.embedding_dim)
            # torchrec default init: U(-sqrt(1/rows), sqrt(1/rows))
            bound = (1.0 / max(1, t.num_embeddings)) ** 0.5
            lo = -bound if t.weight_init_min is None else t.weight_init_min
            hi = bound if t.weight_init_max is None else t.weight_init_max
            with torch.no_grad():
                bag.weight.uniform_(lo, hi)
            self.embedding_bags[t.name] = bag
        if device is not None:
            self.to(device)

    def embedding_bag_configs(self):
        return self._embedding_bag_configs

    def table_for(self, feature: str) -> _Bag:
        for t in self._embedding_bag_configs:
            if feature in t.feature_names:
                return self.embedding_bags[t.name]
        raise KeyError(feature)

    def is_weighted(self) -> bool:
        return self._is_weighted

    def forward(self, features: KeyedJaggedTensor) -> Dict[str, torch.Tensor]:
        weights = None
        if self._is_weighted:
            weights = features.weights_or_none()
            if weights is None:
                raise ValueError("EmbeddingBagCollection(is_weighted=True) needs a "
                                 "KeyedJaggedTensor with weights")
            if any(t.pooling == PoolingType.MEAN for t in self._embedding_bag_configs):
                raise ValueError(_MEAN_WEIGHTS)
        if weights is None and features.is_single_id():
            ids = features.single_id_split()
            out = {}
            for t in self._embedding_bag_configs:
                bag = self.embedding_bags[t.name]
                for f in t.feature_names:
                    if f in ids:
                        out[f] = gather_rows(bag.weight, ids[f])   # (.weight: rows current)
            return out
        return self._forward_pooled(features, weights)

    def _forward_pooled(self, features: KeyedJaggedTensor, weights) -> Dict[str, torch.Tensor]:
        keys, stride = features.keys(), features.stride()
        values, lengths = features.values(), features.lengths()
        if values.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        opk = features.offset_per_key()        # (one host read, cached on the KJT)
        out = {}
        for t in self._embedding_bag_configs:
            bag = self.embedding_bags[t.name]
            mode = "mean" if t.pooling == PoolingType.MEAN else "sum"
            for f in t.feature_names:
                if f not in keys:
                    continue
                i = keys.index(f)
                z = torch.zeros(1, dtype=torch.int64, device=values.device)
                off = torch.cat([z, torch.cumsum(lengths[i * stride:(i + 1) * stride].to(
                    device=values.device, dtype=torch.int64), 0)])
                w = None if weights is None else weights[opk[i]:opk[i + 1]]
                owned = bag._sync is not None
                table = bag.weight             # (.weight: rows current)
                if owned:   # the fused optimizer binding owns this table's gradient
                    with torch.no_grad():
                        out[f] = pool_rows(table.detach(), values[opk[i]:opk[i + 1]], off, w, mode)
                else:
                    out[f] = pool_rows(table, values[opk[i]:opk[i + 1]], off, w, mode,
                                       sparse=self._sparse)
        return out

    def set_sync(self, fn):
        """Install the callable that brings lagging table rows current before a read."""
        for bag in self.embedding_bags.values():
            bag._sync = fn


_NO_CPU = ("ncf_amd: the AdvancedNCF path runs on the GPU only (no CPU fallback); "
           "move the model to cuda")
_MEAN_WEIGHTS = "per-id weights are for SUM pooling only (mode 'mean' takes no weights)"

# Occurrences of one id that one lane group sums in the pooled backward before the partial sums
# are added in chunk order (csrc/segments.h NCF_PIECE, the dedup's piece length; chunks are cut
# at sorted positions that are multiples of it)
BAG_BWD_CHUNK = 16

_MODES = {"sum": 0, "mean": 1}


class _PoolRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, weights, ids, offsets, mode, check, sparse=False):
        ctx.sparse = sparse
        t = table.detach()
        bags = offsets.numel() - 1
        out = torch.empty(bags, t.shape[1], device=t.device, dtype=torch.float32)
        err = torch.zeros(1, dtype=torch.int32, device=t.device) if check else None
        w = None if weights is None else weights.detach()
        _lib.call("ncf_bag_pool_fwd", _lib.ptr(ids), ids.numel(), _lib.ptr(offsets), bags,
                  _lib.ptr(w), _lib.ptr(t), t.shape[0], t.shape[1], mode, _lib.ptr(out),
                  _lib.ptr(err), _lib.stream_ptr(t.device))
        if check:
            flag = int(err.item())
            if flag & 1:
                raise IndexError("embedding id out of range")
            if flag & 2:
                raise ValueError("pool_rows: offsets must ascend within [0, ids.numel()]")
        ctx.save_for_backward(t, w, ids, offsets)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, grad_out):
        t, w, ids, offsets = ctx.saved_tensors
        need_t, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and w is not None
        if not (need_t or need_w):
            return None, None, None, None, None, None, None
        g = grad_out.to(torch.float32).contiguous()
        n, bags, dim = ids.numel(), offsets.numel() - 1, t.shape[1]
        compact = need_t and ctx.sparse
        if compact:     # one row per unique id at most: O(n), whatever the table's height
            gt = torch.empty(max(1, min(n, t.shape[0])), dim, device=t.device, dtype=torch.float32)
        else:
            gt = torch.empty_like(t) if need_t else None    # (zero-filled by the call)
        gw = torch.empty(n, device=t.device, dtype=torch.float32) if need_w else None
        ws = torch.empty(_lib.query("ncf_bag_pool_bwd_workspace", n, bags, dim), dtype=torch.uint8,
                         device=t.device)
        mode = ctx.mode | (_lib.BAG_COMPACT if compact else 0)
        _lib.call("ncf_bag_pool_bwd", _lib.ptr(ids), n, _lib.ptr(offsets), bags, _lib.ptr(w),
                  _lib.ptr(t) if need_w else None, _lib.ptr(g), t.shape[0], dim, mode,
                  _lib.ptr(gt), _lib.ptr(gw), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(t.device))
        if compact:
            # the call's output block at the head of its workspace (include/ncf_hip.h): the one
            # host read of the sparse backward, then copies of the U ids so the workspace goes
            c0, i0 = _lib.BAG_WS_COUNT_OFFSET, _lib.BAG_WS_IDS_OFFSET
            u = int(ws[c0:c0 + 4].view(torch.int32).item())
            idx = ws[i0:i0 + 8 * u].view(torch.int64).clone().unsqueeze(0)
            gt = torch.sparse_coo_tensor(idx, gt[:u], t.shape, is_coalesced=True)
            # A sparse gradient that autograd's AccumulateGrad can steal is rebuilt there from its
            # indices and values without the coalesced flag; one that is referenced elsewhere is
            # cloned, flag kept (and to exactly U rows).  Hold it until the graph goes, so that
            # ``table.grad.is_coalesced()``.
            ctx.keep = gt
        return gt, gw, None, None, None, None, None


def pool_rows(table: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, weights=None,
              mode: str = "sum", check: bool = True, sparse: bool = False) -> torch.Tensor:
    """HIP pooled lookup, the functional form beside ``gather_rows``:
    ``out[b] = scale_b * sum_{p in [offsets[b], offsets[b+1])} weights[p] * table[ids[p]]`` for
    ``offsets`` of ``bags + 1`` entries relative to ``ids`` (``nn.functional.embedding_bag`` with
    ``include_last_offset=True``).  ``mode`` "sum" (scale 1) or "mean" (scale 1 / bag length);
    an empty bag is a zero row; ``weights`` (per id, "sum" only: ValueError with "mean", the rule
    embedding_bag enforces) default to 1.  An unweighted bag of one id is bitwise
    ``gather_rows`` of that id.  fp32 table of width 16, 32, 64, 128 or 256, on the GPU only.

    Differentiable: the gradient to ``table`` is dense ``[rows, dim]`` (what torchrec's unsharded
    EBC / ``nn.EmbeddingBag(sparse=False)`` produce), bitwise reproducible (no float atomics; one
    id's terms are added in sorted-position order, in chunks of ``BAG_BWD_CHUNK``); ``weights``
    get theirs when they require grad; only what is asked for is computed.  No bf16 tables, no
    fused LayerNorm.

    ``sparse=True`` (``nn.EmbeddingBag(sparse=True)``): the gradient to ``table`` is a coalesced
    ``torch.sparse_coo_tensor`` of ``table.shape`` instead: indices ``[1, U]``, the unique ids
    ascending, values ``[U, dim]``, row for row the bits the dense gradient holds there
    (``grad.to_dense()`` is the dense path's gradient bitwise).  The backward then touches memory
    proportional to ``ids.numel()`` and never to the table's height (no ``[rows, dim]`` buffer,
    no zero-fill), and reads ``U`` from the device once per backward, whatever ``check`` is.  An
    id none of whose positions lies in a bag is listed with a zero row; an id out of range
    (``check=False``) is not listed, and makes row 0 listed (a zero row unless real positions name
    it).  Everything else is as without it.  ``ncf_amd.SparseAdam`` and
    ``torch.optim.SparseAdam`` step such gradients.

    ``check=True`` reads the kernel's flag once: IndexError for an id outside the table,
    ValueError for offsets that decrease or leave ``[0, ids.numel()]`` (the kernel clamps: nothing
    is read out of bounds either way).  ``check=False`` does no host read."""
    if mode not in _MODES:
        raise ValueError(f"pool_rows: mode must be 'sum' or 'mean', not {mode!r}")
    if weights is not None and mode == "mean":
        raise ValueError(_MEAN_WEIGHTS)
    if table.device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    if table.dtype != torch.float32 or table.dim() != 2:
        raise ValueError("pool_rows: the table must be a 2-d float32 tensor (bf16 tables are not "
                         "supported)")
    if not table.is_contiguous():
        raise ValueError("pool_rows: the table must be contiguous")
    ids = ids.to(device=table.device, dtype=torch.int64).contiguous()
    offsets = offsets.to(device=table.device, dtype=torch.int64).contiguous()
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("pool_rows: offsets needs bags + 1 entries")
    if weights is not None:
        weights = weights.to(device=table.device, dtype=torch.float32).contiguous()
        if weights.numel() != ids.numel():
            raise ValueError("pool_rows: one weight per id")
    return _PoolRows.apply(table, weights, ids.reshape(-1), offsets, _MODES[mode], bool(check),
                           bool(sparse))


def gather_rows(table: torch.Tensor, ids: torch.Tensor, gamma=None, beta=None, eps=1e-5) -> torch.Tensor:
    """HIP row gather (+ optional LayerNorm); rows of ``table`` at int64 ``ids``."""
    if table.device.type != "cuda":
        raise RuntimeError(_NO_CPU)
    ids = ids.to(device=table.device, dtype=torch.int64).contiguous()
    table = table.detach()
    out = torch.empty(ids.numel(), table.shape[1], device=table.device, dtype=torch.float32)
    err = torch.zeros(1, dtype=torch.int32, device=table.device)
    _lib.call("ncf_gather_rows", _lib.ptr(ids), ids.numel(), _lib.ptr(table), table.shape[0],
              table.shape[1], _lib.ptr(gamma), _lib.ptr(beta), eps, _lib.ptr(out), _lib.ptr(err),
              _lib.stream_ptr(table.device))
    if int(err.item()):
        raise IndexError("embedding id out of range")
    return out
