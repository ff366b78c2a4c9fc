"""Global gradient-norm clipping for AdvancedNCF (src/model/trainer.py:278-283).

The reference trainer is written to call ``torch.nn.utils.clip_grad_norm_(self.model.parameters(),
config['gradient_clipping'])`` between ``loss.backward()`` and ``optimizer.step()``.  On this
package's model torch's function is silently wrong: after a backward the four embedding tables
hold no ``.grad`` (their gradients are the compact rows of the engine's pending workspace), torch
skips parameters without one, and so it returns the norm of the dense parameters alone and leaves
the table gradients unscaled.  ``clip_grad_norm_`` here is the one-line replacement: the norm over
the compact rows (their count read on the device), the flat dense gradient buffer and every other
dense ``.grad`` among the parameters, and the scale of all of them in place, in two launches of
``ncf_grad_clip`` (csrc/grad_clip.hip) with no host synchronisation.
"""
import ctypes
import math

import torch

from . import _lib
from . import optim as _optim
from ._lib import ptr

_NONFINITE = ("The total norm of order {} for gradients from `parameters` is non-finite, so it "
              "cannot be clipped. To disable this error and scale the gradients by the non-finite "
              "norm anyway, set `error_if_nonfinite=False`")


def _norm_kind(norm_type) -> int:
    nt = float(norm_type)
    if nt == 2.0:
        return 0
    if nt == math.inf:
        return 1
    raise NotImplementedError(f"ncf_amd.clip_grad_norm_: norm_type {norm_type!r} (2 or inf)")


def _dense_segment(g, what):
    if not g.is_cuda:
        raise RuntimeError(f"ncf_amd.clip_grad_norm_: {what} has a CPU gradient (HIP kernels, no "
                           "CPU fallback)")
    if g.dtype != torch.float32 or g.layout != torch.strided:
        raise RuntimeError(f"ncf_amd.clip_grad_norm_: {what} has a {g.dtype} {g.layout} gradient "
                           "(dense fp32 only)")
    if not g.is_contiguous():
        raise RuntimeError(f"ncf_amd.clip_grad_norm_: {what} has a non-contiguous gradient")
    return (g, None, 1, g.numel())


def table_segments(w, keys=("mf_user", "mlp_user", "mf_item", "mlp_item")):
    """The compact table gradients of workspace ``w`` (engine.pending) as segments: w.G[key]
    [n, width] fp32 with the first num_unique[kind] rows valid, the count read on the device."""
    segs = []
    for key in keys:
        G = w.G[key]
        cnt = w.num_unique
        if w.split is not None and key.startswith("mf"):
            cnt = w.split["num_unique"]     # (split widths: the MF collection's own dedup)
        kind = 0 if key.endswith("user") else 1
        segs.append((G, cnt.data_ptr() + 4 * kind, G.shape[0], G.shape[1]))
    return segs


def _model_segments(m, ids, handled):
    """The segments of one live AdvancedNCF whose tables are among the parameters: the compact
    rows of its pending backward and, when every dense gradient is the flat buffer's view, that
    buffer as one segment.  ``handled`` receives the id() of the parameters they cover."""
    eng = m.engine
    tables = eng.table_params()
    segs = []
    w = eng.pending
    if w is not None and getattr(w, "sent_rows", False):
        raise NotImplementedError("ncf_amd.clip_grad_norm_: the row-sharded step's table gradients "
                                  "are already in its send buffer (a global norm across ranks is "
                                  "not supported)")
    if w is not None and any(p.requires_grad and p.grad is not None for p in tables.values()):
        # dense table .grad (accumulation) and pending rows: one dense gradient, as the
        # optimizer binding makes it
        eng.materialize_table_grads(accumulate=True)
        w = None
    if w is not None:
        handled.update(id(p) for p in tables.values())
        segs += table_segments(w, [k for k, p in tables.items() if p.requires_grad])
    # (grad_views: the dense parameters with their views of the flat buffer, cached by the
    # engine — dense_params() walks the modules, 40 us of host time a call)
    views = eng.grad_views() if eng.flat_grad is not None else ()
    if views and all(p.grad is gv and id(p) in ids for p, gv in views):
        handled.update(id(p) for p, _ in views)
        segs.append((eng.flat_grad, None, 1, eng.flat_grad.numel()))
    return segs


def _module_params(mod):
    """list(mod.parameters()); for an AdvancedNCF kept between calls (the walk over its modules is
    ~90 us of host time, on a step that is host-bound) and taken again whenever the engine
    re-validates its parameter layout (a parameter moved or re-assigned: ensure_layout)."""
    eng = mod.__dict__.get("_engine")
    key = getattr(eng, "_layout_key", None)
    if key is None:
        return list(mod.parameters())
    c = mod.__dict__.get("_clip_params")
    if c is None or c[0] is not key:
        c = mod.__dict__["_clip_params"] = (key, list(mod.parameters()))
    return c[1]


def _segments(parameters):
    """[(tensor, device count pointer or None, rows, dim)] over everything that holds a
    gradient, and the device of the first parameter."""
    if isinstance(parameters, torch.Tensor):
        params = [parameters]
    elif isinstance(parameters, torch.nn.Module):
        params = _module_params(parameters)
    else:
        params = list(parameters)
    ids = {id(p) for p in params}
    handled = set()
    segs = []
    for m in list(_optim._models):
        eng = m.engine
        if eng.flat is None or not eng.flat.is_cuda:
            continue
        if all(id(p) in ids for p in eng.table_params().values()):
            segs += _model_segments(m, ids, handled)
    for i, p in enumerate(params):
        if id(p) in handled:
            continue
        handled.add(id(p))
        if not p.requires_grad or p.grad is None:
            continue           # as torch skips them
        if p.grad.numel():
            segs.append(_dense_segment(p.grad, f"parameter {i} {tuple(p.shape)}"))
    if len(segs) > _lib.GRAD_CLIP_MAX_SEGS:
        raise ValueError(f"ncf_amd.clip_grad_norm_: {len(segs)} gradient segments, at most "
                         f"{_lib.GRAD_CLIP_MAX_SEGS} (pass the parameters of one model)")
    devs = {s[0].device for s in segs}
    if len(devs) > 1:
        raise RuntimeError(f"ncf_amd.clip_grad_norm_: gradients on several devices {devs}")
    dev = devs.pop() if devs else (params[0].device if params else torch.device("cpu"))
    return segs, dev


def seg_array(segs):
    """ncf_grad_seg[len(segs)] of (tensor, count pointer, rows, dim) tuples."""
    arr = (_lib.GradSeg * max(1, len(segs)))()
    for a, (t, cnt, rows, dim) in zip(arr, segs):
        a.data, a.rows_dev, a.rows, a.dim = ptr(t), cnt, rows, dim
    return arr


_workspaces = {}


def _workspace(dev, nbytes):
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _workspaces[dev] = torch.empty(max(64, (nbytes + 7) // 8), dtype=torch.float64,
                                            device=dev)
    return ws


def run(segs, kind, max_norm, dev, ws=None):
    """ncf_grad_clip over the segments on the current stream of ``dev``; returns the device
    tensor {norm, coefficient}.  ``ws``: a float64 workspace of the caller's (a captured step keeps
    its own)."""
    arr = seg_array(segs)
    addr = ctypes.addressof(arr)
    need = _lib.query("ncf_grad_clip_workspace", addr, len(segs))
    if ws is None or ws.numel() * 8 < need:
        ws = _workspace(dev, need)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.call("ncf_grad_clip", addr, len(segs), kind, float(max_norm), ptr(ws), ws.numel() * 8,
              ptr(out), _lib.stream_ptr(dev))
    return out


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for parameters that include an AdvancedNCF's: the total norm
    covers the tables' pending compact gradients too, and every gradient is multiplied by
    ``min(1, max_norm / (total_norm + 1e-6))`` in place.  ``parameters``: an AdvancedNCF, or an
    iterable of parameters (``model.parameters()``).  Returns the total norm as a 0-dim fp32
    device tensor; nothing synchronises the host unless ``error_if_nonfinite`` (which reads the
    norm before anything is scaled).  ``norm_type`` 2 or inf; ``foreach`` is accepted and has no
    meaning here (one launch pair covers every gradient)."""
    kind = _norm_kind(norm_type)
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError(f"ncf_amd.clip_grad_norm_: max_norm must be > 0, got {max_norm}")
    segs, dev = _segments(parameters)
    if not segs:
        return torch.zeros((), dtype=torch.float32, device=dev)
    if error_if_nonfinite:
        total = run(segs, kind, math.inf, dev)[0]
        if not math.isfinite(float(total)):
            raise RuntimeError(_NONFINITE.format(norm_type))
    return run(segs, kind, max_norm, dev)[0]


def grad_norm(parameters, norm_type=2.0):
    """The total gradient norm ``clip_grad_norm_`` would return, without scaling anything."""
    kind = _norm_kind(norm_type)
    segs, dev = _segments(parameters)
    if not segs:
        return torch.zeros((), dtype=torch.float32, device=dev)
    return run(segs, kind, math.inf, dev)[0]
