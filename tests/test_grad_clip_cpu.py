"""CPU-only checks of the gradient-clipping C-ABI (grad_clip.hip, include/ncf_hip.h): the layout
of ncf_grad_seg, the exported symbols, and the host-side
arithmetic and refusals of the entry points (everything that returns before a launch)."""
import ctypes
import os
import re
import subprocess

import pytest

import _ncf_pkg
from tests.conftest import ROOT

ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ncf_hip.h")
NAMES = ("ncf_grad_clip_chunk", "ncf_grad_clip_workspace", "ncf_grad_clip")


def _header():
    return open(HEADER).read()


def test_grad_seg_mirror_matches_header():
    """Field order of the header's typedef (the mirror is built from it); every field 8 bytes (two
    pointers, two int64), so the offsets are 0, 8, 16, 24 and the size 32."""
    hdr = _header()
    body = hdr[hdr.index("typedef struct ncf_grad_seg"):hdr.index("} ncf_grad_seg;")]
    names = [f[0] for f in _lib.GradSeg._fields_]
    assert names == ["data", "rows_dev", "rows", "dim"]
    assert [getattr(_lib.GradSeg, n).offset for n in names] == [0, 8, 16, 24]
    assert ctypes.sizeof(_lib.GradSeg) == 32
    assert re.search(r"const int32_t\*\s*rows_dev;", body) and re.search(r"float\*\s*data;", body)
    assert f"#define NCF_GRAD_CLIP_MAX_SEGS {_lib.GRAD_CLIP_MAX_SEGS}" in hdr


def test_symbols_exported_and_signature_arity():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NAMES:
        assert name in syms, name
    # the fast-call binding carries them too (generated from the header)
    _lib.load()
    assert all(n in _lib.FAST for n in NAMES)


def _segs(shapes, data=64):
    arr = (_lib.GradSeg * max(1, len(shapes)))()
    for a, (rows, dim) in zip(arr, shapes):
        a.data, a.rows_dev, a.rows, a.dim = data, None, rows, dim
    return arr


def test_workspace_query_is_chunks_of_each_capacity():
    """8 bytes (one fp64 partial) per chunk of ncf_grad_clip_chunk() floats of every segment's
    capacity, each segment rounded up on its own."""
    chunk = _lib.query("ncf_grad_clip_chunk")
    assert chunk >= 256 and chunk % 256 == 0
    shapes = [(40, 64), (20480, 64), (24, 7), (1, 3 * chunk + 1), (0, 16)]
    want = sum(-(-(r * d) // chunk) for r, d in shapes)
    arr = _segs(shapes)
    assert _lib.query("ncf_grad_clip_workspace", ctypes.addressof(arr), len(shapes)) == 8 * want
    assert _lib.query("ncf_grad_clip_workspace", None, 0) == 8
    assert _lib.query("ncf_grad_clip_workspace", ctypes.addressof(arr), 33) == 0


@pytest.mark.parametrize("nsegs,kind,max_norm", [(1, 0, 0.0), (1, 0, -1.0), (1, 0, float("nan")),
                                                 (33, 0, 1.0), (-1, 0, 1.0), (1, 2, 1.0)])
def test_refusals_before_any_launch(nsegs, kind, max_norm):
    arr = _segs([(4, 4)] * 33)
    with pytest.raises(_lib.NCFArgumentError):
        _lib.call("ncf_grad_clip", ctypes.addressof(arr), nsegs, kind, max_norm, 64, 1 << 20, 64,
                  None)


def test_bad_segment_and_small_workspace():
    lib = _lib.load()
    for shape, data in (((4, 0), 64), ((-1, 4), 64), ((4, 4), 0), ((4, 4), 66)):
        arr = _segs([shape], data)
        with pytest.raises(_lib.NCFArgumentError):
            _lib.call("ncf_grad_clip", ctypes.addressof(arr), 1, 0, 1.0, 64, 1 << 20, 64, None)
    arr = _segs([(1, 3 * _lib.query("ncf_grad_clip_chunk"))])
    assert lib.ncf_grad_clip(ctypes.addressof(arr), 1, 0, 1.0, 64, 16, 64, None) == -3
