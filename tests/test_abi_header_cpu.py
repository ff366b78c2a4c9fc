"""The Python binding is generated from include/ncf_hip.h (_abi.parse_header).  The reader on small
headers written here: every declaration form the header uses parses to the expected type codes,
and a form it does not understand is refused by name, never skipped.  Then the real header: the
ctypes table binds exactly the parsed types, the struct mirrors have the C layout worked out here
from the parsed fields, the built library exports exactly the declared entry points, and the
fast-call extension wraps exactly the entry points it can."""
import ctypes
import os
import subprocess

import pytest

import _ncf_pkg
from tests.conftest import ROOT

ncf = _ncf_pkg.load()
from ncf_amd import _abi, _lib  # noqa: E402

FUNCTIONS, STRUCTS, DEFINES = _abi.parse_header(os.path.join(ROOT, "include", "ncf_hip.h"))


def test_accepted_forms():
    f, s, d = _abi.parse_header(text="""
        /* a block comment with int ncf_ghost(int x); inside */
        #ifndef NCF_HIP_H
        #define NCF_HIP_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define NCF_ERR_ARG (-1)
        #define NCF_LOCK 0x40000000
        #define NCF_MAX_WORLD 64 /* ranks */
        typedef struct ncf_desc {
          const float* part;  /* partial rows */
          int64_t stride;
          int32_t L, cols;
          float scale;
        } ncf_desc;
        typedef struct ncf_list { int32_t count; ncf_desc d[NCF_MAX_WORLD]; } ncf_list;
        typedef struct ncf_recv { int32_t world; int32_t start[NCF_MAX_WORLD + 1]; } ncf_recv;
        typedef struct ncf_pair {
          float *p0, *m0;
          const float *g0, *g1;
          double lr;
        } ncf_pair;
        typedef struct __attribute__((aligned(8))) ncf_cand {
          float logit;
          int32_t item;
        } ncf_cand;
        int ncf_version(void);   // int ncf_ghost2(void);
        const char* ncf_last_error(void);
        int64_t ncf_query(int64_t n, int32_t which, int mode, uint64_t seed, float eps,
                          double lr);
        int ncf_run(const float* x, float* const* grads, void** event, const ncf_list* list,
                    const uint16_t *bf, unsigned long long* sum, const char* name,
                    void* stream);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert f == {"ncf_version": ("i", ()), "ncf_last_error": ("s", ()),
                 "ncf_query": ("l", ("l", "i", "i", "u", "f", "d")), "ncf_run": ("i", ("p",) * 8)}
    assert list(f) == ["ncf_version", "ncf_last_error", "ncf_query", "ncf_run"]   # header order
    assert d == {"NCF_ERR_ARG": -1, "NCF_LOCK": 0x40000000, "NCF_MAX_WORLD": 64}
    assert s == {"ncf_desc": [("part", "p"), ("stride", "l"), ("L", "i"), ("cols", "i"),
                              ("scale", "f")],
                 "ncf_list": [("count", "i"), ("d", ("ncf_desc", 64))],
                 "ncf_recv": [("world", "i"), ("start", ("i", 65))],
                 "ncf_pair": [("p0", "p"), ("m0", "p"), ("g0", "p"), ("g1", "p"), ("lr", "d")],
                 "ncf_cand": [("logit", "f"), ("item", "i")]}
    assert list(s) == ["ncf_desc", "ncf_list", "ncf_recv", "ncf_pair", "ncf_cand"]
    assert s["ncf_cand"].aligned == 8 and s["ncf_desc"].aligned == 0


SEG = "typedef struct ncf_seg { float* data; } ncf_seg;\n"


@pytest.mark.parametrize("text,named", [
    ("int ncf_bad(long n);", "ncf_bad"),                              # unknown scalar types
    ("int ncf_bad(int64_t n, size_t bytes);", "bytes"),
    ("int ncf_bad(unsigned int n);", "ncf_bad"),
    ("void ncf_bad(int n);", "ncf_bad"),
    ("float* ncf_bad(int n);", "ncf_bad"),                            # a pointer result
    ("int ncf_bad(int n, int (*cb)(int), void* stream);", "ncf_bad"),  # function pointers
    ("typedef struct ncf_cb { int (*f)(int); } ncf_cb;", "ncf_cb"),
    (SEG + "int ncf_bad(ncf_seg seg, void* stream);", "seg"),         # structs by value
    (SEG + "ncf_seg ncf_bad(void);", "ncf_bad"),
    ("int ncf_bad(float x[4]);", "ncf_bad"),
    ("typedef struct ncf_bits { int32_t a : 3; int32_t b; } ncf_bits;", "ncf_bits"),  # bit-field
    ("typedef struct ncf_u { union { int a; float b; } u; } ncf_u;", "ncf_u"),
    ("typedef struct ncf_s { long n; } ncf_s;", "ncf_s"),
    ("typedef struct ncf_s { int32_t a[NCF_NOWHERE]; } ncf_s;", r"ncf_s\.a"),
    ("typedef struct ncf_a { int n; } ncf_b;", "ncf_a"),
    ("typedef int ncf_int;", "ncf_int"),
    ("int ncf_bad(int n, int m;\nint ncf_good(void);", "ncf_bad"),    # half-matched declarations
    ("int ncf_bad(int n)", "ncf_bad"),
    ("static inline int ncf_bad(int n) { return n; }\nint ncf_good(void);", "ncf_bad"),
    ("#define NCF_NAME \"x\"", "NCF_NAME"),
    ("#define NCF_SQ(x) ((x) * (x))", "NCF_SQ"),
    ("#if NCF_WIDE\nint ncf_wide(void);\n#endif", "NCF_WIDE"),
])
def test_refused_forms_name_the_declaration(text, named):
    with pytest.raises(_abi.HeaderError, match=named):
        _abi.parse_header(text=text)


def test_every_parsed_function_is_bound_with_the_parsed_types():
    assert len(FUNCTIONS) == 148 and len(STRUCTS) == 11
    assert list(_lib.SIGNATURES) == list(FUNCTIONS)
    for name, (res, args) in FUNCTIONS.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is _abi.CTYPES[res], name
        assert len(got_args) == len(args), name
        assert all(g is _abi.CTYPES[a] for g, a in zip(got_args, args)), name
    # what the codes bind, and a few rows spelled out slot by slot
    assert _abi.CTYPES == {"p": ctypes.c_void_p, "l": ctypes.c_int64, "i": ctypes.c_int32,
                           "f": ctypes.c_float, "d": ctypes.c_double, "u": ctypes.c_uint64,
                           "s": ctypes.c_char_p}
    assert FUNCTIONS["ncf_fill_2d"] == ("i", ("p", "l", "l", "l", "f", "p"))
    assert FUNCTIONS["ncf_step_clock_advance"] == ("i", ("p", "u", "p"))
    assert FUNCTIONS["ncf_grad_clip"] == ("i", ("p", "i", "i", "d", "p", "l", "p", "p"))
    assert FUNCTIONS["ncf_attn_mlp_bwd_workspace"] == ("l", ("l", "i"))
    assert FUNCTIONS["ncf_build_info"] == ("s", ())


def test_limits_come_from_the_header(tmp_path):
    assert (_lib.REDUCE_LIST_MAX, _lib.WGRAD_GROUP_MAX, _lib.GRAD_CLIP_MAX_SEGS,
            _lib.SHARD_MAX_WORLD, _lib.DTYPE_F32, _lib.DTYPE_BF16) == (64, 8, 32, 64, 0, 1)
    from ncf_amd import neighbors, scoring
    assert scoring.KTH_LDS_MAX == DEFINES["NCF_SCORE_KTH_LDS_MAX"] == 38912
    assert scoring.SELECT_MAX == neighbors.MERGE_MAX == DEFINES["NCF_SCORE_SELECT_MAX"] == 8192
    # the header is required at import; the source hash alone tolerates its absence
    with pytest.raises(_lib.NCFLibraryError, match="nowhere.h"):
        _lib._read_header(str(tmp_path / "nowhere.h"))
    assert _abi.src_hash(str(tmp_path / "no_csrc")) == ""


SCALAR_BYTES = {"i": 4, "f": 4, "l": 8, "u": 8, "d": 8, "p": 8}


def c_layout(name):
    """(size, alignment, [(field, offset, size)]) of a parsed struct by the C rules: every field
    at the next multiple of its own alignment, a scalar's alignment its size, an array's its
    element's, the struct's the largest of its fields' (or its aligned(N)), the size rounded up to
    the struct's alignment."""
    def of(t):
        if isinstance(t, tuple):
            size, align = of(t[0])
            return size * t[1], align
        return c_layout(t)[:2] if t in STRUCTS else (SCALAR_BYTES[t], SCALAR_BYTES[t])
    at, biggest, out = 0, max(1, STRUCTS[name].aligned), []
    for field, t in STRUCTS[name]:
        size, align = of(t)
        at = -(-at // align) * align
        out.append((field, at, size))
        at += size
        biggest = max(biggest, align)
    return -(-at // biggest) * biggest, biggest, out


def test_struct_mirrors_have_the_c_layout():
    assert {n: c.__name__ for n, c in _lib._MIRRORS.items()} == {
        "ncf_reduce_desc": "ReduceDesc", "ncf_reduce_list": "ReduceList",
        "ncf_wgrad_desc": "WgradDesc", "ncf_mlp_layer": "MlpLayer", "ncf_head_args": "HeadArgs",
        "ncf_grad_seg": "GradSeg", "ncf_shard_plan_out": "ShardPlanOut",
        "ncf_shard_recv": "ShardRecv", "ncf_table_pair": "TablePair"}
    for name, cls in _lib._MIRRORS.items():
        size, align, fields = c_layout(name)
        assert ctypes.sizeof(cls) == size and ctypes.alignment(cls) == align, name
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size)
                for f, _ in cls._fields_] == fields, name
    # the rule itself: the two structs without a mirror, and sizes known from the C side
    assert c_layout("ncf_score_cand")[:2] == (8, 8) and STRUCTS["ncf_score_cand"].aligned == 8
    assert c_layout("ncf_step_clock") == (16, 8, [("t", 0, 4), ("reserved", 4, 4), ("seed", 8, 8)])
    assert c_layout("ncf_reduce_desc")[0] == 56 and c_layout("ncf_head_args")[0] == 22 * 8
    assert c_layout("ncf_reduce_list")[2][2] == ("d", 8, 56 * 64)


def test_exports_are_exactly_the_declared_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {s for s in (l.split()[-1] for l in out.splitlines() if l.strip())
                if s.startswith("ncf_")}           # the C-linkage names (C++ ones are mangled)
    assert exported - set(FUNCTIONS) == set(), "exported but not declared in the header"
    assert set(FUNCTIONS) - exported == set(), "declared but not exported"


def test_fast_call_names_are_the_wrappable_entry_points():
    from ncf_amd import _ncffast
    names = set(_ncffast.NAMES)
    assert len(names) == len(_ncffast.NAMES) and names <= set(FUNCTIONS), names - set(FUNCTIONS)
    wrappable = {n for n, (res, args) in FUNCTIONS.items()
                 if res in ("i", "l") and set(args) <= set("plifdu")}
    assert wrappable <= names, wrappable - names
    assert set(FUNCTIONS) - wrappable == {"ncf_last_error", "ncf_build_info"}
