"""The C-ABI of libncf_hip.so as include/ncf_hip.h declares it, and the library's build identity
(stdlib only, no torch import: build_ext.sh runs it before anything else).

``parse_header()`` reads the header: every entry point's result and argument types, the structs'
fields and the integer ``#define NCF_*`` limits.  It is the only description of the C-ABI on the
Python side: ``_lib`` builds its ctypes table, struct mirrors and limits from it, and
``csrc/gen_fastcall.py`` the fast-call wrappers.  A declaration it does not understand is an
error (``HeaderError``), never a skipped row.

Two hashes are compiled into the library (``ncf_build_info()``, include/ncf_hip.h) and checked by
``_lib.load()`` before any entry point is bound:

* ``abi``: the entry points of the header (names, result and argument types, in order).  A
  library built from another header would take its arguments in the wrong slots; it is refused.
* ``src``: the kernel sources the library was compiled from (``csrc/*.hip``, ``csrc/*.h``,
  ``include/ncf_hip.h``).  A library older or newer than the sources beside it — rebuilt while a
  GPU call waited in the queue, or not rebuilt after an edit — is refused too (when the sources
  are present; an installed package without them skips this half).

    python _abi.py abi      # the hash of the header's entry points
    python _abi.py src [DIR]  # the hash of the sources (DIR: another csrc tree, A/B builds)
"""
import ctypes
import hashlib
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "ncf_hip.h"))

# type codes: the scalar types the header may pass by value, "p" any pointer, "s" a
# `const char*` result
SCALARS = {"int": "i", "int32_t": "i", "int64_t": "l", "uint64_t": "u", "float": "f",
           "double": "d"}
CTYPES = {"p": ctypes.c_void_p, "l": ctypes.c_int64, "i": ctypes.c_int, "f": ctypes.c_float,
          "d": ctypes.c_double, "u": ctypes.c_uint64, "s": ctypes.c_char_p}
_CODE = {t: c for c, t in CTYPES.items()}


class HeaderError(ValueError):
    """A declaration of the header that parse_header does not understand."""


class StructFields(list):
    """[(field name, type)] of one struct; ``aligned``: its __attribute__((aligned(n))) or 0."""
    aligned = 0


# ([const] base [const]) ([* [const]]...) [name] [[bound]]
_DECL = re.compile(r"((?:const\s+)?(?:unsigned\s+long\s+long|\w+)(?:\s+const)?)\s*"
                   r"((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(?:\[([^\]]*)\])?")
_STRUCT = re.compile(r"typedef\s+struct\s+(?:__attribute__\s*\(\(aligned\((\d+)\)\)\)\s*)?"
                     r"(\w+)\s*\{(.*)\}\s*(\w+)", re.S)
_FUNC = re.compile(r"([^()]*?)(\w+)\s*\((.*)\)", re.S)


def _int_expr(text, defines, where):
    """An integer literal, a define, or a sum of them (one pair of outer parentheses allowed)."""
    text = text.strip()
    text = text[1:-1] if text.startswith("(") and text.endswith(")") else text
    try:
        return sum(defines[t] if t in defines else int(t, 0)
                   for t in (t.strip() for t in text.split("+")))
    except ValueError:
        raise HeaderError(f"{where}: cannot evaluate {text!r}") from None


def _declarator(text, where, structs, defines):
    """(name or None, type, type prefix) of one declarator; a type is a scalar code, "p", the
    name of a struct parsed before, or (type, count) for an array."""
    text = " ".join(text.split())
    odd = "function pointer" if "(" in text else "bit-field" if ":" in text else ""
    m = None if odd else _DECL.fullmatch(text)
    if not m:
        raise HeaderError(f"{where}: cannot parse {odd or 'declarator'} {text!r}")
    prefix, stars, name, bound = m.groups()
    base = " ".join(w for w in prefix.split() if w != "const")
    if stars:
        t = "s" if (base, stars.strip()) == ("char", "*") else "p"
    elif base in SCALARS or base in structs:
        t = SCALARS.get(base, base)
    else:
        raise HeaderError(f"{where}: unknown scalar type {base!r} in {text!r}")
    if bound is not None:
        t = (t, _int_expr(bound, defines, f"{where}.{name}"))
    return name, t, prefix


def _function(stmt, structs):
    m = _FUNC.fullmatch(stmt)
    if not m:
        raise HeaderError(f"cannot parse declaration {' '.join(stmt.split())[:80]!r}")
    result, name, arglist = m.groups()
    extra, res, _ = _declarator(result, name, structs, {})
    if extra is not None or res not in ("i", "l", "u", "f", "d", "s"):
        raise HeaderError(f"{name}: result {result.strip()!r} is neither a scalar nor const char*")
    if "(" in arglist:
        raise HeaderError(f"{name}: function-pointer argument or unterminated declaration")
    args = []
    for a in [] if arglist.split() == ["void"] else arglist.split(","):
        arg, t, _ = _declarator(a, name, structs, {})
        if t == "s":
            t = "p"
        if t not in CTYPES:
            raise HeaderError(f"{name}: argument {arg} ({' '.join(a.split())!r}) is a struct by "
                              f"value or an array")
        args.append(t)
    return name, (res, tuple(args))


def _struct(stmt, structs, defines):
    m = _STRUCT.fullmatch(stmt)
    if not m or m.group(2) != m.group(4):
        raise HeaderError(f"cannot parse typedef {' '.join(stmt.split())[:80]!r}")
    aligned, name, body, _ = m.groups()
    fields = StructFields()
    fields.aligned = int(aligned or 0)
    *decls, rest = body.split(";")
    if rest.strip():
        raise HeaderError(f"{name}: field {rest.strip()!r} without ';'")
    for decl in decls:
        first, *more = decl.split(",")     # `float *p0, *m0`: the type prefix is the first one's
        prefix = _declarator(first, name, structs, defines)[2]
        for d in [first] + [f"{prefix} {x}" for x in more]:
            field, t, _ = _declarator(d, name, structs, defines)
            if field is None:
                raise HeaderError(f"{name}: field without a name in {' '.join(decl.split())!r}")
            fields.append((field, "p" if t == "s" else t))
    return name, fields


def parse_header(path=HEADER, text=None):
    """(functions, structs, defines) of the header (or of ``text``), each a dict in header order:
    functions: name -> (result code, tuple of argument codes);
    structs:   name -> StructFields [(field, type)], a type being a scalar code, "p", an
               (element type, count) array or the name of a struct parsed before it;
    defines:   the integer ``#define NCF_*`` values."""
    if text is None:
        with open(path) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'#ifdef __cplusplus\s*(extern "C" \{|\})\s*#endif', " ", text)
    functions, structs, defines = {}, {}, {}
    code = []
    for line in text.split("\n"):
        d = " ".join(line.replace("#", "# ", 1).split())
        m = re.fullmatch(r"# define (NCF_\w+) (.+)", d)
        if m:
            defines[m.group(1)] = _int_expr(m.group(2), defines, m.group(1))
        elif d.startswith("#") and not re.fullmatch(
                r"# (ifndef \w+|define \w+|include <\w+\.h>|endif)", d):
            raise HeaderError(f"cannot parse directive {line.strip()!r}")
        code.append("" if d.startswith("#") else line)
    # a statement ends at a ';' outside braces
    *stmts, rest = re.split(r";(?![^{}]*\})", "\n".join(code))
    if rest.strip():
        raise HeaderError(f"unterminated declaration {' '.join(rest.split())[:80]!r}")
    for stmt in (s.strip() for s in stmts):
        if stmt.startswith("typedef"):
            name, fields = _struct(stmt, structs, defines)
            structs[name] = fields
        else:
            name, types = _function(stmt, structs)
            functions[name] = types
    return functions, structs, defines


def signatures(functions):
    """name -> (ctypes result type, [ctypes argument types]) of the parsed functions."""
    return {n: (CTYPES[r], [CTYPES[a] for a in args]) for n, (r, args) in functions.items()}


def abi_hash(signatures) -> str:
    text = ";".join(f"{n}:{_CODE[r]}:{''.join(_CODE[a] for a in args)}"
                    for n, (r, args) in signatures.items())
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def source_files(csrc: str = CSRC):
    if not os.path.isdir(csrc):
        return []
    fs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc)
                if f.endswith((".hip", ".h")))
    if os.path.exists(HEADER):
        fs.append(HEADER)
    return fs


def src_hash(csrc: str = CSRC) -> str:
    """'' when the sources are not present."""
    fs = source_files(csrc)
    if not fs:
        return ""
    h = hashlib.sha256()
    for f in fs:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    return h.hexdigest()[:16]


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "abi"
    print(abi_hash(signatures(parse_header()[0])) if what == "abi"
          else src_hash(sys.argv[2] if len(sys.argv) > 2 else CSRC))
