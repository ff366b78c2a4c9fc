"""The stochastic rounding of the bf16 tables restated in plain numpy — TEST INFRASTRUCTURE ONLY.

Restated from the device code's definition, not derived from its output:

* ``csrc/ncf_common.h`` ``ncf_sr_base`` / ``ncf_sr_key`` / ``ncf_sr_bits``: the store of step
  ``s`` on element ``e = row * D + col`` of table ``j`` (0: GMF, 1: MLP) of pair ``kind`` (0:
  users, 1: items) under ``seed`` (32 bits) draws

      base = mix32(seed ^ 0x9E3779B9 * (2 * (e >> 32) + kind + 1))
      key  = mix32(base + s)
      h    = mix32((uint32)e * 0x9E3779B9 ^ key)
      r    = h & 0xFFFF  (j = 0)   or   h >> 16  (j = 1)

  with ``ncf_mix32`` as ``tests/dropout_stream.py`` restates it, everything modulo 2^32.
* ``ncf_sr_round``: the stored bf16 is ``(bits_of(x) + r) >> 16`` of the fp32 result ``x``; a
  NaN takes ``r = 0`` (its high half: what nearest-even stores for the quiet NaNs arithmetic
  produces).  Inf + r stays inf; the largest finite magnitudes may carry into inf.

``word`` / ``bits`` / ``store`` are the vectorised forms; ``word_scalar`` / ``store_scalar`` the
same in Python integers, one element at a time (tests/test_sr_stream_cpu.py holds the two
together).  ``adam_sr`` is the stand-in the GPU tests' premises are measured with: the fp32 CPU
Adam of tests/adam_ref.py with the restated store in the kernel's place.
"""
import numpy as np

from tests import adam_ref as A
from tests.dropout_stream import mix32

M32 = 0xFFFFFFFF
GOLDEN32 = 0x9E3779B9
U64 = np.uint64


def _mix32_scalar(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def word_scalar(seed, kind, step, e):
    """The 32 bits of element e at step `step` of pair `kind`, in Python integers."""
    base = _mix32_scalar((seed & M32) ^ ((GOLDEN32 * (2 * (e >> 32) + kind + 1)) & M32))
    key = _mix32_scalar((base + step) & M32)
    return _mix32_scalar((((e & M32) * GOLDEN32) & M32) ^ key)


def store_scalar(x, r):
    """The bf16 bit pattern stored for the fp32 value x (a numpy float32) under the 16 bits r."""
    b = int(np.float32(x).view(np.uint32))
    if (b & 0x7FFFFFFF) > 0x7F800000:       # NaN
        r = 0
    return ((b + r) & M32) >> 16


def word(seed, kind, step, e):
    """ncf_sr_bits of elements e (any integer array, < 2^63): uint64 array of 32-bit values."""
    e = np.asarray(e, U64)
    pre = (U64(GOLDEN32) * ((U64(2) * (e >> U64(32)) + U64(kind + 1)) & U64(M32))) & U64(M32)
    base = mix32(U64(int(seed) & M32) ^ pre)
    key = mix32((base + U64(int(step) & M32)) & U64(M32))
    return mix32((((e & U64(M32)) * U64(GOLDEN32)) & U64(M32)) ^ key)


def bits(seed, kind, j, step, e):
    """The 16 uniform bits r of the contract (include/ncf_hip.h)."""
    h = word(seed, kind, step, e)
    return (h >> U64(16)) if j else (h & U64(0xFFFF))


def store(x, r):
    """bf16 bit patterns (uint16) of the fp32 array x under the 16-bit values r."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(U64)
    nan = (b & U64(0x7FFFFFFF)) > U64(0x7F800000)
    r = np.where(nan, U64(0), np.asarray(r, U64))
    return (((b + r) & U64(M32)) >> U64(16)).astype(np.uint16)


def widen(h16):
    """fp32 values of bf16 bit patterns."""
    return (np.asarray(h16, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def sr_round(x, seed, kind, j, step, e0=0):
    """x [rows, D] fp32 (elements e0 + row * D + col) rounded as the device stores it."""
    x = np.ascontiguousarray(x, np.float32)
    e = np.arange(x.size, dtype=np.uint64).reshape(x.shape) + U64(e0)
    return widen(store(x, bits(seed, kind, j, step, e)))


def nearest(x):
    """fp32 -> bf16 to nearest even, widened (the dtype-1 store; finite values)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(U64)
    b = b + U64(0x7FFF) + ((b >> U64(16)) & U64(1))
    return widen(((b & U64(M32)) >> U64(16)).astype(np.uint16))


def neighbours(x64):
    """(lo, hi, spacing) float64: the bf16 values next below / above |x| in magnitude, signed as x;
    lo == hi == x where bf16 holds x (x finite, within the fp32 range)."""
    x64 = np.asarray(x64, np.float64)
    a = np.abs(x64)
    sub = a < 2.0 ** -126                              # bf16 subnormals: spacing 2^-133
    _, ex = np.frexp(np.where(sub, 1.0, a))            # a = m * 2^ex, m in [0.5, 1)
    spacing = np.where(sub, 2.0 ** -133, np.ldexp(1.0, ex - 8))   # 8 significant bits at a
    lo = np.floor(a / spacing) * spacing
    hi = np.where(lo == a, lo, lo + spacing)
    s = np.where(np.signbit(x64), -1.0, 1.0)
    return s * lo, s * hi, spacing


def adam_sr(p, m, v, g, has, lr, t, hp, seed, kind, j, e0=0, rd=None):
    """Step t of one [rows, D] table in fp32 (tests/adam_ref.py: adam_step for the rows with a
    gradient, ``has``; zero_step_folded for the others), the parameter stored through the
    restated stochastic rounding (``rd``: another store, e.g. ``nearest``, for mutants)."""
    s = A.make_scalars(lr, hp, t)
    a = A.adam_step(p, m, v, g, None, None, None, A.F32, s=s)
    b = A.zero_step_folded(p, m, v, s, A.F32)
    pp, mm, vv = (np.where(np.asarray(has)[:, None], x, y).astype(np.float32) for x, y in zip(a, b))
    pp = rd(pp) if rd is not None else sr_round(pp, seed, kind, j, t, e0)
    return pp, mm, vv
