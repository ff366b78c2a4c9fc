"""The package's dropout stream restated in plain numpy — TEST INFRASTRUCTURE ONLY.

Restated from the device code, not derived from its output:

* ``csrc/ncf_common.h`` ``ncf_drop_threshold`` / ``ncf_mix32`` / ``ncf_drop_bits`` /
  ``ncf_dropout_scale``: element ``idx`` is kept iff the 16-bit field ``idx & 3`` of the 64 bits
  hashed from ``(seed, idx >> 2)`` is ``>= (uint32)(p * 65536.0f + 0.5f)``; a kept element is
  scaled by ``1.0f / (1.0f - p)`` (fp32), a dropped one is 0.
* ``csrc/mlp_tower_dev.h`` ``make_args`` / ``engine.py`` (per-layer launches): tower layer ``l``
  draws from the seed ``(seed + 0x9E37 * (l + 1)) & (2^63 - 1)``, element index ``row * W + col``.
* ``csrc/attention.hip`` / ``attn_block_dev.h``: the attention weights draw from the unmodified
  seed, flat index ``((b * H + h) * M + i) * M + j``.
* ``csrc/adam.hip`` ``clock_advance``: under the device step clock the seed of a step is the
  clock's; the first step's is the base seed, and after ``t`` advances it is
  ``splitmix64(base_seed + 0x9E3779B97F4A7C15 * (t + 1)) & (2^62 - 1)``.  The kernels add the
  clock's seed to the host's (0 under the clock), so one formula covers both forms.

A property of the stream worth knowing (a note, not a defect the tests hold the kernels to):
the seed enters ``ncf_drop_bits`` only through the 32-bit key ``k``, and the key only through
``i ^ k``.  The bits of seed s' at group g therefore equal the bits of seed s at group
``g ^ (k ^ k')``: the streams of the attention weights and of the tower layers of one step (and
of any two steps) are XOR-permutations of ONE sequence of 2^32 groups.  Over a power-of-two
aligned index range that the permutation maps onto itself the keep rates of all of them are
identical, not merely close.  What the tests assert is the keep rate and the absence of
same-index correlation between the streams one step uses together, nothing stronger.
"""
import numpy as np

M32 = 0xFFFFFFFF
M63 = (1 << 63) - 1
M64 = (1 << 64) - 1
LAYER_STRIDE = 0x9E37
GOLDEN64 = 0x9E3779B97F4A7C15


def mix32(x):
    """ncf_mix32 on a uint64 array holding 32-bit values (products wrapped to 32 bits)."""
    x = np.asarray(x, np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def drop_bits(seed, idx4):
    """ncf_drop_bits: (h0, h1), the low and the high 32 of the 64 bits of float4 group idx4."""
    seed = int(seed) & M64
    idx4 = np.asarray(idx4, np.uint64)
    k = np.uint64(seed & M32) ^ mix32(np.uint64(seed >> 32) ^ (idx4 >> np.uint64(32)))
    i = idx4 & np.uint64(M32)
    return mix32(i ^ k), mix32(i ^ k ^ np.uint64(0x9E3779B9))


def drop_threshold(p):
    """ncf_drop_threshold: (uint32)(p * 65536.0f + 0.5f), in fp32 as the device computes it."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_bits(seed, count, p, start=0):
    """Boolean keep decisions of elements start .. start + count - 1."""
    idx = np.arange(start, start + count, dtype=np.uint64)
    h0, h1 = drop_bits(seed, idx >> np.uint64(2))
    f = idx & np.uint64(3)
    word = np.where(f < 2, h0, h1)
    u = (word >> (np.uint64(16) * (f & np.uint64(1)))) & np.uint64(0xFFFF)
    return u >= np.uint64(drop_threshold(p))


def keep_scales(seed, count, p):
    """ncf_dropout_scale of elements 0 .. count - 1: float32 values in {0, 1 / (1 - p)}."""
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep_bits(seed, count, p), inv_keep, np.float32(0.0)).astype(np.float32)


def layer_seed(seed, l):
    """The seed of tower layer l (0-based) in a step whose seed is ``seed``."""
    return (int(seed) + LAYER_STRIDE * (l + 1)) & M63


def clock_seed(base_seed, t):
    """ncf_step_clock.seed after t advances: the seed of step t + 1 (t = 0: the base seed)."""
    if t == 0:
        return int(base_seed)
    z = (int(base_seed) + GOLDEN64 * (t + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & ((1 << 62) - 1)


def step_masks(seed, B, H, M, widths, p):
    """The oracle's ``dropout_masks`` for one training step of B groups of M rows: ``attn``
    [B, H, M, M] from the step's seed, ``mlp[l]`` [B * M, widths[l]] from layer l's."""
    return {"attn": keep_scales(seed, B * H * M * M, p).reshape(B, H, M, M),
            "mlp": [keep_scales(layer_seed(seed, l), B * M * w, p).reshape(B * M, w)
                    for l, w in enumerate(widths)]}
