"""The float64 restatement of the pooled lookup (``ncf_amd.sparse.pool_rows``) that
test_bag_pool_cpu.py checks against ``torch.nn.functional.embedding_bag`` and test_gpu_bag_pool.py
compares the HIP kernels with (not a test module), and the case list both run on.

    out[b]   = scale_b * sum_{p in bag b} w_p * table[ids[p]]      scale_b = 1 (sum), 1/L_b (mean)
    gtab[r]  = sum_{p : ids[p] = r} scale_b(p) * w_p * G[b(p)]
    gw[p]    = <G[b(p)], table[ids[p]]>

Bounds (derived, element-wise; fp32 summation of n terms in ANY order is within
(n - 1) u sum|terms| + O(u^2) of the exact sum, u = 2^-24; each term's own products and the
mean's reciprocal and scaling add at most 3 more roundings of relative size u, and the float64
restatement itself is exact to ~1e-16):

    forward   |err| <= (L_b + 4) u scale_b sum_p |w_p x_p|
    gtab      |err| <= (c_r + 4) u sum |terms|          c_r = occurrences of row r
    gw        |err| <= (dim + 4) u sum_d |g x|
"""
import numpy as np

U24 = 2.0 ** -24
ROWS = 1000
DIMS = (16, 32, 64, 128, 256)
BAGS = 67
# every length the kernel treats differently: empty (first, last, two in a row), around the
# 4-row in-flight unroll, around a wave's width, and one long bag
LENGTHS_HEAD = [0, 1, 2, 3, 4, 5, 0, 0, 63, 64, 65, 200]


def make_case(dim, hot_count, seed=0):
    """One ragged case: dict of numpy arrays ``table`` f32 [ROWS, dim], ``ids`` i64, ``offsets``
    i64 [BAGS + 1], ``lengths``, ``weights`` f32 (N(0, 1) with exact zeros and negatives), ``C``
    f32 [BAGS, dim] (the loss's fixed multiplier), ``hot`` (an id with ``hot_count`` occurrences
    across bags)."""
    rng = np.random.RandomState(1000 * seed + dim)
    lengths = LENGTHS_HEAD + rng.randint(0, 13, size=BAGS - len(LENGTHS_HEAD) - 1).tolist() + [0]
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.size == BAGS
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(offsets[-1])
    assert n < 8192
    hot = 7
    ids = rng.randint(8, ROWS - 1, size=n).astype(np.int64)      # (never 0, hot or ROWS - 1)
    b5 = int(offsets[5])                                          # the bag of 5: one id twice
    ids[b5 + 1] = ids[b5 + 3] = 4
    where = np.asarray([p for p in rng.permutation(n) if p not in (b5 + 1, b5 + 3)])
    ids[where[:hot_count]] = hot
    ids[where[hot_count]] = 0
    ids[where[hot_count + 1]] = ROWS - 1
    assert int((ids == hot).sum()) == hot_count
    table = rng.standard_normal((ROWS, dim)).astype(np.float32)
    weights = rng.standard_normal(n).astype(np.float32)
    weights[where[-5:]] = 0.0
    assert (weights < 0).any()
    C = rng.standard_normal((BAGS, dim)).astype(np.float32)
    return dict(dim=dim, table=table, ids=ids, offsets=offsets, lengths=lengths, weights=weights,
                C=C, hot=hot, hot_count=hot_count)


def _bag_of(offsets, n):
    bag = np.full(n, -1, dtype=np.int64)
    for b in range(offsets.size - 1):
        bag[offsets[b]:offsets[b + 1]] = b
    return bag


def _coef(offsets, n, weights, mode):
    bag = _bag_of(offsets, n)
    lengths = np.diff(offsets).astype(np.float64)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    if mode == "mean":
        w = w / lengths[bag]
    return bag, w


def forward(table, ids, offsets, weights=None, mode="sum"):
    """(out [bags, dim] float64, bound [bags, dim]): the pooled rows and the forward bound."""
    T = np.asarray(table, dtype=np.float64)
    n, bags = ids.size, offsets.size - 1
    bag, w = _coef(offsets, n, weights, mode)
    terms = T[ids] * w[:, None]
    out = np.zeros((bags, T.shape[1]))
    mag = np.zeros_like(out)
    np.add.at(out, bag, terms)
    np.add.at(mag, bag, np.abs(terms))
    L = np.diff(offsets).astype(np.float64)
    return out, (L[:, None] + 4) * U24 * mag


def grad_table(rows, ids, offsets, G, weights=None, mode="sum"):
    """(gtab [rows, dim] float64, bound, count [rows]) for upstream gradient ``G`` [bags, dim]."""
    G64 = np.asarray(G, dtype=np.float64)
    bag, w = _coef(offsets, ids.size, weights, mode)
    terms = G64[bag] * w[:, None]
    gt = np.zeros((rows, G64.shape[1]))
    mag = np.zeros_like(gt)
    np.add.at(gt, ids, terms)
    np.add.at(mag, ids, np.abs(terms))
    count = np.bincount(ids, minlength=rows).astype(np.float64)
    return gt, (count[:, None] + 4) * U24 * mag, count


def grad_weights(table, ids, offsets, G):
    """(gw [n] float64, bound [n]) of SUM pooling."""
    T = np.asarray(table, dtype=np.float64)
    G64 = np.asarray(G, dtype=np.float64)
    bag = _bag_of(offsets, ids.size)
    prod = G64[bag] * T[ids]
    return prod.sum(axis=1), (T.shape[1] + 4) * U24 * np.abs(prod).sum(axis=1)


def within(got, want, bound):
    """Largest ``|got - want| - bound`` (<= 0 when every element is inside its bound) and the
    largest error over its bound where the bound is positive."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return float((err - bound).max()) if err.size else 0.0, ratio
