"""The float64 restatement of the nearest-product search that test_neighbors_cpu.py checks
against a brute force and test_gpu_neighbors.py compares ``ProductSearch`` with (not a test
module).

    sim = V64 @ (q64 / |q64|)         over the index's own fp32 rows, widened
    masked by category and skip
    argsort(-sim, stable)[:k]          (similarity desc, then position asc)

Tolerance (derived): with unit rows and a unit query sum |a_i b_i| <= 1, so the fp32 accumulation
of D terms plus the query's normalisation stay within ``atol(D) = (D + 8) * 2^-24``."""
import numpy as np


def atol(dim: int) -> float:
    return (dim + 8) * 2.0 ** -24


def restate(V, q, k, cat=None, qcat=None, skip=None):
    """``V`` [I, D], ``q`` [n, D] (any float dtype); ``cat`` [I] with ``qcat`` [n] (< 0: no
    filter); ``skip`` [n] positions (< 0: none).  Returns ``(sim [n, I] float64, mask [n, I] bool,
    ids)``: ``ids[r]`` the positions of query r's top ``min(k, matches)`` in order."""
    V64 = np.asarray(V, dtype=np.float64)
    q64 = np.asarray(q, dtype=np.float64)
    nrm = np.sqrt((q64 * q64).sum(axis=1, keepdims=True))
    qn = np.where(nrm > 0, q64 / np.where(nrm > 0, nrm, 1.0), q64)
    sim = qn @ V64.T
    n, I = sim.shape
    mask = np.ones((n, I), dtype=bool)
    if qcat is not None:
        qc = np.asarray(qcat).reshape(-1, 1)
        mask &= (qc < 0) | (np.asarray(cat).reshape(1, -1) == qc)
    if skip is not None:
        for r, s in enumerate(np.asarray(skip).tolist()):
            if 0 <= s < I:
                mask[r, s] = False
    ids = []
    for r in range(n):
        order = np.argsort(-sim[r], kind="stable")
        ids.append(order[mask[r][order]][:k])
    return sim, mask, ids


def check(got_sim, got_ids, sim, mask, ids, k, tol, report=None):
    """``got_*`` [n, k] (positions) against ``restate``'s output: ids equal except where the
    reference similarities of the differing entries lie within ``2 tol`` of each other,
    similarities within ``tol`` of the reference value of the returned id, filter membership and
    skip exact, unused slots ``(0.0, -1)``.  ``report``: a list that receives the largest
    similarity error seen."""
    got_sim, got_ids = np.asarray(got_sim), np.asarray(got_ids)
    assert got_sim.shape == got_ids.shape == (len(ids), k)
    worst = 0.0
    for r, exp in enumerate(ids):
        m = len(exp)
        assert (got_ids[r, m:] == -1).all() and (got_sim[r, m:] == 0.0).all(), r
        g = got_ids[r, :m]
        assert (g >= 0).all() and len(set(g.tolist())) == m, r
        assert mask[r][g].all(), f"query {r}: an item outside its filter came back"
        err = np.abs(got_sim[r, :m].astype(np.float64) - sim[r][g])
        if m:
            worst = max(worst, float(err.max()))
        assert (err <= tol).all(), (r, float(err.max()), tol)
        d = g != exp
        assert (np.abs(sim[r][g[d]] - sim[r][exp[d]]) <= 2 * tol).all(), \
            f"query {r}: ids differ beyond a tie: {g[d][:5]} != {exp[d][:5]}"
        key = list(zip((-got_sim[r, :m]).tolist(), g.tolist()))
        assert key == sorted(key), f"query {r}: not ordered by (similarity desc, id asc)"
    if report is not None:
        report.append(worst)
