"""The embedding end of the step restated in plain torch on the CPU — TEST INFRASTRUCTURE ONLY.

Restated from the reference module's definition (four single-id EmbeddingBag lookups,
nn.LayerNorm(D) on each, the GMF Linear(D, 1) of LN(u) * LN(i); backward = LayerNorm backward
followed by the dense embedding backward's index_add), not derived from the kernels' output.
Every function takes ``dtype``: float64 is the reference, float32 the yardstick a bound is
measured with (tests/test_embed_cpu.py).  In float32 a row's sums run in the kernels' order
(``lane_sum``) and the backward sums as csrc/embedding_bwd.hip does: position order inside a
piece, the LayerNorm backward per piece, a segment's pieces added in piece order; dgamma / dbeta
per lane group, wave and block (``block_partials``) and then over the blocks of both kinds in
ncf_reduce_parts' order (``parts_sum``).  Every product is rounded before it is added, as
written; where the compiler fuses one the kernel differs by that rounding.

Tables and gradients come as dicts keyed "mfu", "mlpu", "mfi", "mlpi" (GMF / MLP table of users /
items); the LayerNorm parameters as dict(mf_gamma, mf_beta, mlp_gamma, mlp_beta).

* ``gather_ln_gmf``: csrc/gather_ln.hip's k_gather_ln_gmf (entry points ncf_gather_ln_gmf_fwd,
  _scaled_fwd, _ld_fwd, _bf16_fwd).  Row r is a source row if G <= 1, or r % G == 0, or its user
  differs from the user of its group's first row; the LN'd user rows are defined on source rows
  only.  An id outside [0, rows) reads row 0 and raises bit 0 of err.
* ``gather_rows``: ncf_gather_rows / ncf_embedding_export (LayerNorm optional, then the row
  divided by its Euclidean norm).
* ``embedding_bwd``: ncf_dedup_ids + ncf_embedding_bwd_reduce.  Per kind the sorted unique ids
  and the compact gradients LNbwd(sum of the id's occurrences); dgamma / dbeta of both norms,
  each summed over users and items.
* ``pieces``: the pieces the kernels cut the sorted ids into (csrc/segments.h: a segment = the
  run of one id, cut at every sorted position that is a multiple of NCF_PIECE = 16).
"""
import torch

LN_EPS = 1e-5
PIECE = 16
TABLES = ("mfu", "mlpu", "mfi", "mlpi")
F64, F32 = torch.float64, torch.float32


def _t(x, dtype):
    return None if x is None else torch.as_tensor(x).to(dtype)


def lane_sum(v):
    """The sum over the last axis (D = 4 L columns) in the kernels' order: a lane adds its four
    consecutive columns left to right, then the xor butterfly over the L lanes, widest stride
    first (ncf_common.h group_sum; the two-float4 gather's first level is the same pair)."""
    L = v.shape[-1] // 4
    q = v.reshape(*v.shape[:-1], L, 4)
    s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    idx, o = torch.arange(L), L // 2
    while o:
        s = s + s[..., idx ^ o]
        o //= 2
    return s[..., 0]


def nbr_of(n, D):
    """segments.h nbr_of: the piece-reduce blocks for n ids per kind (4 waves of 64 / (D / 4) lane
    groups, one piece per group at a time), capped at 768."""
    per = 4 * (1 if D >= 256 else 256 // D)
    return max(1, min(768, (n + n // PIECE + 2 + per - 1) // per))


def block_partials(v, nbr):
    """k_piece_reduce_ln's dgamma / dbeta partial rows [nbr, D] of one kind from the per-piece
    terms v [P, D]: lane group sg of wave w of block b takes the pieces (4 b + w) S + sg + k *
    (4 nbr S) in turn, the groups of a wave are added by xor butterfly (nearest first), the four
    waves in order."""
    D = v.shape[1]
    S = 64 // (D // 4)
    slots = nbr * 4 * S
    rounds = -(-v.shape[0] // slots)
    v = torch.cat([v, torch.zeros(rounds * slots - v.shape[0], D, dtype=v.dtype)])
    a = v[:slots]
    for k in range(1, rounds):
        a = a + v[k * slots:(k + 1) * slots]
    a = a.reshape(nbr, 4, S, D)
    idx, o = torch.arange(S), 1
    while o < S:
        a = a + a[:, :, idx ^ o]
        o *= 2
    a = a[:, :, 0]
    return ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]


def _parts_chunk(rows):
    """One chunk of ncf_reduce_parts (reduce_dev.h stage1_sum, reduce.hip stage2_sum): "wave" w
    takes rows w, w + 4, ...; while four of its rows remain they go to accumulators 0..3, its
    last (at most three) rows to accumulator 0; (a0 + a1) + (a2 + a3), then (w0 + w1) + (w2 + w3)."""
    ws = []
    for w in range(4):
        r = rows[w::4]
        a = [torch.zeros_like(rows[0]) for _ in range(4)]
        full = r.shape[0] // 4
        for g in range(full):
            for k in range(4):
                a[k] = a[k] + r[4 * g + k]
        for j in range(4 * full, r.shape[0]):
            a[0] = a[0] + r[j]
        ws.append((a[0] + a[1]) + (a[2] + a[3]))
    return (ws[0] + ws[1]) + (ws[2] + ws[3])


def parts_sum(rows):
    """ncf_reduce_parts over the partial rows [P, L]: one chunk up to 256 rows, otherwise chunks
    of 64 rows and then the chunk sums, each in ``_parts_chunk``'s order."""
    if rows.shape[0] <= 256:
        return _parts_chunk(rows)
    return _parts_chunk(torch.stack([_parts_chunk(rows[i:i + 64]) for i in range(0, rows.shape[0], 64)]))


def row_sum(v):
    return v.sum(-1) if v.dtype == F64 else lane_sum(v)


def ln_stats(x, eps):
    """(x - mean, 1 / sqrt(biased variance + eps)) of each row."""
    D = x.shape[-1]
    xc = x - (row_sum(x) / D)[..., None]
    return xc, 1.0 / torch.sqrt(row_sum(xc * xc) / D + eps)


def layer_norm(x, gamma, beta, eps):
    xc, rstd = ln_stats(x, eps)
    return xc * rstd[..., None] * gamma + beta


def layer_norm_bwd(dy, x, gamma, eps):
    """(dx, h): the LayerNorm backward at input rows x, and the normalised rows."""
    D = x.shape[-1]
    xc, rstd = ln_stats(x, eps)
    h = xc * rstd[..., None]
    gd = dy * gamma
    m1, m2 = row_sum(gd) / D, row_sum(gd * h) / D
    return rstd[..., None] * (gd - m1[..., None] - h * m2[..., None]), h


def safe_ids(ids, rows):
    """Ids outside [0, rows) read row 0; the second value is the error bit."""
    ids = torch.as_tensor(ids).long()
    bad = (ids < 0) | (ids >= rows)
    return torch.where(bad, torch.zeros_like(ids), ids), int(bool(bad.any()))


def source_rows(uid, G):
    uid = torch.as_tensor(uid).long()
    r = torch.arange(uid.numel())
    if G <= 1:
        return torch.ones_like(r, dtype=torch.bool)
    return (r % G == 0) | (uid != uid[r - r % G])


def gather_ln_gmf(uid, iid, tables, ln, w_mf, b_mf, eps=LN_EPS, item_scale=None, f=0.0, G=0,
                  dtype=F64, norm=layer_norm):
    """dict(mf_pred [n], mf_user_ln, mf_item_ln, mlp_user_ln, mlp_item_ln [n, D], src [n] bool,
    err).  The user rows are computed for every row; only those of ``src`` rows are defined.
    ``item_scale`` [n, D]: both LN'd item rows are multiplied by 1 + f * item_scale (f as the
    float32 the entry point takes) before the GMF product."""
    tab = {k: _t(v, dtype) for k, v in tables.items()}
    p = {k: _t(v, dtype) for k, v in ln.items()}
    w_mf, b_mf = _t(w_mf, dtype).reshape(-1), _t(b_mf, dtype).reshape(-1)[0]
    u, eu = safe_ids(uid, tab["mfu"].shape[0])
    i, ei = safe_ids(iid, tab["mfi"].shape[0])
    yu = norm(tab["mfu"][u], p["mf_gamma"], p["mf_beta"], eps)
    yi = norm(tab["mfi"][i], p["mf_gamma"], p["mf_beta"], eps)
    zu = norm(tab["mlpu"][u], p["mlp_gamma"], p["mlp_beta"], eps)
    zi = norm(tab["mlpi"][i], p["mlp_gamma"], p["mlp_beta"], eps)
    if item_scale is not None:
        m = 1.0 + float(torch.tensor(f, dtype=F32)) * _t(item_scale, dtype)
        yi, zi = yi * m, zi * m
    return dict(mf_pred=row_sum(yu * yi * w_mf) + b_mf, mf_user_ln=yu, mf_item_ln=yi,
                mlp_user_ln=zu, mlp_item_ln=zi, src=source_rows(uid, G), err=eu | ei)


def gather_rows(ids, table, gamma, beta, eps=LN_EPS, l2=False, dtype=F64, norm=layer_norm):
    """(rows [n, D], err): table[ids], LayerNorm when gamma is given, then / its L2 norm."""
    table = _t(table, dtype)
    i, err = safe_ids(ids, table.shape[0])
    x = table[i]
    if gamma is not None:
        x = norm(x, _t(gamma, dtype), _t(beta, dtype), eps)
    if l2:
        x = x / torch.sqrt(row_sum(x * x))[..., None]
    return x, err


def pieces(sorted_ids):
    """The piece list of one kind's sorted ids: dict(start [U + 1] segment starts, pstart [P + 1],
    pseg [P] the piece's segment, first [P] whether it is its segment's first piece,
    fpiece [U + 1] the first piece of each segment)."""
    s = torch.as_tensor(sorted_ids).long()
    n = s.numel()
    assert n >= 1 and bool((s[1:] >= s[:-1]).all())
    pos = torch.arange(n)
    head = torch.ones(n, dtype=torch.bool)
    head[1:] = s[1:] != s[:-1]
    phead = head | (pos % PIECE == 0)
    pst = pos[phead]
    first = head[pst]
    end = torch.tensor([n])
    return dict(start=torch.cat([pos[head], end]), pstart=torch.cat([pst, end]),
                pseg=(torch.cumsum(head.long(), 0) - 1)[pst], first=first,
                fpiece=torch.cat([torch.arange(pst.numel())[first], torch.tensor([pst.numel()])]))


def _gammas(gammas, dtype):
    return {"mf": _t(gammas[0], dtype), "mlp": _t(gammas[1], dtype)}


def _rows(tables, k, uniq, compact, dtype):
    """The table rows of the sorted unique ids (``compact``: the tables hold just those)."""
    return _t(tables[k] if compact else torch.as_tensor(tables[k])[uniq], dtype)


def embedding_bwd(uid, iid, dys, tables, gammas, eps=LN_EPS, compact=False):
    """float64.  dict(uniq_u, uniq_i, grads {table: [num_unique, D]}, mf_gamma, mf_beta,
    mlp_gamma, mlp_beta [D]); ``gammas`` = (mf, mlp)."""
    gam = _gammas(gammas, F64)
    out = dict(grads={})
    pg = {}
    for kind, ids in (("u", uid), ("i", iid)):
        uniq, inv = torch.unique(torch.as_tensor(ids).long(), sorted=True, return_inverse=True)
        out["uniq_" + kind] = uniq
        for t in ("mf", "mlp"):
            k = t + kind
            dy = _t(dys[k], F64)
            S = torch.zeros(uniq.numel(), dy.shape[1], dtype=F64).index_add_(0, inv, dy)
            dx, h = layer_norm_bwd(S, _rows(tables, k, uniq, compact, F64), gam[t], eps)
            out["grads"][k] = dx
            pg[t + "_gamma"] = pg.get(t + "_gamma", 0) + (S * h).sum(0)
            pg[t + "_beta"] = pg.get(t + "_beta", 0) + S.sum(0)
    return dict(out, **pg)


def embedding_bwd_f32(uid, iid, dys, tables, gammas, eps=LN_EPS, compact=False,
                      lnbwd=layer_norm_bwd, drop_last_extra=False, dgamma_through_gamma=False):
    """The same in float32 and in the kernels' order.  The other arguments make the mutants of
    tests/test_embed_cpu.py: another LayerNorm backward, the last extra piece of a multi-piece
    segment left out, dgamma accumulated as dy * gamma * h."""
    gam = _gammas(gammas, F32)
    out = dict(grads={})
    parts = {}
    for kind, ids in (("u", uid), ("i", iid)):
        ids = torch.as_tensor(ids).long()
        order = torch.argsort(ids, stable=True)
        pc = pieces(ids[order])
        uniq = ids[order][pc["start"][:-1]]
        out["uniq_" + kind] = uniq
        ps, cnt = pc["pstart"][:-1], pc["pstart"][1:] - pc["pstart"][:-1]
        fp, npc = pc["fpiece"][:-1], pc["fpiece"][1:] - pc["fpiece"][:-1]
        for t in ("mf", "mlp"):
            k = t + kind
            dy = _t(dys[k], F32)
            acc = torch.zeros(ps.numel(), dy.shape[1], dtype=F32)
            for j in range(PIECE):          # position order inside a piece
                m = cnt > j
                acc[m] += dy[order[ps[m] + j]]
            dx, h = lnbwd(acc, _rows(tables, k, uniq, compact, F32)[pc["pseg"]], gam[t], eps)
            G = dx[fp].clone()
            for e in range(1, int(npc.max())):      # the extra pieces, in piece order
                m = npc > (e + 1 if drop_last_extra else e)
                G[m] += dx[fp[m] + e]
            out["grads"][k] = G
            term = acc * gam[t] * h if dgamma_through_gamma else acc * h
            nbr = nbr_of(ids.numel(), dy.shape[1])
            parts.setdefault(t + "_gamma", []).append(block_partials(term, nbr))
            parts.setdefault(t + "_beta", []).append(block_partials(acc, nbr))
    return dict(out, **{q: parts_sum(torch.cat(v)) for q, v in parts.items()})
