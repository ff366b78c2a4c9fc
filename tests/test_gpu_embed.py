"""The embedding end of the step, one kernel family at a time, against float64
(tests/embed_ref.py), on the MI355X: k_gather_ln_gmf through its entry points (plain, _scaled,
_ld, _bf16) with ncf_gather_rows / ncf_embedding_export, and ncf_dedup_ids +
ncf_embedding_bwd_reduce (k_piece_reduce_ln, k_piece_fixup) with its _bf16, _rows and deferred
forms, at every D the kernels dispatch and at the geometries where they branch.

Each check takes the implementation under test as an argument (tests/test_gpu_rowops.py is the
pattern, and its ``_hold`` / ``frac`` are used here): the kernel here; tests/test_embed_cpu.py
runs the same check, on the same inputs, with the fp32 restatement (which must pass with a
quarter of every bound to spare, or stand in the tables below) and with mutants (which must
fail).

Bounds, none fitted to the GPU's output: forward outputs rtol 1e-5 / atol 2e-6, gradients
rtol 2e-4 / atol 2e-6 (tests/test_gpu_rowops.TOL).
"""
import functools

import pytest
import torch

import _ncf_pkg
from tests import embed_ref as R
from tests.test_gpu_rowops import TOL, _hold

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")
EPS = R.LN_EPS
DIMS = (16, 32, 64, 128, 256)

# Where the fp32 restatement does not stay within a quarter of the project's bound: its measured
# worst fraction of that bound (one host thread; tests/test_embed_cpu.py re-measures it), and the
# case's bound for that quantity is 4 x the figure.  The gather: mf_pred, a sum of D products
# that may cancel to near 0 under an absolute bound of 2e-6, and the LN'd rows of the
# low-variance table rows (U_LOW, I_LOW below: 1 / sqrt(var + eps) = 95 magnifies the rounding of
# x - mean).  The backward: sums over up to 280 occurrences (the table gradients at D = 256) or
# over every occurrence of both kinds (dgamma / dbeta) that nearly cancel in some column.
# key: (D, n, group_rows, variant), over the runs with and without out-of-range ids
GATHER_FP32 = {
    (16, 1000, 5, "plain"): {"mf_user_ln": 0.311},
    (16, 1000, 5, "scaled"): {"mf_user_ln": 0.311},
    (16, 1000, 5, "ld"): {"mf_user_ln": 0.311},
    (32, 1003, 0, "plain"): {"mf_pred": 0.2712, "mlp_item_ln": 0.2976},
    (32, 1000, 5, "plain"): {"mf_pred": 0.3086},
    (32, 1003, 0, "scaled"): {"mlp_item_ln": 0.4543},
    (32, 1000, 5, "scaled"): {"mf_pred": 0.3014, "mlp_item_ln": 0.277},
    (32, 1003, 0, "ld"): {"mf_pred": 0.2712, "mlp_item_ln": 0.2976},
    (32, 1000, 5, "ld"): {"mf_pred": 0.3086},
    (64, 1000, 5, "plain"): {"mf_pred": 0.2784},
    (64, 1003, 0, "scaled"): {"mf_pred": 0.2839},
    (64, 1000, 5, "scaled"): {"mf_pred": 0.3484},
    (64, 1000, 5, "ld"): {"mf_pred": 0.2784},
    (64, 1000, 5, "bf16"): {"mf_pred": 0.2873},
    (128, 1003, 0, "plain"): {"mf_pred": 0.2778, "mlp_item_ln": 0.2797, "mf_user_ln": 0.3199,
                              "mf_item_ln": 0.2677},
    (128, 1000, 5, "plain"): {"mlp_user_ln": 0.2592},
    (128, 1003, 0, "scaled"): {"mlp_item_ln": 0.3197, "mf_user_ln": 0.3199, "mf_item_ln": 0.315},
    (128, 1000, 5, "scaled"): {"mf_pred": 0.3843, "mlp_user_ln": 0.2592},
    (128, 1003, 0, "ld"): {"mf_pred": 0.2778, "mlp_item_ln": 0.2797, "mf_user_ln": 0.3199,
                           "mf_item_ln": 0.2677},
    (128, 1000, 5, "ld"): {"mlp_user_ln": 0.2592},
    (128, 1003, 0, "bf16"): {"mf_pred": 0.2804},
    (256, 1003, 0, "plain"): {"mf_user_ln": 0.4519},
    (256, 1000, 5, "plain"): {"mf_pred": 0.27},
    (256, 1003, 0, "scaled"): {"mf_pred": 0.264, "mf_user_ln": 0.4519},
    (256, 1000, 5, "scaled"): {"mf_pred": 0.2578},
    (256, 1003, 0, "ld"): {"mf_user_ln": 0.4519},
    (256, 1000, 5, "ld"): {"mf_pred": 0.27},
    (256, 1000, 5, "bf16"): {"mf_pred": 0.2638},
}
# key: (D, LayerNorm, l2_normalize), ncf_gather_rows / ncf_embedding_export
ROWS_FP32 = {
    (128, True, 0): 0.2677,
}
# key: (D, layout, num_users, bf16 tables)
BWD_FP32 = {
    (64, "struct", 700, False): {"mlp_beta": 1.062},
    (128, "struct", 700, False): {"mf_gamma": 0.3195},
    (256, "struct", 700, False): {"mfu": 0.4494, "mlpu": 0.7543, "mlpi": 0.3091, "mlp_beta": 0.9424},
    (256, "big256", 20000, False): {"mf_gamma": 0.3214, "mlp_beta": 0.302},
    (16, "big16", 60000, False): {"mfu": 0.3806, "mlpu": 0.3066, "mfi": 0.297, "mf_gamma": 0.7743},
    (16, "struct", 2048, False): {"mf_gamma": 0.5938},
    (64, "struct", 700, True): {"mf_gamma": 0.3924},
    (256, "struct", 700, True): {"mlpi": 0.6847},
}


# ----------------------------------------------------------------------------- the gather
U, I = 700, 300
# exactly constant rows (LayerNorm gives beta), and rows of standard deviation 0.01 around 0.1
# (var = 1e-4 against eps = 1e-5: where eps enters decides 5 % of the output).  The constants
# have few mantissa bits, so every partial sum of D of them is exact in fp32 in any order and the
# fp32 result is beta itself; a constant with a full mantissa would measure the rounding of the
# mean magnified by 1 / sqrt(eps) = 316, not the kernel.
U_CONST, U_LOW, I_CONST, I_LOW = 41, 2, 17, 3
CONST = {"u": 0.375, "i": -1.25}
SCALE_F = 0.3
GATHER_VARIANTS = ("plain", "scaled", "ld", "bf16")
GATHER_OUT = ("mf_pred", "mlp_user_ln", "mlp_item_ln", "mf_user_ln", "mf_item_ln")
# (n, group_rows, out-of-range ids): 1003 rows are no multiple of the 256-thread block's rows at
# any lane count; groups of 5 rows of one user with one row that leaves its group's user
GATHER_RUNS = ((1, 0, False), (1, 0, True), (1003, 0, False), (1003, 0, True), (1000, 5, False),
               (1000, 5, True))
G_ODD_ROW = 5 * 7 + 2


@functools.lru_cache(maxsize=6)
def gather_case(D, n, G, bad):
    g = torch.Generator().manual_seed(1009 * D + 7 * n + G)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    tables = {}
    for k in R.TABLES:
        kind = k[-1]
        t = rn(U if kind == "u" else I, D) * 0.7 + 0.1
        t[U_CONST if kind == "u" else I_CONST] = CONST[kind]
        t[U_LOW if kind == "u" else I_LOW] = 0.1 + 0.01 * rn(D)
        tables[k] = t
    ln = dict(mf_gamma=0.5 + torch.rand(D, generator=g), mf_beta=rn(D),
              mlp_gamma=0.5 + torch.rand(D, generator=g), mlp_beta=rn(D))
    if G:
        gu = torch.randint(0, U, (n // G,), generator=g)
        gu[3], gu[4] = U_CONST, U_LOW
        uid = gu.repeat_interleave(G)
        uid[G_ODD_ROW] = (uid[G_ODD_ROW] + 1) % U
    else:
        uid = torch.randint(0, U, (n,), generator=g)
        uid[4 % n], uid[3 % n] = U_LOW, U_CONST
    iid = torch.randint(0, I, (n,), generator=g)
    iid[6 % n], iid[5 % n] = I_LOW, I_CONST
    if bad:
        iid[11 % n], uid[17 % n] = I + 4, -1
    return dict(D=D, n=n, G=G, bad=bad, uid=uid, iid=iid, tables=tables, ln=ln,
                tables_bf={k: v.bfloat16() for k, v in tables.items()},
                w_mf=rn(D) / D ** 0.5, b_mf=rn(1), item_scale=rn(n, D), ref={})


def gather_ref(c, variant):
    """float64, once per case and variant ("ld" reads the same tables as "plain"; "bf16" the
    rounded tables widened)."""
    key = "plain" if variant == "ld" else variant
    if key not in c["ref"]:
        tabs = {k: v.float() for k, v in c["tables_bf"].items()} if key == "bf16" else c["tables"]
        c["ref"][key] = R.gather_ln_gmf(
            c["uid"], c["iid"], tabs, c["ln"], c["w_mf"], c["b_mf"], EPS,
            item_scale=c["item_scale"] if key == "scaled" else None, f=SCALE_F, G=c["G"])
    return c["ref"][key]


def check_gather(D, n, G, bad, variant, impl):
    """``impl(case, variant)`` -> dict of the five outputs (pre-filled with nan by the
    implementation, so an unwritten row shows) and err.  Source rows of the user outputs and
    every row of the item outputs and mf_pred against float64; copy rows still nan; bit 0 of err
    exactly when an id is out of range.  Returns the worst fraction per quantity."""
    c = gather_case(D, n, G, bad)
    ref, got = gather_ref(c, variant), impl(c, variant)
    worst, tag = {}, (D, n, G, bad, variant)
    fp32 = GATHER_FP32.get((D, n, G, variant), {})
    assert int(got["err"]) == (1 if bad else 0), tag
    src = ref["src"]
    if G:       # every group one user, but for the odd row (and the row of the id -1)
        assert int(src.sum()) == n // G + 1 + int(bad) and bool(src[G_ODD_ROW])
    else:
        assert bool(src.all())
    for k in GATHER_OUT:
        rows = src if "user" in k else torch.ones(n, dtype=torch.bool)
        _hold(worst, tag, k, got[k][rows], ref[k][rows], TOL["fwd"], fp32.get(k))
        assert bool(torch.isnan(got[k][~rows]).all()), (tag, k, "a copy row was written")
    # constant rows: beta itself in float64 (and within the bound above in the implementation)
    cu, ci = (c["uid"] == U_CONST) & src, c["iid"] == I_CONST
    assert bool(cu.any()) and bool(ci.any()) or (n == 1 and bad), tag
    for t in ("mf", "mlp"):
        beta = c["ln"][t + "_beta"].double()
        assert bool((ref[t + "_user_ln"][cu] == beta).all()), tag
        if variant != "scaled":
            assert bool((ref[t + "_item_ln"][ci] == beta).all()), tag
    return worst


def _dev(t):
    return t.to(DEV)


def _nan(*s, dtype=torch.float32):
    return torch.full(s, float("nan"), device=DEV, dtype=dtype)


def gpu_gather(c, variant, null_mf=False):
    from ncf_amd import _lib
    D, n, G = c["D"], c["n"], c["G"]
    st = _lib.stream_ptr(DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    uid, iid = _dev(c["uid"]), _dev(c["iid"])
    par = [_dev(c["ln"][k]) for k in ("mf_gamma", "mf_beta", "mlp_gamma", "mlp_beta")] + \
        [_dev(c["w_mf"]), _dev(c["b_mf"])]
    outs = [_nan(n)] + [_nan(n, D) for _ in range(4)]
    op = [P(o) for o in outs]
    if null_mf:
        op[3] = op[4] = None
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    src = c["tables_bf"] if variant == "bf16" else c["tables"]
    if variant == "ld":     # one [rows, 2 D] buffer per kind: mf = buf, mlp = buf + D
        bu = _dev(torch.cat([src["mfu"], src["mlpu"]], 1).contiguous())
        bi = _dev(torch.cat([src["mfi"], src["mlpi"]], 1).contiguous())
        keep, tp = (bu, bi), [P(bu), P(bi), P(bu) + 4 * D, P(bi) + 4 * D]
    else:
        keep = [_dev(src[k]) for k in ("mfu", "mfi", "mlpu", "mlpi")]
        tp = [P(t) for t in keep]
    head = [P(uid), P(iid), n, *tp, U, I, D]
    pp = [P(x) for x in par]
    if variant == "ld":
        _lib.call("ncf_gather_ln_gmf_ld_fwd", *head, 2 * D, *pp, EPS, G, *op, P(err), st)
    elif variant == "bf16":
        _lib.call("ncf_gather_ln_gmf_bf16_fwd", *head, *pp, EPS, G, *op, P(err), st)
    elif variant == "scaled":
        zs = _dev(c["item_scale"])
        _lib.call("ncf_gather_ln_gmf_scaled_fwd", *head, *pp, EPS, P(zs), SCALE_F, G, *op, P(err), st)
    elif G:                 # the plain kernel with groups: the scaled entry point without a scale
        _lib.call("ncf_gather_ln_gmf_scaled_fwd", *head, *pp, EPS, None, 0.0, G, *op, P(err), st)
    else:
        _lib.call("ncf_gather_ln_gmf_fwd", *head, *pp, EPS, *op, P(err), st)
    torch.cuda.synchronize()
    del keep
    res = {k: o.cpu() for k, o in zip(GATHER_OUT, outs)}
    res["err"] = int(err.cpu())
    return res


def _report(name, worst):
    print(f"{name}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _merge(total, worst):
    for k, v in worst.items():
        total[k] = max(total.get(k, 0.0), v)


@pytest.mark.parametrize("D", DIMS)
def test_gather_ln_gmf_vs_float64(D):
    for variant in GATHER_VARIANTS:
        total = {}
        for n, G, bad in GATHER_RUNS:
            _merge(total, check_gather(D, n, G, bad, variant, gpu_gather))
        _report(f"gather D {D} {variant}", total)


@pytest.mark.parametrize("D", DIMS)
def test_gather_null_mf_outputs(D):
    """mf_user_ln / mf_item_ln NULL: accepted, and the other outputs the same bits."""
    for variant in GATHER_VARIANTS:
        for n, G, bad in ((1003, 0, True), (1000, 5, False)):
            c = gather_case(D, n, G, bad)
            full, part = gpu_gather(c, variant), gpu_gather(c, variant, null_mf=True)
            assert full["err"] == part["err"]
            for k in GATHER_OUT[:3]:
                assert torch.equal(full[k].view(torch.int32), part[k].view(torch.int32)), (variant, k)
            for k in GATHER_OUT[3:]:
                assert bool(torch.isnan(part[k]).all())


# (entry point, LayerNorm, l2_normalize)
ROWS_RUNS = (("rows", False, 0), ("rows", True, 0), ("export", False, 0), ("export", True, 0),
             ("export", False, 1), ("export", True, 1))


def check_gather_rows(D, bad, entry, ln, l2, impl):
    """``impl(case, entry, ln, l2)`` -> (rows [n, D], err): the GMF item table of the gather's
    case under its item ids."""
    c = gather_case(D, 1003, 0, bad)
    key = ("rows", ln, l2)
    if key not in c["ref"]:
        c["ref"][key] = R.gather_rows(c["iid"], c["tables"]["mfi"], c["ln"]["mf_gamma"] if ln else None,
                                      c["ln"]["mf_beta"], EPS, bool(l2))
    want, werr = c["ref"][key]
    got, err = impl(c, entry, ln, l2)
    assert err == werr == int(bad), (D, bad, entry, ln, l2)
    worst = {}
    _hold(worst, (D, bad, entry, ln, l2), "rows", got, want, TOL["fwd"], ROWS_FP32.get((D, ln, l2)))
    return worst


def gpu_gather_rows(c, entry, ln, l2):
    from ncf_amd import _lib
    D, n = c["D"], c["n"]
    ids, tab = _dev(c["iid"]), _dev(c["tables"]["mfi"])
    gam, bet = _dev(c["ln"]["mf_gamma"]), _dev(c["ln"]["mf_beta"])
    out, err = _nan(n, D), torch.zeros(1, dtype=torch.int32, device=DEV)
    head = [ids.data_ptr(), n, tab.data_ptr(), I, D, gam.data_ptr() if ln else None,
            bet.data_ptr() if ln else None, EPS]
    if entry == "rows":
        assert not l2
        _lib.call("ncf_gather_rows", *head, out.data_ptr(), err.data_ptr(), _lib.stream_ptr(DEV))
    else:
        _lib.call("ncf_embedding_export", *head, l2, out.data_ptr(), err.data_ptr(),
                  _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return out.cpu(), int(err.cpu())


@pytest.mark.parametrize("D", DIMS)
def test_gather_rows_and_export_vs_float64(D):
    total = {}
    for bad in (False, True):
        for entry, ln, l2 in ROWS_RUNS:
            _merge(total, check_gather_rows(D, bad, entry, ln, l2, gpu_gather_rows))
    _report(f"gather_rows D {D}", total)


# ----------------------------------------------------------------------------- the backward
PARAMS = ("mf_gamma", "mf_beta", "mlp_gamma", "mlp_beta")
# Occurrences per id in sorted-id order (users; the items take the list reversed).  Sorted
# positions: 15 singletons, a pair on 15..16 (split by the cut at 16), singletons to 31, 16 on
# 32..47 (one whole piece), 17 on 48..64, 150 on 65..214 (10 pieces: 9 extras, the fix-up's second
# round of 8), 280 on 215..494 (18 pieces: 17 extras, its third round), short runs and singletons
# to 603 = 37 * 16 + 11.
STRUCT = [1] * 15 + [2] + [1] * 15 + [16, 17, 150, 280] + [3, 1, 1, 5, 1, 2, 1, 1, 7, 1, 4] + [1] * 81
LAYOUTS = {
    "struct": STRUCT,
    "one": [1],
    "two": [2],
    # more unique ids than one sweep of the fix-up's 2048 blocks covers (8192 at D = 256), with
    # the multi-piece segments past them, and more pieces than 768 blocks x 4 waves take at once
    "big256": [1] * 8400 + [40, 2, 17, 33] + [1] * 9,
    # more pieces than 768 blocks x 4 waves x 16 lane groups take at once (D = 16)
    "big16": [1] * 49500 + [40, 2, 17, 33] + [3] * 300,
}
BWD_MODES = ("reduce", "onecall", "bf16", "rows", "defer")
ROWS_PAD = 8        # out_ld = 2 D + 8 in mode "rows"


nbr_of = R.nbr_of


def fixup_blocks(n, D):
    """embedding_bwd.hip piece_reduce: fix-up blocks of 256 threads, D / 4 lanes per segment."""
    return max(1, min(2048, (n * (D // 4) + 255) // 256))


def sort_passes(rows0, rows1):
    """segments.h sort_passes: radix digits of at most 11 bits over the larger table's ids."""
    b = 1
    while b < 32 and (1 << b) < max(rows0, rows1):
        b += 1
    return (b + 10) // 11


def coverage(sorted_ids):
    """What the piece structure of one kind's sorted ids contains."""
    pc = R.pieces(sorted_ids)
    s0, ln = pc["start"][:-1], pc["start"][1:] - pc["start"][:-1]
    npc = pc["fpiece"][1:] - pc["fpiece"][:-1]
    cnt = pc["pstart"][1:] - pc["pstart"][:-1]
    assert int(cnt.max()) <= R.PIECE and int(cnt.min()) >= 1
    return dict(split_pair=bool(((ln == 2) & (s0 % R.PIECE == R.PIECE - 1)).any()),
                whole_piece=bool(((ln == R.PIECE) & (s0 % R.PIECE == 0)).any()),
                seventeen=bool((ln == 17).any()), ten_pieces=bool((npc >= 10).any()),
                eighteen_pieces=bool((npc >= 18).any()), singletons=bool((ln == 1).any()),
                short_last_piece=int(cnt[-1]) < R.PIECE, pieces=int(cnt.numel()),
                segments=int(ln.numel()),
                last_multi_piece_segment=int(torch.nonzero(npc > 1).max()) if bool((npc > 1).any()) else -1)


def _pick_ids(rows, m, g):
    """m distinct sorted ids of [0, rows) with both ends of the range among them."""
    if m == 1:
        return torch.tensor([rows - 1])
    pool = torch.unique(torch.randint(1, rows - 1, (8 * m + 64,), generator=g))
    assert pool.numel() >= m - 2
    sel = pool[torch.randperm(pool.numel(), generator=g)[:m - 2]]
    return torch.sort(torch.cat([torch.tensor([0]), sel, torch.tensor([rows - 1])])).values


@functools.lru_cache(maxsize=3)
def bwd_case(D, layout, num_users, num_items, bf16=False):
    """Id lists built from the layout's per-id counts and permuted by position; the rows of the
    unique ids only (compact, in sorted-id order: the tables are built around them where they
    are needed), rounded to bf16 when the tables are; float64 results."""
    counts = LAYOUTS[layout]
    n, m = sum(counts), len(counts)
    g = torch.Generator().manual_seed(4099 * D + n + num_users % 1013 + bf16)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(D=D, layout=layout, U=num_users, I=num_items, bf16=bf16, n=n)
    for kind, rows, cnt in (("u", num_users, counts), ("i", num_items, counts[::-1])):
        ids = _pick_ids(rows, m, g)
        c["sorted_" + kind] = ids.repeat_interleave(torch.tensor(cnt))
        c[kind + "id"] = c["sorted_" + kind][torch.randperm(n, generator=g)]
        c["uniq_" + kind] = ids
    c["rows"] = {k: rn(m, D) * 0.7 + 0.1 for k in R.TABLES}
    if bf16:
        c["rows"] = {k: v.bfloat16().float() for k, v in c["rows"].items()}
    c["dys"] = {k: rn(n, D) for k in R.TABLES}
    c["gammas"] = (0.5 + torch.rand(D, generator=g), 0.5 + torch.rand(D, generator=g))
    # mode "rows": unique row c of a kind goes to row out_rows[c] of n + 3
    c["out_rows"] = {k: torch.randperm(n + 3, generator=g)[:n].int() for k in "ui"}
    c["ref"] = R.embedding_bwd(c["uid"], c["iid"], c["dys"], c["rows"], c["gammas"], EPS, compact=True)
    assert torch.equal(c["ref"]["uniq_u"], c["uniq_u"]) and torch.equal(c["ref"]["uniq_i"], c["uniq_i"])
    return c


def pad_bwd(c, res):
    """A result of tests/embed_ref.embedding_bwd* in the layout the checks read: uniq ids in n
    slots (-7 beyond num_unique), gradients in [n, D] (nan beyond)."""
    n, D = c["n"], c["D"]
    out = dict(nu=[res["uniq_u"].numel(), res["uniq_i"].numel()], grads={})
    for kind in "ui":
        u = torch.full((n,), -7, dtype=torch.int64)
        u[:res["uniq_" + kind].numel()] = res["uniq_" + kind]
        out["uniq_" + kind] = u
    for k in R.TABLES:
        G = torch.full((n, D), float("nan"))
        G[:res["grads"][k].shape[0]] = res["grads"][k]
        out["grads"][k] = G
    out.update({q: res[q] for q in PARAMS})
    return out


def check_bwd(c, impl, mode="reduce", **kw):
    """``impl(case, mode)`` -> dict(nu [2], uniq_u, uniq_i [n], grads {table: [n, D]}, the four
    PARAMS).  num_unique and the unique ids equal the reference's; the compact gradients on
    [0, num_unique) and the LayerNorm parameter gradients against float64; the rows beyond
    num_unique untouched.  Returns the worst fraction per quantity."""
    got, ref = impl(c, mode, **kw), c["ref"]
    worst, tag = {}, (c["D"], c["layout"], c["U"], mode)
    fp32 = BWD_FP32.get((c["D"], c["layout"], c["U"], c["bf16"]), {})
    for j, kind in enumerate("ui"):
        nu = ref["uniq_" + kind].numel()
        assert int(got["nu"][j]) == nu, tag
        assert torch.equal(got["uniq_" + kind][:nu], ref["uniq_" + kind]), tag
        assert bool((got["uniq_" + kind][nu:] == -7).all()), tag
    for k in R.TABLES:
        nu = ref["grads"][k].shape[0]
        _hold(worst, tag, k, got["grads"][k][:nu], ref["grads"][k], TOL["grad"], fp32.get(k))
        assert bool(torch.isnan(got["grads"][k][nu:]).all()), (tag, k, "rows beyond num_unique written")
    for q in PARAMS:
        _hold(worst, tag, q, got[q], ref[q], TOL["grad"], fp32.get(q))
    return worst


def gpu_bwd(c, mode, small=None):
    """``small``: ncf_dedup_set_small_max for the call (2048: the one-launch dedup where n fits,
    0: the radix sort; None: as the library stands)."""
    from ncf_amd import _lib
    n, D, NU, NI = c["n"], c["D"], c["U"], c["I"]
    assert c["bf16"] == (mode == "bf16")
    st = _lib.stream_ptr(DEV)
    P = lambda t: t.data_ptr()  # noqa: E731
    uid, iid = _dev(c["uid"]), _dev(c["iid"])
    dys = [_dev(c["dys"][k]) for k in R.TABLES]
    gm, gl = _dev(c["gammas"][0]), _dev(c["gammas"][1])
    # the tables: nan everywhere but the rows the ids name (a row read elsewhere shows)
    tdt = torch.bfloat16 if mode == "bf16" else torch.float32
    if mode == "rows":      # one [rows, 2 D] buffer per kind: mf = buf, mlp = buf + D
        bufs = {}
        for kind, rows in (("u", NU), ("i", NI)):
            b = _nan(rows, 2 * D)
            b[_dev(c["uniq_" + kind])] = _dev(torch.cat([c["rows"]["mf" + kind], c["rows"]["mlp" + kind]], 1))
            bufs[kind] = b
        tp = [P(bufs["u"]), P(bufs["u"]) + 4 * D, P(bufs["i"]), P(bufs["i"]) + 4 * D]
    else:
        tabs = []
        for k in R.TABLES:
            t = _nan(NU if k[-1] == "u" else NI, D, dtype=tdt)
            t[_dev(c["uniq_" + k[-1]])] = _dev(c["rows"][k]).to(tdt)
            tabs.append(t)
        tp = [P(t) for t in tabs]
    ws = torch.full((_lib.query("ncf_embedding_bwd_workspace", n, D),), 0x5A, dtype=torch.uint8,
                    device=DEV)
    uq = [torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
    nu = torch.zeros(2, dtype=torch.int32, device=DEV)
    pg = [_nan(D) for _ in range(4)]
    ld = 2 * D + ROWS_PAD
    if mode == "rows":
        ob = {k: _nan(n + 3, ld) for k in "ui"}
        gp = [P(ob["u"]), P(ob["u"]) + 4 * D, P(ob["i"]), P(ob["i"]) + 4 * D]
        orow = {k: _dev(c["out_rows"][k]) for k in "ui"}
    else:
        G = [_nan(n, D) for _ in range(4)]
        gp = [P(x) for x in G]
    lst = None
    if mode == "defer":
        lst = _lib.ReduceList()
        lst.count = 0
    prev = None if small is None else _lib.query("ncf_dedup_set_small_max", small)
    try:
        dy_p, pg_p = [P(x) for x in dys], [P(x) for x in pg]
        if mode == "onecall":
            _lib.call("ncf_embedding_bwd", P(uid), P(iid), n, D, NU, NI, *dy_p, *tp, P(gm), P(gl), EPS,
                      *gp, P(uq[0]), P(uq[1]), None, None, P(nu), *pg_p, P(ws), ws.numel(), st)
        else:
            _lib.call("ncf_dedup_ids", P(uid), P(iid), n, D, NU, NI, P(uq[0]), P(uq[1]), None, None,
                      P(nu), P(ws), ws.numel(), st)
            head = [n, D, NU, NI, *dy_p, *tp, P(gm), P(gl), EPS, *gp, P(uq[0]), P(uq[1])]
            tail = [*pg_p, P(ws), ws.numel(), None if lst is None else lst.address, st]
            if mode == "rows":
                _lib.call("ncf_embedding_bwd_reduce_rows", *head, P(orow["u"]), P(orow["i"]), ld,
                          2 * D, *tail)
            else:
                _lib.call("ncf_embedding_bwd_reduce_bf16" if mode == "bf16" else
                          "ncf_embedding_bwd_reduce", *head, *tail)
        if lst is not None:
            assert lst.count == 4
            scratch = _nan(max(_lib.query("ncf_reduce_batch_scratch", lst.address), 1))
            _lib.call("ncf_reduce_batch", lst.address, scratch.data_ptr(), scratch.numel(), st)
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            _lib.query("ncf_dedup_set_small_max", prev)
    res = dict(nu=nu.cpu().tolist(), uniq_u=uq[0].cpu(), uniq_i=uq[1].cpu(), grads={})
    if mode == "rows":      # the rows named by out_rows; the gaps and the unused rows stay nan
        for j, kind in enumerate("ui"):
            buf, k = ob[kind].cpu(), res["nu"][j]
            rows = c["out_rows"][kind][:k].long()
            for t, lo in (("mf", 0), ("mlp", D)):
                g = torch.full((n, D), float("nan"))
                g[:k] = buf[rows, lo:lo + D]
                res["grads"][t + kind] = g
            buf[rows, :2 * D] = float("nan")
            assert bool(torch.isnan(buf).all()), ("rows", kind, "written outside out_rows' rows")
    else:
        res["grads"] = {k: x.cpu() for k, x in zip(R.TABLES, G)}
    res.update({q: x.cpu() for q, x in zip(PARAMS, pg)})
    return res


def _same_bits(a, b):
    assert a["nu"] == b["nu"]
    for k in ("uniq_u", "uniq_i"):
        assert torch.equal(a[k], b[k]), k
    for k in R.TABLES:
        assert torch.equal(a["grads"][k].view(torch.int32), b["grads"][k].view(torch.int32)), k
    for q in PARAMS:
        assert torch.equal(a[q].view(torch.int32), b[q].view(torch.int32)), q


@pytest.mark.parametrize("small", [2048, 0], ids=["small", "radix"])
@pytest.mark.parametrize("D", DIMS)
def test_embedding_bwd_vs_float64(D, small):
    """The structured id list, one id, and one id twice, through both dedup forms, as the two
    calls and as the one call."""
    for layout in ("struct", "one", "two"):
        c = bwd_case(D, layout, U, I)
        for mode in ("reduce", "onecall"):
            _report(f"embedding_bwd D {D} {layout} {mode} small_max {small}",
                    check_bwd(c, gpu_bwd, mode, small=small))


@pytest.mark.parametrize("D,layout,rows", [(256, "big256", 20000), (16, "big16", 60000)])
def test_embedding_bwd_grid_stride(D, layout, rows):
    """More pieces than the capped piece grid takes at once and (D = 256) more segments than the
    capped fix-up grid does (tests/test_embed_cpu.py asserts both from the formulas above)."""
    c = bwd_case(D, layout, rows, rows)
    _report(f"embedding_bwd D {D} {layout}", check_bwd(c, gpu_bwd, "reduce"))


@pytest.mark.parametrize("num_users", [1 << 11, 300000, (1 << 22) + 1])
def test_embedding_bwd_radix_passes(num_users):
    """1, 2 and 3 radix passes (an odd count leaves the sorted pairs in the other ping-pong
    buffer), D = 16."""
    assert sort_passes(num_users, I) == {1 << 11: 1, 300000: 2, (1 << 22) + 1: 3}[num_users]
    c = bwd_case(16, "struct", num_users, I)
    _report(f"embedding_bwd D 16 rows {num_users}", check_bwd(c, gpu_bwd, "reduce", small=0))


@pytest.mark.parametrize("mode", ["bf16", "rows", "defer"])
@pytest.mark.parametrize("D", [16, 64, 256])
def test_embedding_bwd_modes(D, mode):
    """bf16 tables, the out_rows / out_ld / table_ld form and the deferred dgamma / dbeta, each
    against float64; a second run of the same call gives the same bits (every sum has a fixed
    order)."""
    c = bwd_case(D, "struct", U, I, mode == "bf16")
    runs = []

    def impl(case, m):
        runs.append(gpu_bwd(case, m))
        return runs[-1]
    _report(f"embedding_bwd D {D} {mode}", check_bwd(c, impl, mode))
    _same_bits(runs[0], gpu_bwd(c, mode))
