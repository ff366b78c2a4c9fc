"""The premises of tests/test_gpu_embed.py, without a GPU: the float64 restatements
(tests/embed_ref.py) agree with torch autograd; on every case of every check there the fp32
restatement passes with a quarter of each bound to spare (or stands, with its measured fraction,
in GATHER_FP32 / ROWS_FP32 / BWD_FP32); the mutants a subtly wrong kernel would be fail the same check on the
same inputs; and every case contains the piece structure and reaches the grid caps it is there
for."""
import pytest
import torch

from tests import embed_ref as R
from tests import test_gpu_embed as G
from tests.test_rowops_cpu import one_thread

F64, F32 = torch.float64, torch.float32
NAN = float("nan")


def _headroom(tag, worst, listed):
    """A quarter of the project's bound, or the figure recorded beside the case; and no bound
    wider than 4 x what is measured here."""
    for k, v in worst.items():
        assert v < 0.25 or (k in listed and v <= 1.001 * listed[k]), (tag, k, v)
    for k, v in listed.items():
        assert 0.25 <= v <= 1.001 * worst[k], (tag, k, v, worst[k])


# ----------------------------------------------------------------------------- float64 against autograd
@pytest.mark.parametrize("D", G.DIMS)
def test_gather_float64_matches_torch(D):
    c = G.gather_case(D, 1003, 0, False)
    ref = G.gather_ref(c, "plain")
    ln = {k: v.double() for k, v in c["ln"].items()}
    F = torch.nn.functional
    rows = {k: c["tables"][k].double()[c["uid" if k[-1] == "u" else "iid"]] for k in R.TABLES}
    yu = F.layer_norm(rows["mfu"], (D,), ln["mf_gamma"], ln["mf_beta"], G.EPS)
    yi = F.layer_norm(rows["mfi"], (D,), ln["mf_gamma"], ln["mf_beta"], G.EPS)
    want = dict(mf_user_ln=yu, mf_item_ln=yi,
                mlp_user_ln=F.layer_norm(rows["mlpu"], (D,), ln["mlp_gamma"], ln["mlp_beta"], G.EPS),
                mlp_item_ln=F.layer_norm(rows["mlpi"], (D,), ln["mlp_gamma"], ln["mlp_beta"], G.EPS),
                mf_pred=F.linear(yu * yi, c["w_mf"].double()[None], c["b_mf"].double())[:, 0])
    for k, v in want.items():
        torch.testing.assert_close(ref[k], v, rtol=1e-12, atol=1e-13)
    # the export: LayerNorm, then the row over its norm
    got, _ = R.gather_rows(c["iid"], c["tables"]["mfi"], c["ln"]["mf_gamma"], c["ln"]["mf_beta"],
                           G.EPS, True)
    torch.testing.assert_close(got, yi / yi.norm(dim=1, keepdim=True), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("D", G.DIMS)
def test_embedding_bwd_float64_matches_autograd(D):
    """layer_norm over table[ids] and the dense table gradient (index_add) by autograd."""
    c = G.bwd_case(D, "struct", G.U, G.I)
    ref = c["ref"]
    pg = {q: torch.zeros(D, dtype=F64) for q in G.PARAMS}
    for k in R.TABLES:
        kind, t = k[-1], k[:-1]
        rows = G.U if kind == "u" else G.I
        uniq = c["uniq_" + kind]
        tab = torch.zeros(rows, D, dtype=F64)
        tab[uniq] = c["rows"][k].double()
        tab.requires_grad_(True)
        gam = c["gammas"][0 if t == "mf" else 1].double().requires_grad_(True)
        bet = torch.zeros(D, dtype=F64, requires_grad=True)
        y = torch.nn.functional.layer_norm(tab[c[kind + "id"]], (D,), gam, bet, G.EPS)
        y.backward(c["dys"][k].double())
        torch.testing.assert_close(ref["grads"][k], tab.grad[uniq], rtol=1e-10, atol=1e-11)
        assert int((tab.grad != 0).any(1).sum()) == uniq.numel()    # no other row has a gradient
        pg[t + "_gamma"] += gam.grad
        pg[t + "_beta"] += bet.grad
    for q in G.PARAMS:
        torch.testing.assert_close(ref[q], pg[q], rtol=1e-10, atol=1e-10)


def test_fp32_restatement_equals_float64_structure():
    """The piece-ordered restatement evaluated on float64-exact inputs (small integers) gives the
    reference's sums: the pieces partition every segment."""
    c = G.bwd_case(16, "struct", G.U, G.I)
    ints = {k: torch.randint(-8, 9, v.shape, generator=torch.Generator().manual_seed(1)).float()
            for k, v in c["dys"].items()}
    a = R.embedding_bwd(c["uid"], c["iid"], ints, c["rows"], c["gammas"], G.EPS, compact=True)
    b = R.embedding_bwd_f32(c["uid"], c["iid"], ints, c["rows"], c["gammas"], G.EPS, compact=True)
    for q in ("mf_beta", "mlp_beta"):       # sums of small integers: exact in both
        assert torch.equal(a[q].float(), b[q])
    for k in ("uniq_u", "uniq_i"):
        assert torch.equal(a[k], b[k])


# ----------------------------------------------------------------------------- the gather, fp32 and mutants
def gather_impl(norm=R.layer_norm, copy_odd_row=False, scale_mlp=True, oob_last=False):
    """The fp32 restatement as an implementation for G.check_gather; the arguments make the
    mutants: another LayerNorm, the row that leaves its group's user treated as a copy, the item
    scale on the GMF rows only, an out-of-range id clamped to the last row."""
    def impl(c, variant):
        with one_thread():
            return run(c, variant)

    def run(c, variant):
        tabs = {k: v.float() for k, v in c["tables_bf"].items()} if variant == "bf16" else c["tables"]
        uid, iid = c["uid"], c["iid"]
        if oob_last:
            uid = torch.where((uid < 0) | (uid >= G.U), torch.full_like(uid, G.U - 1), uid)
            iid = torch.where((iid < 0) | (iid >= G.I), torch.full_like(iid, G.I - 1), iid)
        kw = dict(eps=G.EPS, f=G.SCALE_F, G=c["G"], dtype=F32, norm=norm)
        scale = c["item_scale"] if variant == "scaled" else None
        out = R.gather_ln_gmf(uid, iid, tabs, c["ln"], c["w_mf"], c["b_mf"], item_scale=scale, **kw)
        if scale is not None and not scale_mlp:
            out["mlp_item_ln"] = R.gather_ln_gmf(uid, iid, tabs, c["ln"], c["w_mf"], c["b_mf"],
                                                 **kw)["mlp_item_ln"]
        src = R.source_rows(c["uid"], c["G"])
        if copy_odd_row:
            src[G.G_ODD_ROW] = False
        for k in ("mlp_user_ln", "mf_user_ln"):
            out[k] = torch.where(src[:, None], out[k], torch.full_like(out[k], NAN))
        out["err"] = int(c["bad"])
        return out
    return impl


@pytest.mark.parametrize("D", G.DIMS)
def test_gather_fp32_restatement_passes_with_headroom(D):
    for variant in G.GATHER_VARIANTS:
        for n, gr in sorted({(n, gr) for n, gr, _ in G.GATHER_RUNS}):
            worst = {}
            for bad in (False, True):       # (one entry of GATHER_FP32 for the two id lists)
                assert (n, gr, bad) in G.GATHER_RUNS
                G._merge(worst, G.check_gather(D, n, gr, bad, variant, gather_impl()))
            print(f"gather fp32 D {D} n {n} G {gr} {variant}: "
                  + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
            tag = (D, n, gr, variant)
            _headroom(tag, worst, G.GATHER_FP32.get(tag, {}))


def _norm_unbiased(x, gamma, beta, eps):
    D = x.shape[-1]
    xc = x - (R.row_sum(x) / D)[..., None]
    return xc / torch.sqrt(R.row_sum(xc * xc) / (D - 1) + eps)[..., None] * gamma + beta


def _norm_eps_outside(x, gamma, beta, eps):
    D = x.shape[-1]
    xc = x - (R.row_sum(x) / D)[..., None]
    return xc / (torch.sqrt(R.row_sum(xc * xc) / D) + eps)[..., None] * gamma + beta


# name: (n, group_rows, bad ids, variant, the mutant); every D
GATHER_MUTANTS = {
    "unbiased_var": (1003, 0, False, "plain", dict(norm=_norm_unbiased)),
    "eps_outside_root": (1003, 0, False, "plain", dict(norm=_norm_eps_outside)),
    "eps_outside_root_groups": (1000, 5, False, "bf16", dict(norm=_norm_eps_outside)),
    "odd_row_copied": (1000, 5, False, "ld", dict(copy_odd_row=True)),
    "scale_gmf_only": (1, 0, False, "scaled", dict(scale_mlp=False)),
    "oob_last_row": (1003, 0, True, "plain", dict(oob_last=True)),
    "oob_last_row_one": (1, 0, True, "scaled", dict(oob_last=True)),
}


@pytest.mark.parametrize("D", G.DIMS)
@pytest.mark.parametrize("name", list(GATHER_MUTANTS))
def test_gather_mutant_fails(name, D):
    n, gr, bad, variant, kw = GATHER_MUTANTS[name]
    assert (n, gr, bad) in G.GATHER_RUNS
    with pytest.raises(AssertionError):
        G.check_gather(D, n, gr, bad, variant, gather_impl(**kw))


def rows_impl(l2_first=False, oob_last=False, norm=R.layer_norm):
    def impl(c, entry, ln, l2):
        ids, tab = c["iid"], c["tables"]["mfi"]
        gam, bet = (c["ln"]["mf_gamma"], c["ln"]["mf_beta"]) if ln else (None, None)
        if oob_last:
            ids = torch.where((ids < 0) | (ids >= G.I), torch.full_like(ids, G.I - 1), ids)
        with one_thread():
            if l2_first and l2 and ln:
                x, _ = R.gather_rows(ids, tab, None, None, G.EPS, True, dtype=F32)
                return norm(x, gam.float(), bet.float(), G.EPS), int(c["bad"])
            return R.gather_rows(ids, tab, gam, bet, G.EPS, bool(l2), dtype=F32, norm=norm)[0], int(c["bad"])
    return impl


def test_gather_rows_fp32_restatement_and_mutants():
    total = {}
    for D in G.DIMS:
        for entry, ln, l2 in G.ROWS_RUNS:
            worst = {}
            for bad in (False, True):
                G._merge(worst, G.check_gather_rows(D, bad, entry, ln, l2, rows_impl()))
            listed = G.ROWS_FP32.get((D, ln, l2))
            _headroom((D, entry, ln, l2), worst, {} if listed is None else {"rows": listed})
            G._merge(total, worst)
        with pytest.raises(AssertionError):     # L2 normalisation taken before the LayerNorm
            G.check_gather_rows(D, False, "export", True, 1, rows_impl(l2_first=True))
        with pytest.raises(AssertionError):
            G.check_gather_rows(D, True, "rows", False, 0, rows_impl(oob_last=True))
        with pytest.raises(AssertionError):
            G.check_gather_rows(D, False, "export", True, 1, rows_impl(norm=_norm_eps_outside))
    print("gather_rows fp32: " + " ".join(f"{k} {v:.3g}" for k, v in total.items()))


# ----------------------------------------------------------------------------- the backward, fp32 and mutants
def bwd_impl(swap_gammas=False, **kw):
    def impl(c, mode, **_):
        gam = c["gammas"][::-1] if swap_gammas else c["gammas"]
        with one_thread():
            res = R.embedding_bwd_f32(c["uid"], c["iid"], c["dys"], c["rows"], gam, G.EPS,
                                      compact=True, **kw)
        return G.pad_bwd(c, res)
    return impl


# every (D, layout, num_users, num_items, bf16) the GPU tests run
def bwd_cases():
    cases = [(D, layout, G.U, G.I, False) for D in G.DIMS for layout in ("struct", "one", "two")]
    cases += [(256, "big256", 20000, 20000, False), (16, "big16", 60000, 60000, False)]
    cases += [(16, "struct", rows, G.I, False) for rows in (1 << 11, 300000, (1 << 22) + 1)]
    cases += [(D, "struct", G.U, G.I, True) for D in (16, 64, 256)]
    return cases


@pytest.mark.parametrize("case", bwd_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_embedding_bwd_fp32_restatement_passes_with_headroom(case):
    c = G.bwd_case(*case)
    worst = G.check_bwd(c, bwd_impl())
    print(f"embedding_bwd fp32 {case}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    D, layout, rows, _, bf16 = case
    _headroom(case, worst, G.BWD_FP32.get((D, layout, rows, bf16), {}))


def _lnbwd_no_m2(dy, x, gamma, eps):
    D = x.shape[-1]
    xc, rstd = R.ln_stats(x, eps)
    gd = dy * gamma
    return rstd[..., None] * (gd - (R.row_sum(gd) / D)[..., None]), xc * rstd[..., None]


def _lnbwd_unbiased(dy, x, gamma, eps):
    D = x.shape[-1]
    xc = x - (R.row_sum(x) / D)[..., None]
    rstd = 1.0 / torch.sqrt(R.row_sum(xc * xc) / (D - 1) + eps)
    h = xc * rstd[..., None]
    gd = dy * gamma
    m1, m2 = R.row_sum(gd) / D, R.row_sum(gd * h) / D
    return rstd[..., None] * (gd - m1[..., None] - h * m2[..., None]), h


BWD_MUTANTS = {
    "no_m2_term": dict(lnbwd=_lnbwd_no_m2),
    "unbiased_var": dict(lnbwd=_lnbwd_unbiased),
    "gammas_swapped": dict(swap_gammas=True),
    "last_extra_piece_dropped": dict(drop_last_extra=True),
    "dgamma_through_gamma": dict(dgamma_through_gamma=True),
}


@pytest.mark.parametrize("D", G.DIMS)
@pytest.mark.parametrize("name", list(BWD_MUTANTS))
def test_embedding_bwd_mutant_fails(name, D):
    with pytest.raises(AssertionError):
        G.check_bwd(G.bwd_case(D, "struct", G.U, G.I), bwd_impl(**BWD_MUTANTS[name]))


def test_embedding_bwd_small_mutants_fail():
    """The mutants that the smallest inputs already tell apart: n = 1 and one id twice."""
    for layout in ("one", "two"):
        for name in ("no_m2_term", "gammas_swapped", "dgamma_through_gamma"):
            with pytest.raises(AssertionError):
                G.check_bwd(G.bwd_case(256, layout, G.U, G.I), bwd_impl(**BWD_MUTANTS[name]))
    c = G.bwd_case(16, "struct", G.U, G.I)

    def writes_beyond(case, mode, **_):
        out = bwd_impl()(case, mode)
        out["grads"]["mlpi"][case["ref"]["uniq_i"].numel()] = 0.0
        return out
    with pytest.raises(AssertionError):
        G.check_bwd(c, writes_beyond)

    def one_id_short(case, mode, **_):
        out = bwd_impl()(case, mode)
        out["nu"][0] -= 1
        return out
    with pytest.raises(AssertionError):
        G.check_bwd(c, one_id_short)


# ----------------------------------------------------------------------------- what the cases contain
def test_struct_layout_contains_every_piece_shape():
    assert sum(G.STRUCT) == 603
    for D, rows in ((16, G.U), (256, G.U), (16, 300000), (16, (1 << 22) + 1)):
        c = G.bwd_case(D, "struct", rows, G.I)
        cov = G.coverage(c["sorted_u"])
        for k in ("split_pair", "whole_piece", "seventeen", "ten_pieces", "eighteen_pieces",
                  "singletons", "short_last_piece"):
            assert cov[k], (D, rows, k)
        assert cov["segments"] == len(G.STRUCT)
        assert G.coverage(c["sorted_i"])["eighteen_pieces"]       # (the reversed list)
        assert c["n"] == 603 and sorted(c["uid"].tolist()) == c["sorted_u"].tolist()
        assert not torch.equal(c["uid"], c["sorted_u"])            # permuted by position
        assert int(c["uniq_u"][0]) == 0 and int(c["uniq_u"][-1]) == rows - 1
    assert G.bwd_case(16, "one", G.U, G.I)["n"] == 1
    two = G.bwd_case(16, "two", G.U, G.I)
    assert two["n"] == 2 and int(two["uid"][0]) == int(two["uid"][1])


def test_pieces_restates_the_cut_rule():
    ids = torch.tensor([3] * 15 + [5] * 2 + [9] * 15 + [11] * 33)
    pc = R.pieces(ids)
    assert pc["start"].tolist() == [0, 15, 17, 32, 65]
    assert pc["pstart"].tolist() == [0, 15, 16, 17, 32, 48, 64, 65]
    assert pc["pseg"].tolist() == [0, 1, 1, 2, 3, 3, 3]
    assert pc["first"].tolist() == [True, True, False, True, True, False, False]
    assert pc["fpiece"].tolist() == [0, 1, 3, 4, 7]


def test_big_layouts_pass_the_grid_caps():
    """Restated from segments.h nbr_of and embedding_bwd.hip piece_reduce."""
    c = G.bwd_case(256, "big256", 20000, 20000)
    n = c["n"]
    assert n > 8192
    for kind in "ui":
        cov = G.coverage(c["sorted_" + kind])
        assert cov["pieces"] > 768 * 4                  # a second pass of the piece grid (D = 256:
        assert G.nbr_of(n, 256) == 768                  # one piece per wave, 4 waves per block)
        assert cov["segments"] > 2048 * 256 // 64       # a second sweep of the fix-up's segments
    assert (n * 64 + 255) // 256 > 2048 and G.fixup_blocks(n, 256) == 2048
    assert G.coverage(c["sorted_u"])["last_multi_piece_segment"] >= 2048 * 256 // 64
    c = G.bwd_case(16, "big16", 60000, 60000)
    for kind in "ui":
        assert G.coverage(c["sorted_" + kind])["pieces"] > 768 * 4 * 16 == 49152
    assert G.nbr_of(c["n"], 16) == 768 and G.fixup_blocks(c["n"], 16) < 2048
    # the small cases stay below both caps
    assert G.nbr_of(603, 16) == 11 and G.nbr_of(603, 256) == 161 and G.nbr_of(1, 256) == 1
    assert G.fixup_blocks(603, 256) == 151
    assert [G.sort_passes(r, G.I) for r in (G.U, 1 << 11, (1 << 11) + 1, 300000, 1 << 22, (1 << 22) + 1)] \
        == [1, 1, 2, 2, 2, 3]


def test_gather_cases_hold_their_rows():
    for D in G.DIMS:
        for n, gr, bad in G.GATHER_RUNS:
            c = G.gather_case(D, n, gr, bad)
            assert c["n"] == n == c["uid"].numel() == c["iid"].numel()
            oob = ((c["uid"] < 0) | (c["uid"] >= G.U)).sum() + ((c["iid"] < 0) | (c["iid"] >= G.I)).sum()
            assert int(oob) == (2 if bad and n > 1 else 2 * int(bad))
            if bad:
                assert int(c["iid"].max()) == G.I + 4 and int(c["uid"].min()) == -1
            for k in R.TABLES:
                row = c["tables"][k][G.U_CONST if k[-1] == "u" else G.I_CONST]
                assert bool((row == row[0]).all())
            if gr:
                first = c["uid"].view(-1, gr)[:, :1]
                assert int((c["uid"].view(-1, gr) != first).sum()) == 1 + int(bad)
    # 1003 rows: no multiple of a block's rows at any lane count (D / 4 or D / 8 lanes per row)
    assert all(1003 % (256 // lanes) for lanes in (2, 4, 8, 16, 32, 64))
