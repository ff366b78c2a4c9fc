"""The per-layer path's kernels, one at a time, against float64 (tests/rowops_ref.py), on the MI355X:
ncf_relu_ln_dropout_fwd/_bwd at every width rowops.hip dispatches, ncf_head_fwd/_bwd at the
widths head.hip accepts, ncf_gemm_rows at its eight (K, N) with padded leading dimensions.

Each check takes the implementation under test as an argument (tests/test_gpu_bf16.check_adam_bf16
is the pattern): here it is the kernel; tests/test_rowops_cpu.py runs the same check, on the same
inputs, with the fp32 restatement (which must pass with a quarter of every bound to spare) and
with mutants (which must fail).

Bounds, none fitted to the GPU's output: forward outputs rtol 1e-5 / atol 2e-6, gradients
rtol 2e-4 / atol 2e-6 (test_train_vs_oracle's), GEMM outputs test_gemm_vs_torch's
atol 1e-4 sqrt(K) / rtol 1e-4.  tests/test_rowops_cpu.py measures the fp32 restatement against
float64 under each; the figures stand in TOL's comments.
"""
import functools

import pytest
import torch

import _ncf_pkg
from tests import dropout_stream as S
from tests import rowops_ref as R

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")

# (rtol, atol).  The CPU's fp32 restatement against float64, worst case over every case below
# (tests/test_rowops_cpu.py asserts < 0.25): the head 0.07 of its bound (mlp_pred; gradients
# 0.016, loss 0.009), the GEMM 0.012; the row kernels below 0.25 (worst 0.2465, dbias at W = 128,
# n = 8201) except for the entries of RELU_FP32.
TOL = {"fwd": (1e-5, 2e-6), "grad": (2e-4, 2e-6)}
EPS = R.LN_EPS


def gemm_tol(K):
    return 1e-4, 1e-4 * K ** 0.5


def frac(got, want, tol):
    """The largest |got - want| as a fraction of atol + rtol |want| (nan / inf: inf)."""
    rtol, atol = tol
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    f = (got - want).abs() / (atol + rtol * want.abs())
    f = torch.where(torch.isfinite(f), f, torch.full_like(f, float("inf")))
    return float(f.max()) if f.numel() else 0.0


def _hold(worst, tag, name, got, want, tol, fp32=None):
    """``fp32``: the fp32 restatement's measured fraction of this bound where it is above a
    quarter; the bound of that quantity in that case is then 4 x that figure."""
    f = frac(got, want, tol)
    worst[name] = max(worst.get(name, 0.0), f)
    assert f < max(1.0, 4 * (fp32 or 0.0)), (tag, name, f)


# ----------------------------------------------------------------------------- relu -> LN -> dropout
WIDTHS = (16, 32, 64, 128, 256, 512, 1024)
RELU_MODES = ("thirds", "thirds_pad", "separate", "no_bias", "deferred")


# Where the fp32 restatement does not stay within a quarter of the project's bound: its measured
# worst fraction of that bound (this CPU, one host thread; tests/test_rowops_cpu.py re-measures
# it), and the case's bound for that quantity is 4 x the figure.  The rows with nearly all of r at
# zero (W = 16, 32: rstd up to 316) and the column sums over thousands of rows that nearly cancel.
RELU_FP32 = {
    (16, 65601, 0.0): {"dlin": 0.6151},
    (16, 65601, 0.25): {"dlin": 0.6228},
    (32, 32801, 0.0): {"dlin": 0.327},
    (32, 32801, 0.25): {"dlin": 0.3158},
    (256, 4101, 0.0): {"dgamma": 0.7627},
    (256, 4101, 0.25): {"dgamma": 0.4542, "dbias": 3.057},
    (512, 4101, 0.0): {"dgamma": 0.5643, "dbeta": 0.2995},
    (512, 4101, 0.25): {"out": 0.2905},
    (1024, 4101, 0.0): {"dgamma": 0.432, "dbeta": 0.8213},
    (1024, 4101, 0.25): {"out": 0.3128, "dgamma": 0.2973, "dbeta": 0.7296, "dbias": 0.2698},
}


def row_slots(W):
    """Row slots of a backward block: 256 threads / min(64, W / 4) lanes per row."""
    return 256 // min(64, W // 4)


def bwd_rows_per_block(n, W):
    """rowops.hip's bwd_rows_per_block: about 1024 blocks, a multiple of the row slots."""
    s = row_slots(W)
    rpb = (n + 1023) // 1024
    return max(s, (rpb + s - 1) // s * s)


def relu_rows(W):
    """n = 1; a ragged second block; past 1024 x slots rows, where the backward's row loop makes
    a second pass and the last block is short (4101 for W >= 256, 65601 for W = 16)."""
    s = row_slots(W)
    return (1, s + 3, 1025 * s + 1)


@functools.lru_cache(maxsize=2)
def relu_case(W, n, p):
    """Inputs (r = relu(randn): half exact zeros; gamma, beta random) and the float64 results."""
    g = torch.Generator().manual_seed(7919 * W + n)
    c = dict(W=W, n=n, p=p, seed=(0x2545F491 << 30) + 977 * W + n,
             r=torch.relu(torch.randn(n, W, generator=g)), gamma=0.5 + torch.rand(W, generator=g),
             beta=torch.randn(W, generator=g), dout=torch.randn(n, W, generator=g))
    c["scales"] = torch.from_numpy(S.keep_scales(c["seed"], n * W, p).reshape(n, W)) if p > 0 else None
    out, mean, rstd = R.relu_ln_dropout_fwd(c["r"], c["gamma"], c["beta"], EPS, c["scales"])
    dlin, dgamma, dbeta, dbias = R.relu_ln_dropout_bwd(c["dout"], c["r"], c["gamma"], c["scales"], EPS)
    c["ref"] = dict(out=out, mean=mean, rstd=rstd, dlin=dlin, dgamma=dgamma, dbeta=dbeta, dbias=dbias)
    return c


def check_relu_ln(W, n, p, impl, modes=RELU_MODES):
    """``impl(case, modes)`` -> {mode: dict(out, mean, rstd, dlin, dgamma, dbeta, dbias)} (fp32;
    dbias None in mode "no_bias").  Every mode against float64; "deferred" equals "thirds" bit for
    bit; the dropout drops about p of the elements that r leaves non-zero.  Returns the worst
    fraction of its bound per quantity."""
    c = relu_case(W, n, p)
    res = impl(c, modes)
    worst, ref = {}, c["ref"]
    for mode in modes:
        got, tag = res[mode], (W, n, p, mode)
        fp32 = RELU_FP32.get((W, n, p), {})
        for k in ("out", "mean", "rstd"):
            _hold(worst, tag, k, got[k], ref[k], TOL["fwd"], fp32.get(k))
        for k in ("dlin", "dgamma", "dbeta", "dbias"):
            if k == "dbias" and mode == "no_bias":
                assert got[k] is None
                continue
            _hold(worst, tag, k, got[k], ref[k], TOL["grad"], fp32.get(k))
        assert bool((got["dlin"][c["r"] == 0] == 0).all()), tag     # ReLU' from r > 0
    if "deferred" in modes and "thirds" in modes:
        for k in ("dlin", "dgamma", "dbeta", "dbias"):
            assert torch.equal(res["deferred"][k], res["thirds"][k]), (W, n, p, k)
    if p > 0:
        # (LayerNorm's output is 0 nowhere on these inputs: every 0 of out is a dropped element)
        out, live = res[modes[0]]["out"], c["r"] > 0
        cnt = int(live.sum())
        if cnt:
            dropped = float((out[live] == 0).double().mean())
            want = S.drop_threshold(p) / 65536
            assert abs(dropped - want) < 4 * (want * (1 - want) / cnt) ** 0.5, (W, n, p, dropped)
            assert bool(((out == 0) == (c["scales"] == 0)).all())
    return worst


def gpu_relu_ln(c, modes):
    from ncf_amd import _lib
    W, n, p, seed = c["W"], c["n"], c["p"], c["seed"]
    st = _lib.stream_ptr(DEV)
    f = dict(device=DEV, dtype=torch.float32)
    r, gamma, beta, dout = (c[k].to(DEV) for k in ("r", "gamma", "beta", "dout"))
    nan = lambda *s: torch.full(s, float("nan"), **f)  # noqa: E731
    out, mean, rstd = nan(n, W), nan(n), nan(n)
    _lib.call("ncf_relu_ln_dropout_fwd", r.data_ptr(), n, W, gamma.data_ptr(), beta.data_ptr(), EPS,
              p, seed, None, out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), st)
    assert torch.equal(r.cpu(), c["r"])         # (the input is read only)
    fwd = dict(out=out.cpu(), mean=mean.cpu(), rstd=rstd.cpu())
    need = _lib.query("ncf_relu_ln_dropout_bwd_workspace", n, W)
    res = {}
    for mode in modes:
        ws, dlin = nan(need), nan(n, W)
        keep, lst = [], None
        if mode == "separate":      # three allocations, not equally spaced
            db, dg, de = nan(W), nan(W), nan(W)
            while dg.data_ptr() - db.data_ptr() == de.data_ptr() - dg.data_ptr():
                keep.append(de)
                de = nan(W)
        else:                       # equally spaced thirds of one buffer, W or W + 8 apart
            sp = W + 8 if mode == "thirds_pad" else W
            buf = nan(3 * sp)
            db, dg, de = buf[0:W], buf[sp:sp + W], buf[2 * sp:2 * sp + W]
        if mode == "deferred":
            lst = _lib.ReduceList()
            lst.count = 0
        _lib.call("ncf_relu_ln_dropout_bwd", dout.data_ptr(), r.data_ptr(), mean.data_ptr(),
                  rstd.data_ptr(), gamma.data_ptr(), n, W, p, seed, None, dlin.data_ptr(),
                  dg.data_ptr(), de.data_ptr(), None if mode == "no_bias" else db.data_ptr(),
                  ws.data_ptr(), need, None if lst is None else lst.address, st)
        if lst is not None:
            assert lst.count == 1       # (equally spaced: one strided descriptor)
            sneed = _lib.query("ncf_reduce_batch_scratch", lst.address)
            scratch = nan(max(sneed, 1))
            _lib.call("ncf_reduce_batch", lst.address, scratch.data_ptr(), scratch.numel(), st)
        torch.cuda.synchronize()
        if mode == "thirds_pad":        # the 8 floats between the thirds stay untouched
            assert bool(torch.isnan(buf[W:sp]).all()) and bool(torch.isnan(buf[sp + W:2 * sp]).all())
        if mode == "no_bias":
            assert bool(torch.isnan(db).all())
        res[mode] = dict(fwd, dlin=dlin.cpu(), dgamma=dg.cpu().clone(), dbeta=de.cpu().clone(),
                         dbias=None if mode == "no_bias" else db.cpu().clone())
    return res


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("W", WIDTHS)
def test_relu_ln_dropout_vs_float64(W, p):
    for n in relu_rows(W):
        worst = check_relu_ln(W, n, p, gpu_relu_ln)
        print(f"relu_ln W {W} n {n} p {p}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- the head
HEAD_DIMS = ((16, 16), (64, 64), (256, 256), (256, 16), (32, 128))
HEAD_ROWS = (1, 15, 17, 50)
# targets: the mean BCE over n; targets_den: over loss_denominator = 3 n; grad_prob: dL/dprob
# given; edge (n >= 4): targets with prob exactly 0, 0, 1, 1 under targets 1, 0, 1, 0
HEAD_MODES = ("targets", "targets_den", "grad_prob", "edge")
HEAD_GRADS = ("da", "du", "di", "dw_out", "db_out", "dw_mf", "db_mf", "dw_fin", "db_fin")


@functools.lru_cache(maxsize=4)
def head_case(width, dim, n, mode):
    g = torch.Generator().manual_seed(31 * width + 7 * dim + n)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(width=width, dim=dim, n=n, mode=mode, a=rn(n, width), w_out=rn(width) / width ** 0.5,
             b_out=rn(1), mf_pred=rn(n), w_fin=rn(2), b_fin=rn(1), u_ln=rn(n, dim), i_ln=rn(n, dim),
             w_mf=rn(dim) / dim ** 0.5, targets=(torch.rand(n, generator=g) < 0.3).float(),
             grad_prob=rn(n) / n, den=3.0 * n if mode == "targets_den" else 0.0)
    mp, prob = R.head_fwd(c["a"], c["w_out"], c["b_out"], c["mf_pred"], c["w_fin"], c["b_fin"])
    c["fwd"] = dict(mlp_pred=mp, prob=prob)
    # the backward's inputs: the float64 forward rounded to fp32 (the same bits for every
    # implementation), with the exact 0 / 1 rows of the edge case
    c["mlp_pred"], c["prob"] = mp.float(), prob.float()
    if mode == "edge":
        c["prob"][:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        c["targets"][:4] = torch.tensor([1.0, 0.0, 1.0, 0.0])
    kw = dict(grad_prob=c["grad_prob"]) if mode == "grad_prob" else \
        dict(targets=c["targets"], loss_denominator=c["den"])
    c["bwd"] = R.head_bwd(c["prob"], c["mf_pred"], c["mlp_pred"], c["a"], c["w_out"], c["w_fin"],
                          c["u_ln"], c["i_ln"], c["w_mf"], **kw)
    return c


def check_head(width, dim, n, mode, impl):
    """``impl(case, defer)`` -> dict(mlp_pred, prob, the HEAD_GRADS, loss (None under grad_prob)),
    run inline and through the deferred list.  Returns the worst fraction per quantity."""
    c = head_case(width, dim, n, mode)
    worst = {}
    for defer in (False, True):
        got, tag = impl(c, defer), (width, dim, n, mode, defer)
        for k in ("mlp_pred", "prob"):
            _hold(worst, tag, k, got[k], c["fwd"][k], TOL["fwd"])
        for k in HEAD_GRADS:
            assert bool(torch.isfinite(got[k]).all()), (tag, k)
            _hold(worst, tag, k, got[k], c["bwd"][k], TOL["grad"])
        if mode == "grad_prob":
            assert got["loss"] is None
        else:
            _hold(worst, tag, "loss", got["loss"], c["bwd"]["loss"], TOL["fwd"])
        if mode == "edge":
            # the clamped loss: 100 for each of the two rows on the wrong side, and no gradient
            # from a saturated row (dz = go (1 - o) o = 0)
            rest = R.bce(c["prob"][4:].double(), c["targets"][4:].double(), n)
            assert abs(float(c["bwd"]["loss"]) - (200.0 / n + float(rest))) < 1e-9
            for k in ("da", "du", "di"):
                assert bool((got[k][:4] == 0).all()), (tag, k)
    return worst


def gpu_head(c, defer):
    from ncf_amd import _lib
    width, dim, n, mode = c["width"], c["dim"], c["n"], c["mode"]
    st = _lib.stream_ptr(DEV)
    f = dict(device=DEV, dtype=torch.float32)
    nan = lambda *s: torch.full(s, float("nan"), **f)  # noqa: E731
    d = {k: c[k].to(DEV) for k in ("a", "w_out", "b_out", "mf_pred", "w_fin", "b_fin", "u_ln", "i_ln",
                                   "w_mf", "targets", "grad_prob", "prob", "mlp_pred")}
    p = lambda k: d[k].data_ptr()  # noqa: E731
    mp, prob = nan(n), nan(n)
    _lib.call("ncf_head_fwd", p("a"), n, width, p("w_out"), p("b_out"), p("mf_pred"), p("w_fin"),
              p("b_fin"), mp.data_ptr(), prob.data_ptr(), st)
    o = dict(da=nan(n, width), du=nan(n, dim), di=nan(n, dim), dw_out=nan(width), db_out=nan(1),
             dw_mf=nan(dim), db_mf=nan(1), dw_fin=nan(2), db_fin=nan(1), loss=nan(1))
    q = lambda k: o[k].data_ptr()  # noqa: E731
    need = _lib.query("ncf_head_bwd_workspace", n, width, dim)
    ws = nan(need)
    lst = None
    if defer:
        lst = _lib.ReduceList()
        lst.count = 0
    gp = mode == "grad_prob"
    _lib.call("ncf_head_bwd", p("prob"), p("grad_prob") if gp else None, None if gp else p("targets"),
              p("mf_pred"), p("mlp_pred"), p("a"), n, width, p("w_out"), p("w_fin"), p("u_ln"),
              p("i_ln"), dim, p("w_mf"), q("da"), q("du"), q("di"), q("dw_out"), q("db_out"),
              q("dw_mf"), q("db_mf"), q("dw_fin"), q("db_fin"), None if gp else q("loss"),
              float(c["den"]), ws.data_ptr(), need, None if lst is None else lst.address, st)
    if lst is not None:
        assert lst.count == (6 if gp else 7)
        sneed = _lib.query("ncf_reduce_batch_scratch", lst.address)
        scratch = nan(max(sneed, 1))
        _lib.call("ncf_reduce_batch", lst.address, scratch.data_ptr(), scratch.numel(), st)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out["loss"] = None if gp else out["loss"][0]
    out.update(mlp_pred=mp.cpu(), prob=prob.cpu())
    return out


def head_cases():
    return [(w, d, n, m) for w, d in HEAD_DIMS for n in HEAD_ROWS for m in HEAD_MODES
            if not (m == "edge" and n < 4)]


@pytest.mark.parametrize("width,dim", HEAD_DIMS)
def test_head_vs_float64(width, dim):
    total = {}
    for w, d, n, mode in head_cases():
        if (w, d) == (width, dim):
            for k, v in check_head(w, d, n, mode, gpu_head).items():
                total[k] = max(total.get(k, 0.0), v)
    print(f"head {width} {dim}: " + " ".join(f"{k} {v:.3g}" for k, v in total.items()))


# ----------------------------------------------------------------------------- ncf_gemm_rows
GEMM_KN = ((64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (128, 256), (256, 64), (256, 128))
GEMM_ROWS = (1, 31, 33, 130)
# past one sweep of the (64, 64) grid: 1024 workgroups x 4 tiles x 32 rows = 131072
GEMM_WRAP = (64, 64, 131117)
PAD = 4


@functools.lru_cache(maxsize=2)
def gemm_case(K, N, M, b_trans, flags):
    """Padded operands (lda = K + 4, ldc = N + 4, ldb 4 past tight), a bias unless the call only
    accumulates, C preset (the accumulate's addend, and the padding that must survive)."""
    g = torch.Generator().manual_seed(K * 1000 + N + M + 17 * b_trans + flags)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(K=K, N=N, M=M, b_trans=b_trans, flags=flags, A=rn(M, K + PAD),
             B=rn(N, K + PAD) if b_trans else rn(K, N + PAD), C0=rn(M, N + PAD),
             bias=None if flags == R.F_ACCUM else rn(N))
    Bv = c["B"][:, :K] if b_trans else c["B"][:, :N]
    c["ref"] = R.gemm(c["A"][:, :K], Bv, c["bias"], flags, c["C0"][:, :N], b_trans)
    return c


def check_gemm_rows(K, N, M, b_trans, flags, impl):
    """``impl(case)`` -> the whole C buffer [M, N + 4] after the call."""
    c = gemm_case(K, N, M, b_trans, flags)
    got = impl(c)
    assert got.shape == c["C0"].shape
    assert torch.equal(got[:, N:].view(torch.int32), c["C0"][:, N:].view(torch.int32)), \
        (K, N, M, b_trans, flags, "padding columns of C written")
    f = frac(got[:, :N], c["ref"], gemm_tol(K))
    assert f < 1.0, (K, N, M, b_trans, flags, f)
    return f


def gpu_gemm_rows(c):
    from ncf_amd import _lib
    K, N, M = c["K"], c["N"], c["M"]
    A, B, C = c["A"].to(DEV), c["B"].to(DEV), c["C0"].to(DEV)
    bias = None if c["bias"] is None else c["bias"].to(DEV)
    _lib.call("ncf_gemm_rows", M, N, K, A.data_ptr(), A.shape[1], B.data_ptr(), B.shape[1],
              c["b_trans"], C.data_ptr(), C.shape[1], None if bias is None else bias.data_ptr(),
              c["flags"], _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return C.cpu()


@pytest.mark.parametrize("K,N", GEMM_KN)
def test_gemm_rows_vs_float64(K, N):
    worst = 0.0
    for M in GEMM_ROWS:
        for b_trans in (0, 1):
            for flags in (0, 1, 2, 3):
                worst = max(worst, check_gemm_rows(K, N, M, b_trans, flags, gpu_gemm_rows))
    print(f"gemm_rows ({K}, {N}): {worst:.3g} of its tolerance")


def test_gemm_rows_tile_loop_wraps():
    K, N, M = GEMM_WRAP
    f = check_gemm_rows(K, N, M, 1, R.F_RELU, gpu_gemm_rows)
    print(f"gemm_rows wrap: {f:.3g} of its tolerance")


def test_gemm_rows_refusals():
    """(256, 256) and a misaligned A are refused with an error before any launch."""
    from ncf_amd import _lib
    st = _lib.stream_ptr(DEV)
    A, B, C = (torch.zeros(64 * 256 + 4, device=DEV) for _ in range(3))
    with pytest.raises(ValueError, match=r"unsupported \(K=256, N=256\)"):
        _lib.call("ncf_gemm_rows", 32, 256, 256, A.data_ptr(), 256, B.data_ptr(), 256, 1,
                  C.data_ptr(), 256, None, 0, st)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("ncf_gemm_rows", 32, 64, 64, A[1:].data_ptr(), 64, B.data_ptr(), 64, 1,
                  C.data_ptr(), 64, None, 0, st)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("ncf_gemm_rows", 32, 64, 64, A.data_ptr(), 66, B.data_ptr(), 64, 1,
                  C.data_ptr(), 64, None, 0, st)
    torch.cuda.synchronize()
    assert float(C.abs().max()) == 0.0
