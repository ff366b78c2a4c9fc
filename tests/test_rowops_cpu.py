"""The premises of tests/test_gpu_rowops.py, without a GPU: on every case of every check there,
the fp32 restatement (tests/rowops_ref.py evaluated in float32) passes with a quarter of each
bound to spare, and the mutants a subtly wrong kernel would be fail the same check on the same
inputs.  Also: ncf_head_bwd's partial layout fits its LDS image at every accepted (width, dim)."""
import contextlib
import os
import re

import pytest
import torch

from tests import rowops_ref as R
from tests import test_gpu_rowops as G

F32 = torch.float32


@contextlib.contextmanager
def one_thread():
    """torch's threaded CPU reductions do not fix their order (test_gpu_fullsize): the measured
    figures are one host thread's."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


# ----------------------------------------------------------------------------- relu -> LN -> dropout
def relu_impl(fwd=R.relu_ln_dropout_fwd, scales=None, pos=None, dgamma_rows=None):
    """The fp32 restatement as an implementation for G.check_relu_ln; the arguments make the
    mutants: another forward, other keep-scales ``scales(case)``, another ReLU' ``pos(r)``,
    dgamma from the first ``dgamma_rows(case)`` rows only."""
    def impl(c, modes):
        with one_thread():
            return run(c, modes)

    def run(c, modes):
        s = c["scales"] if scales is None else scales(c)
        out, mean, rstd = fwd(c["r"], c["gamma"], c["beta"], G.EPS, s, dtype=F32)
        dlin, dgamma, dbeta, dbias = R.relu_ln_dropout_bwd(
            c["dout"], c["r"], c["gamma"], s, G.EPS, dtype=F32,
            pos=None if pos is None else pos(c["r"]))
        if dgamma_rows is not None:
            k = dgamma_rows(c)
            dgamma = R.relu_ln_dropout_bwd(c["dout"][:k], c["r"][:k], c["gamma"],
                                           None if s is None else s[:k], G.EPS, dtype=F32)[1]
        one = dict(out=out, mean=mean, rstd=rstd, dlin=dlin, dgamma=dgamma, dbeta=dbeta, dbias=dbias)
        return {m: dict(one, dbias=None) if m == "no_bias" else one for m in modes}
    return impl


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("W", G.WIDTHS)
def test_relu_ln_fp32_restatement_passes_with_headroom(W, p):
    for n in G.relu_rows(W):
        worst = G.check_relu_ln(W, n, p, relu_impl())
        print(f"relu_ln fp32 W {W} n {n} p {p}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        listed = G.RELU_FP32.get((W, n, p), {})
        for k, v in worst.items():
            # a quarter of the project's bound, or the figure recorded beside the case
            assert v < 0.25 or (k in listed and v <= 1.001 * listed[k]), (W, n, p, k, v)
        for k, v in listed.items():     # no bound wider than 4 x what is measured here
            assert 0.25 <= v <= 1.001 * worst[k], (W, n, p, k, v, worst[k])


def test_relu_rows_reach_the_second_pass():
    """The largest n of each width gives a backward block more rows than it has row slots (a lane
    group's row loop runs twice), and a last block that is short."""
    assert G.relu_rows(16)[2] == 65601 and G.relu_rows(256)[2] == G.relu_rows(1024)[2] == 4101
    for W in G.WIDTHS:
        s = G.row_slots(W)
        n = G.relu_rows(W)[2]
        rpb = G.bwd_rows_per_block(n, W)
        assert n > 1024 * s and rpb == 2 * s and 0 < n % rpb < rpb
        n = G.relu_rows(W)[1]
        assert G.bwd_rows_per_block(n, W) == s and n % s == 3


def _unbiased_fwd(r, gamma, beta, eps, scales, dtype):
    r = r.to(dtype)
    mean = r.mean(-1)
    rstd = 1.0 / torch.sqrt(r.var(-1, unbiased=True) + eps)
    out = (r - mean[:, None]) * rstd[:, None] * gamma + beta
    return (out if scales is None else out * scales), mean, rstd


def _chunk0_scales(c):
    """The keep-scale of float4 chunk c of a lane taken from chunk 0's index."""
    span = 4 * min(64, c["W"] // 4)
    return c["scales"][:, torch.arange(c["W"]) % span]


def _without_last_block(c):
    rpb = G.bwd_rows_per_block(c["n"], c["W"])
    return (c["n"] - 1) // rpb * rpb


RELU_MUTANTS = {
    # a relative error of 1 / (2 (W - 1)) = 5e-4 in rstd at W = 1024, the hardest case
    "unbiased_var": (1024, 1, 0.0, dict(fwd=_unbiased_fwd)),
    "unbiased_var_rows": (1024, 4101, 0.25, dict(fwd=_unbiased_fwd)),
    "chunk0_scale_512": (512, 7, 0.25, dict(scales=_chunk0_scales)),
    "chunk0_scale_1024": (1024, 4101, 0.25, dict(scales=_chunk0_scales)),
    "relu_ge": (16, 67, 0.0, dict(pos=lambda r: r >= 0)),
    "relu_ge_1024": (1024, 1, 0.25, dict(pos=lambda r: r >= 0)),
    "dgamma_last_block": (64, 19, 0.0, dict(dgamma_rows=_without_last_block)),
    "dgamma_last_block_rows": (16, 65601, 0.25, dict(dgamma_rows=_without_last_block)),
}


@pytest.mark.parametrize("name", list(RELU_MUTANTS))
def test_relu_ln_mutant_fails(name):
    W, n, p, kw = RELU_MUTANTS[name]
    assert n in G.relu_rows(W)
    with pytest.raises(AssertionError):
        G.check_relu_ln(W, n, p, relu_impl(**kw), modes=("thirds",))


# ----------------------------------------------------------------------------- the head
def head_impl(clamp=-100.0, use_den=True):
    def impl(c, defer):
        mp, prob = R.head_fwd(c["a"], c["w_out"], c["b_out"], c["mf_pred"], c["w_fin"], c["b_fin"],
                              dtype=F32)
        den = c["den"] if use_den else 0.0
        kw = dict(grad_prob=c["grad_prob"]) if c["mode"] == "grad_prob" else \
            dict(targets=c["targets"], loss_denominator=den)
        out = R.head_bwd(c["prob"], c["mf_pred"], c["mlp_pred"], c["a"], c["w_out"], c["w_fin"],
                         c["u_ln"], c["i_ln"], c["w_mf"], dtype=F32, **kw)
        if clamp is None and out["loss"] is not None:
            out["loss"] = R.bce(c["prob"], c["targets"], den if den > 0 else c["n"], clamp=None)
        return dict(out, mlp_pred=mp, prob=prob)
    return impl


def test_head_fp32_restatement_passes_with_headroom():
    total = {}
    for w, d, n, mode in G.head_cases():
        for k, v in G.check_head(w, d, n, mode, head_impl()).items():
            total[k] = max(total.get(k, 0.0), v)
    print("head fp32: " + " ".join(f"{k} {v:.3g}" for k, v in total.items()))
    assert max(total.values()) < 0.25, total
    assert {n for _, _, n, m in G.head_cases() if m == "edge"} == {15, 17, 50}


@pytest.mark.parametrize("width,dim", G.HEAD_DIMS)
def test_head_mutants_fail(width, dim):
    with pytest.raises(AssertionError):     # log(0) unclamped: the loss is inf or nan
        G.check_head(width, dim, 17, "edge", head_impl(clamp=None))
    for n in G.HEAD_ROWS:                   # the mean over n where 3 n was given
        with pytest.raises(AssertionError):
            G.check_head(width, dim, n, "targets_den", head_impl(use_den=False))


def test_head_bwd_partials_fit_the_lds_image():
    """k_head_bwd keeps P = W3 + D + 6 floats per wave in red[4][...]: inside it for every last
    width and MF dim ncf_head_bwd accepts (each at most 256)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "neural-collaborative-filtering-demo_amd", "csrc", "head.hip")
    with open(src) as fh:
        text = fh.read()
    m = re.search(r"__shared__ float red\[4\]\[(\d+) \+ (\d+) \+ (\d+)\]", text)
    size = sum(int(x) for x in m.groups())
    assert size == 520
    assert "width <= 256 && dim >= 1 && dim <= 256" in text
    for W3 in (16, 32, 64, 128, 256):
        for D in (16, 32, 64, 128, 256):
            assert W3 + D + 6 <= size
    assert 256 + 256 + 6 == 518


# ----------------------------------------------------------------------------- ncf_gemm_rows
def gemm_impl(k_steps=None, accumulate=True):
    def impl(c):
        K, N = c["K"], c["N"]
        kk = K if k_steps is None else k_steps(K)
        Bv = c["B"][:, :kk] if c["b_trans"] else c["B"][:kk, :N]
        flags = c["flags"] if accumulate else c["flags"] & ~R.F_ACCUM
        C = c["C0"].clone()
        C[:, :N] = R.gemm(c["A"][:, :kk], Bv, c["bias"], flags, c["C0"][:, :N], c["b_trans"], dtype=F32)
        return C
    return impl


def _gemm_cases():
    return [(K, N, M, b, f) for K, N in G.GEMM_KN for M in G.GEMM_ROWS for b in (0, 1)
            for f in (0, 1, 2, 3)] + [G.GEMM_WRAP + (1, R.F_RELU)]


def test_gemm_fp32_restatement_passes_with_headroom():
    worst = max(G.check_gemm_rows(*case, gemm_impl()) for case in _gemm_cases())
    print(f"gemm fp32: {worst:.3g} of its tolerance")
    assert worst < 0.25
    K, N, M = G.GEMM_WRAP       # the (64, 64) grid: 1024 workgroups of 4 row tiles of 32 rows
    assert (M + 31) // 32 > 1024 * 4


def test_gemm_mutants_fail():
    for K, N, M, b, f in _gemm_cases():
        with pytest.raises(AssertionError):     # the last k step dropped
            G.check_gemm_rows(K, N, M, b, f, gemm_impl(k_steps=lambda K: K - 1))
        if f & R.F_ACCUM:
            with pytest.raises(AssertionError):     # an accumulate that overwrites
                G.check_gemm_rows(K, N, M, b, f, gemm_impl(accumulate=False))

    def writes_padding(c):
        C = gemm_impl()(c)
        C[:, c["N"]] = 0.0
        return C
    with pytest.raises(AssertionError):
        G.check_gemm_rows(64, 64, 33, 1, 0, writes_padding)
