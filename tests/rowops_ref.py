"""The per-layer path's row operations restated in plain torch on the CPU — TEST INFRASTRUCTURE ONLY.

Restated from the reference module's definition (n x [Linear, ReLU, LayerNorm(h), Dropout(p)],
mlp_output Linear(h, 1), final Linear(2, 1) + Sigmoid, nn.BCELoss), not derived from the
kernels' output.  Every function takes ``dtype``: float64 is the reference, float32 the yardstick
a bound is measured with (tests/test_rowops_cpu.py).

* ``relu_ln_dropout_fwd`` / ``_bwd``: csrc/rowops.hip's contract.  ``r`` already holds
  relu(linear); the backward reads ReLU' from the stored ``r > 0`` (as the kernel does, so an
  op-level comparison needs no kink margin) and returns the pre-ReLU gradient with its column
  sums (the producing Linear's bias gradient) and the LayerNorm's dgamma / dbeta.  ``scales``:
  the keep-scales of the dropout ([n, W], tests/dropout_stream.keep_scales reshaped; None: p = 0).
* ``head_fwd`` / ``head_bwd``: csrc/head.hip's contract.  torch's BCE clamps both logs at -100,
  its backward is (x - t) / max((1 - x) x, 1e-12), the mean is over ``loss_denominator`` samples
  or, when that is 0, over n.
* ``gemm``: C = act(A . B + bias) (+ C0), the flags of ncf_gemm_rows / ncf_gemm_f32.
"""
import torch

LN_EPS = 1e-5
F_RELU, F_ACCUM = 1, 2


def _t(x, dtype):
    return None if x is None else torch.as_tensor(x).to(dtype)


def relu_ln_dropout_fwd(r, gamma, beta, eps, scales, dtype=torch.float64):
    """out = dropout(LayerNorm(r)), the row means and 1 / sqrt(var + eps) (biased variance)."""
    r, gamma, beta, scales = (_t(x, dtype) for x in (r, gamma, beta, scales))
    mean = r.mean(-1)
    var = ((r - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = (r - mean[:, None]) * rstd[:, None] * gamma + beta
    if scales is not None:
        out = out * scales
    return out, mean, rstd


def relu_ln_dropout_bwd(dout, r, gamma, scales, eps=LN_EPS, dtype=torch.float64, pos=None):
    """(dlin, dgamma, dbeta, dbias) of dropout -> LayerNorm -> ReLU from the gradient at the
    dropout's output; mean and rstd are recomputed in ``dtype``.  ``pos``: where ReLU' is 1
    (default: the stored r > 0)."""
    dout, r, gamma, scales = (_t(x, dtype) for x in (dout, r, gamma, scales))
    mean = r.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((r - mean) ** 2).mean(-1, keepdim=True) + eps)
    h = (r - mean) * rstd
    d = dout if scales is None else dout * scales
    gd = d * gamma
    dx = rstd * (gd - gd.mean(-1, keepdim=True) - h * (gd * h).mean(-1, keepdim=True))
    dlin = dx * (r > 0 if pos is None else pos).to(dtype)
    return dlin, (d * h).sum(0), d.sum(0), dlin.sum(0)


def head_fwd(a, w_out, b_out, mf_pred, w_fin, b_fin, dtype=torch.float64):
    """(mlp_pred, prob): mlp_output on the tower's last rows, final Linear(2, 1), sigmoid."""
    a, w_out, b_out, mf_pred, w_fin, b_fin = (_t(x, dtype) for x in
                                              (a, w_out, b_out, mf_pred, w_fin, b_fin))
    w_fin = w_fin.reshape(-1)
    mp = a @ w_out.reshape(-1) + b_out.reshape(-1)[0]
    return mp, torch.sigmoid(w_fin[0] * mf_pred + w_fin[1] * mp + b_fin.reshape(-1)[0])


def bce(prob, targets, den, clamp=-100.0):
    """nn.BCELoss with the sum divided by ``den``; both logs clamped at ``clamp`` (None: not)."""
    lp, lq = torch.log(prob), torch.log(1 - prob)
    if clamp is not None:
        lp, lq = torch.clamp(lp, min=clamp), torch.clamp(lq, min=clamp)
    return -(targets * lp + (1 - targets) * lq).sum() / den


def head_bwd(prob, mf_pred, mlp_pred, a, w_out, w_fin, u_ln, i_ln, w_mf, targets=None,
             grad_prob=None, loss_denominator=0.0, dtype=torch.float64):
    """The head's backward from ``prob`` as given.  Exactly one of ``targets`` (mean BCE: the
    loss is returned too) and ``grad_prob`` (dL/dprob from upstream; loss None)."""
    assert (targets is None) != (grad_prob is None)
    prob, mf_pred, mlp_pred, a, w_out, w_fin, u_ln, i_ln, w_mf, targets, grad_prob = (
        _t(x, dtype) for x in (prob, mf_pred, mlp_pred, a, w_out, w_fin, u_ln, i_ln, w_mf,
                               targets, grad_prob))
    n = prob.numel()
    w_out, w_fin, w_mf = w_out.reshape(-1), w_fin.reshape(-1), w_mf.reshape(-1)
    loss = None
    if targets is not None:
        den = loss_denominator if loss_denominator > 0 else n
        go = (prob - targets) / torch.clamp((1 - prob) * prob, min=1e-12) / den
        loss = bce(prob, targets, den)
    else:
        go = grad_prob
    dz = go * (1 - prob) * prob
    dmf, dml = dz * w_fin[0], dz * w_fin[1]
    return dict(da=dml[:, None] * w_out[None, :],
                du=(dmf[:, None] * w_mf[None, :]) * i_ln, di=(dmf[:, None] * w_mf[None, :]) * u_ln,
                dw_out=dml @ a, db_out=dml.sum().reshape(1),
                dw_mf=dmf @ (u_ln * i_ln), db_mf=dmf.sum().reshape(1),
                dw_fin=torch.stack([dz @ mf_pred, dz @ mlp_pred]), db_fin=dz.sum().reshape(1),
                loss=loss)


def gemm(A, B, bias, flags, C0=None, b_trans=1, dtype=torch.float64):
    """C[M, N] = act(A[M, K] . B + bias) (+ C0 when F_ACCUM); B is [N, K] when b_trans else
    [K, N]; ReLU (F_RELU) applies before the accumulate."""
    A, B, bias, C0 = (_t(x, dtype) for x in (A, B, bias, C0))
    C = A @ (B.t() if b_trans else B)
    if bias is not None:
        C = C + bias
    if flags & F_RELU:
        C = torch.relu(C)
    if flags & F_ACCUM:
        C = C + C0
    return C
