"""The bf16 MLP tower's arithmetic restated in plain torch on the CPU — TEST INFRASTRUCTURE ONLY.

Restated from csrc/mlp_tower_dev.h with MM == 1 (ncf_mlp_fwd_bf16 / ncf_mlp_bwd_bf16, tower mode
1 of ncf_attn_mlp_fwd / _bwd), not derived from its output:

* lin_fwd: y = bf(x) . bf(W)^T + b.  Both operands are rounded to bf16, nearest even (pk8's
  ``(__bf16)x``); the products are exact in fp32, the accumulation and the bias add are fp32.
* lin_bwd: dx = bf(dlin) . bf(W).
* wgrad_layer<..., 1> (the weight gradients fused into the tower backward, engine.MLP_WGRAD):
  dW = bf(dlin)^T . bf(a) (pk4).  With MLP_WGRAD off the weight gradients are wgrad.hip's fp32
  MFMA on the stored fp32 dlin and a: dW = dlin^T . a, nothing rounded (``dw_unrounded`` below).
* ReLU, LayerNorm forward and backward, dropout, the head, BCE and the bias / gamma / beta sums
  stay fp32.

Two uses.  ``make_linear()`` is the ``linear=`` of oracle/ncf_oracle.py's forward / train_step:
the end-to-end float64 reference of a bf16 step.  ``tower_checks`` is the teacher-forced,
layer-by-layer comparison: every reference layer is evaluated in float64 from the fp32 bits the
step under test itself produced one stage earlier, so a correct step differs from it by fp32
accumulation order only (rounding is discontinuous: end to end, a 1e-7 difference upstream moves
an operand by a whole bf16 step).  ``tower_chain`` evaluates the same formulas stage after stage
in one dtype: the CPU stand-in for the GPU, with a wrong rounding in chosen layers on request.

Bounds.  u = 2^-24.  Any fp32 accumulation of K products, in any order, is within
(K - 1) u sum|a_k b_k| of the exact sum (to first order); ``gemm_bound`` is
(K + 8) u (|A| |B|^T + |b|), the 8 for the bias add, the stores, a second reduction over
workgroups and products that are not exact (wgrad.hip's fp32 operands).  A column sum over n
rows is within (n + 8) u of the sum of magnitudes.  The LayerNorm backward is linear in its
incoming gradient: an elementwise bound on that gradient goes through the same formula on
magnitudes (``ln_bwd``'s ``bound``), and the row's own fp32 arithmetic (sums of N terms) adds
(N + 16) u of the magnitudes.  These come from the number format, not from any output; they sit
one to three orders below the project's fp32 tolerances (``ISSUE_TOL``), which are asserted too.
"""
from collections import namedtuple

import torch

from oracle import ncf_oracle as O

U24 = 2.0 ** -24
EPS = O.LN_EPS
# the project's fp32-against-float64 tolerances: test_gemm_vs_torch's form for a GEMM output
# (atol 1e-4 sqrt(K), rtol 1e-4), test_train_vs_oracle's for row operations and gradients
ISSUE_TOL = {"gemm": lambda K: (1e-4 * K ** 0.5, 1e-4), "row": lambda K: (2e-6, 2e-4)}


def bf(x):
    """Round to bf16, nearest even, and widen to the dtype given."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def bf_trunc(x):
    """The wrong convert: the low 16 bits of the fp32 value masked off."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def _same(x):
    return x


# which operand of which product is rounded how: forward x and W, dX's dlin and W, dW's dlin and x
Rounding = namedtuple("Rounding", "fx fw bdy bw wdy wx")
RNE = Rounding(bf, bf, bf, bf, bf, bf)
VARIANTS = {
    "trunc": Rounding(*[bf_trunc] * 6),
    "w_unrounded": RNE._replace(fw=_same, bw=_same),
    "a_unrounded": RNE._replace(fx=_same, wx=_same),
    "bwd_unrounded": RNE._replace(bdy=_same, bw=_same, wdy=_same, wx=_same),
    "dw_unrounded": RNE._replace(wdy=_same, wx=_same),
}
UNROUNDED = Rounding(*[_same] * 6)


def rounding(variant=None):
    return RNE if variant is None else VARIANTS[variant]


class _BF16Linear(torch.autograd.Function):
    """y = fx(x) fw(w)^T + b with the backward the kernels compute, not the derivative of the
    forward (which is 0 almost everywhere in the rounded operands)."""

    @staticmethod
    def forward(ctx, x, w, b, rd):
        ctx.save_for_backward(x, w)
        ctx.rd = rd
        return rd.fx(x) @ rd.fw(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        rd = ctx.rd
        return rd.bdy(dy) @ rd.bw(w), rd.wdy(dy).t() @ rd.wx(x), dy.sum(0), None


def make_linear(variant=None):
    """The ``linear=`` argument of the oracle for the bf16 tower (``variant``: a wrong one)."""
    rd = variant if isinstance(variant, Rounding) else rounding(variant)
    return lambda x, w, b: _BF16Linear.apply(x, w, b, rd)


bf16_linear = make_linear()


# ----------------------------------------------------------------------------- the stages
def lin_fwd(x, W, b, rd):
    return torch.relu(rd.fx(x) @ rd.fw(W).t() + b)


def row_stats(r):
    mu = r.mean(-1)
    var = ((r - mu[:, None]) ** 2).mean(-1)
    return mu, 1.0 / torch.sqrt(var + EPS)


def ln_fwd(r, mu, rs, g, b, mask):
    return ((r - mu[:, None]) * rs[:, None] * g + b) * mask


def head_fwd(a2, mf_pred, P):
    mp = a2 @ P["mlp_output.weight"][0] + P["mlp_output.bias"][0]
    wf = P["final.0.weight"][0]
    return mp, torch.sigmoid(wf[0] * mf_pred + wf[1] * mp + P["final.0.bias"][0])


def head_bwd(prob, targets, P):
    """dL/dz of the mean BCE through the sigmoid, and dL/da_2 (head_bwd: go (1 - o) o)."""
    dz = (prob - targets) / prob.numel()
    return dz, (dz * P["final.0.weight"][0, 1])[:, None] * P["mlp_output.weight"][0][None, :]


def ln_bwd(G, r, mu, rs, g, mask, bound=None):
    """Backward of dropout -> LayerNorm -> ReLU (mlp_tower_dev.h ln_bwd): (dlin, d, h) with d the
    gradient at the LayerNorm's output and h the normalised rows.  ``bound``: an elementwise
    bound on G's error; returns also the bound on dlin's that follows from it."""
    h = (r - mu[:, None]) * rs[:, None]
    pos = (r > 0).to(G.dtype)
    d = G * mask
    gd = d * g

    def through(v, hh):
        return rs[:, None] * (v + v.mean(-1, keepdim=True) + hh * (v * hh).mean(-1, keepdim=True))
    out = pos * rs[:, None] * (gd - gd.mean(-1, keepdim=True) - h * (gd * h).mean(-1, keepdim=True))
    if bound is None:
        return out, d, h
    N = r.shape[1]
    eb = pos * (through(bound * mask * g.abs(), h.abs()) + (N + 16) * U24 * through(gd.abs(), h.abs()))
    return out, d, h, eb


def gemm_bound(A, B, K, bias=None):
    """(K + 8) u (|A| |B|^T + |bias|): see the module's docstring."""
    m = A.abs() @ B.abs().t()
    return (K + 8) * U24 * (m if bias is None else m + bias.abs())


def _names(l):
    return f"mlp.{4 * l}.weight", f"mlp.{4 * l}.bias", f"mlp.{4 * l + 2}.weight", f"mlp.{4 * l + 2}.bias"


def tower_inputs(p, u, i, M, H, attn_mask):
    """What the tower reads of a training step: the attention block's output y [n, D] and the
    GMF prediction [n], from the oracle's own pieces in p's dtype."""
    n = u.numel()
    g, b = p["mlp_norm.weight"], p["mlp_norm.bias"]
    xu = O.layer_norm(p[O.K_MLP_U][u], g, b).view(n // M, M, -1)
    xi = O.layer_norm(p[O.K_MLP_I][i], g, b).view(n // M, M, -1)
    y = O.mha(p, O.ATT, xu, xi, xi, H, attn_mask).reshape(n, -1)
    g, b = p["mf_norm.weight"], p["mf_norm.bias"]
    mf = O.layer_norm(p[O.K_MF_U][u], g, b) * O.layer_norm(p[O.K_MF_I][i], g, b)
    return y, O.linear(mf, p["mf_output.weight"], p["mf_output.bias"]).reshape(-1)


def tower_chain(P, y, mf_pred, masks, targets, D, rd=RNE, layers=(0, 1, 2), dtype=torch.float32):
    """The tower's step evaluated stage after stage in ``dtype``, every stage from the previous
    stage's own result: what the kernels do, with torch's accumulation order in place of the
    MFMA's.  Layers outside ``layers`` round as RNE.  Returns the tensors tower_checks reads."""
    P = {k: v.to(dtype) for k, v in P.items() if v.is_floating_point()}
    y, mf_pred, targets = y.to(dtype), mf_pred.to(dtype).reshape(-1), targets.to(dtype).reshape(-1)
    masks = [m.to(dtype) for m in masks]
    rds = [rd if l in layers else RNE for l in range(3)]
    out = dict(y=y, mf_pred=mf_pred, r=[], a=[], mean=[], rstd=[], dlin=[None] * 3, grads={})
    x = y
    for l in range(3):
        wn, bn, gn, en = _names(l)
        W = P[wn][:, :D] if l == 0 else P[wn]
        r = lin_fwd(x, W, P[bn], rds[l])
        mu, rs = row_stats(r)
        x = ln_fwd(r, mu, rs, P[gn], P[en], masks[l])
        for k, v in zip(("r", "a", "mean", "rstd"), (r, x, mu, rs)):
            out[k].append(v)
    out["mlp_pred"], out["prob"] = head_fwd(x, mf_pred, P)
    dz, G = head_bwd(out["prob"], targets, P)
    out["grads"]["mlp_output.weight"] = (dz * P["final.0.weight"][0, 1] @ x)[None, :]
    out["grads"]["mlp_output.bias"] = (dz * P["final.0.weight"][0, 1]).sum().reshape(1)
    out["grads"]["final.0.weight"] = torch.stack([dz @ mf_pred, dz @ out["mlp_pred"]])[None, :]
    out["grads"]["final.0.bias"] = dz.sum().reshape(1)
    for l in (2, 1, 0):
        wn, bn, gn, en = _names(l)
        dlin, d, h = ln_bwd(G, out["r"][l], out["mean"][l], out["rstd"][l], P[gn], masks[l])
        out["dlin"][l] = dlin
        xin = y if l == 0 else out["a"][l - 1]
        dW = rds[l].wdy(dlin).t() @ rds[l].wx(xin)
        if l == 0:      # (the zero temporal columns of mlp.0 take a zero gradient)
            dW = torch.cat([dW, torch.zeros(dW.shape[0], P[wn].shape[1] - D, dtype=dtype)], 1)
        out["grads"].update({wn: dW, bn: dlin.sum(0), gn: (d * h).sum(0), en: d.sum(0)})
        W = P[wn][:, :D] if l == 0 else P[wn]
        G = rds[l].bdy(dlin) @ rds[l].bw(W)
    out["dy"] = G
    return out


Check = namedtuple("Check", "name layer got want bound kind K")


def tower_checks(T, P, masks, targets, D, wgrad, rd=RNE):
    """The teacher-forced comparisons of one step's tower tensors ``T`` (fp32: y, mf_pred, r, a,
    mean, rstd, dlin, dy, mlp_pred, prob, grads) in float64.  ``wgrad``: "bf16" (the fused weight
    gradients: both operands rounded), "fp32" (wgrad.hip on the stored fp32 dlin and a: nothing
    rounded) or None (no weight gradients in ``T``).  ``rd``: the reference's rounding (RNE;
    anything else only to show that the comparison can tell).  Returns a list of Check; ``layer``
    is the tower layer whose Linear the check involves (None: no Linear in it)."""
    f8 = lambda t: t.double()  # noqa: E731
    P = {k: f8(v) for k, v in P.items() if v.is_floating_point()}
    masks = [f8(m) for m in masks]
    t = f8(targets).reshape(-1)
    n = t.numel()
    y, r, a, dlin = f8(T["y"]), [f8(v) for v in T["r"]], [f8(v) for v in T["a"]], [f8(v) for v in T["dlin"]]
    mean, rstd = [f8(v) for v in T["mean"]], [f8(v) for v in T["rstd"]]
    out = []

    def add(name, layer, got, want, bound, kind, K):
        out.append(Check(name, layer, f8(got).reshape(want.shape), want, bound, kind, K))
    Ws = [P[_names(l)[0]][:, :D] if l == 0 else P[_names(l)[0]] for l in range(3)]
    for l in range(3):
        wn, bn, gn, en = _names(l)
        x = y if l == 0 else a[l - 1]
        K = x.shape[1]
        add(f"r{l}", l, T["r"][l], lin_fwd(x, Ws[l], P[bn], rd),
            gemm_bound(rd.fx(x), rd.fw(Ws[l]), K, P[bn]), "gemm", K)
        mu, rs = row_stats(r[l])
        add(f"mean{l}", None, T["mean"][l], mu, None, "row", 0)
        add(f"rstd{l}", None, T["rstd"][l], rs, None, "row", 0)
        add(f"a{l}", None, T["a"][l], ln_fwd(r[l], mu, rs, P[gn], P[en], masks[l]), None, "row", 0)
    mp, prob = head_fwd(a[2], f8(T["mf_pred"]).reshape(-1), P)
    add("mlp_pred", None, T["mlp_pred"], mp, None, "row", 0)
    add("prob", None, T["prob"], prob, None, "row", 0)
    # backward: the head from the step's own prob and a_2, then layer by layer
    gprob, gmp = f8(T["prob"]).reshape(-1), f8(T["mlp_pred"]).reshape(-1)
    dz, G = head_bwd(gprob, t, P)
    dml = dz * P["final.0.weight"][0, 1]
    g = T["grads"]
    add("mlp_output.weight", None, g["mlp_output.weight"], (dml @ a[2])[None, :], None, "row", 0)
    add("mlp_output.bias", None, g["mlp_output.bias"], dml.sum().reshape(1), None, "row", 0)
    add("final.0.weight", None, g["final.0.weight"],
        torch.stack([dz @ f8(T["mf_pred"]).reshape(-1), dz @ gmp])[None, :], None, "row", 0)
    add("final.0.bias", None, g["final.0.bias"], dz.sum().reshape(1), None, "row", 0)
    Gb = 16 * U24 * G.abs()         # (the head's few fp32 operations per element)
    src = None                      # the layer whose dX Linear produced G
    for l in (2, 1, 0):
        wn, bn, gn, en = _names(l)
        want, d, h, eb = ln_bwd(G, r[l], mean[l], rstd[l], P[gn], masks[l], Gb)
        add(f"dlin{l}", src, T["dlin"][l], want, eb, "row", 0)
        add(bn, None, g[bn], dlin[l].sum(0), (n + 8) * U24 * dlin[l].abs().sum(0), "row", 0)
        db = Gb * masks[l]
        add(gn, src, g[gn], (d * h).sum(0),
            (db * h.abs()).sum(0) + (n + 16) * U24 * (d * h).abs().sum(0), "row", 0)
        add(en, src, g[en], d.sum(0), db.sum(0) + (n + 8) * U24 * d.abs().sum(0), "row", 0)
        if wgrad is not None:
            x = y if l == 0 else a[l - 1]
            wr = rd if wgrad == "bf16" else rd._replace(wdy=_same, wx=_same)
            A, B = wr.wdy(dlin[l]).t(), wr.wx(x).t()
            add(wn, l, g[wn][:, :x.shape[1]], A @ B.t(), gemm_bound(A, B, n), "gemm", n)
            if l == 0:
                add(wn + "[:, D:]", None, g[wn][:, D:], torch.zeros_like(P[wn][:, D:]), None, "row", 0)
        A, B = rd.bdy(dlin[l]), rd.bw(Ws[l]).t()
        G, Gb, src = A @ B.t(), gemm_bound(A, B, Ws[l].shape[0]), l
    add("dy", 0, T["dy"], G, Gb, "gemm", Ws[0].shape[0])
    return out


def fractions(c):
    """(the largest |got - want| as a fraction of the derived bound, of the project's fp32
    tolerance): a correct fp32 step is below 1 on both, the CPU's fp32 evaluation below 1/4."""
    d = (c.got - c.want).abs()
    atol, rtol = ISSUE_TOL[c.kind](c.K)
    issue = float((d / (atol + rtol * c.want.abs())).max())
    if c.bound is None:
        return None, issue
    tight = torch.where(d == 0, torch.zeros_like(d), d / c.bound)
    return float(tight.max()), issue


def failures(checks, limit=1.0):
    """The names of the checks a step does not pass."""
    bad = []
    for c in checks:
        tight, issue = fractions(c)
        if not (issue < limit and (tight is None or tight < limit)):
            bad.append(c.name)
    return bad


def report(checks, tag):
    """One line per check, and the worst fractions (derived bound, project tolerance)."""
    worst = [0.0, 0.0]
    for c in checks:
        tight, issue = fractions(c)
        print(f"{tag} {c.name}: {'-' if tight is None else format(tight, '.3g')} of the derived bound, "
              f"{issue:.3g} of the fp32 tolerance")
        worst = [max(worst[0], tight or 0.0), max(worst[1], issue)]
    print(f"{tag}: worst {worst[0]:.3g} of a derived bound, {worst[1]:.3g} of an fp32 tolerance")
    return worst


# ----------------------------------------------------------------------------- end to end
def e2e_distance(got, want):
    """The distance of a tensor from its reference under the capped exclusion: the smallest
    bound b such that at most 0.1% of the elements are further than b and none further than 8 b
    (scalars and small tensors: the largest difference)."""
    d = (got.double() - want.double()).abs().reshape(-1)
    k = int(1e-3 * d.numel())
    if k == 0:
        return float(d.max())
    top = torch.topk(d, k + 1).values
    return max(float(top[-1]), float(top[0]) / 8)
