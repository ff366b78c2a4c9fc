"""MultiHeadAttention with a key/value length that differs from the query length, on the MI355X:
attention_x.hip (ncf_attention_x_fwd / _x_bwd) through ncf.MultiHeadAttention and at the C-ABI.

Against F10 (the reference's own module, tests/golden/make_golden_xattn.py), against the float64
oracle with the restated dropout stream, and against the equal-length core (attention.hip) where
both apply.  Tolerances are F4's (test_gpu_parity.test_f4_mha): y atol 2e-5 / rtol 1e-5, input
gradients atol 2e-5 / rtol 1e-4, weight gradients atol 5e-5 / rtol 1e-4.  tests/test_xattn_golden.py
holds the oracle to F10 on the CPU (float64 within 3.1e-7 on y, 5.6e-7 on the input gradients and
5.4e-6 on weight gradients of magnitude up to 27)."""
import numpy as np
import pytest
import torch

import _ncf_pkg
from oracle import ncf_oracle as O
from tests import dropout_stream as S
from tests import xattn_cases as X
from tests.conftest import load_npz, sub

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
from ncf_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = -777.25
TAIL = 64


def module_for(c, p=0.0):
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    mod = ncf.MultiHeadAttention(D, H, dropout=p)
    mod.load_state_dict(X.T(sub(c, "w/")))
    return mod.to(DEV)


def dev_mask(c):
    return torch.from_numpy(c["mask"]).to(DEV) if "mask" in c else None


def host_seed(k):
    """The seed the next training-mode call draws (torch.randint(0, 2**62, (1,)) on the default
    generator): seed the generator, draw once, seed it again, so that the call draws the same."""
    torch.manual_seed(k)
    s = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(k)
    return s


# ----------------------------------------------------------------------------- 1. F10 parity
@pytest.mark.parametrize("tag", X.ALL)
def test_f10_mha(tag):
    c = X.case(tag)
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    mod = module_for(c)
    q, k, v = [torch.from_numpy(c[n]).to(DEV).requires_grad_(True) for n in "qkv"]
    y = mod(q, k, v, mask=dev_mask(c))
    assert tuple(y.shape) == (Bn, Lq, D)
    np.testing.assert_allclose(y.detach().cpu().numpy(), c["y"], atol=2e-5, rtol=1e-5)
    y.backward(torch.from_numpy(c["gy"]).to(DEV))
    for n, t in zip("qkv", (q, k, v)):
        assert t.grad.shape == t.shape
        np.testing.assert_allclose(t.grad.cpu().numpy(), c[f"g{n}"], atol=2e-5, rtol=1e-4)
    for n, p in mod.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), c[f"gw/{n}"], atol=5e-5, rtol=1e-4,
                                   err_msg=n)


# ----------------------------------------------------------------------------- 2. training mode
@pytest.mark.parametrize("tag", ["x1_50", "x1_50@padding", "x3_7", "x3_7@padding", "x7_64_h1",
                                 "x7_64_h1@padding"])
def test_train_mode_vs_float64_oracle(tag):
    """dropout 0.3 in training mode: y, dq, dk, dv and every weight gradient against O.mha in
    float64 with the keep-scales of the seed the call drew, restated on the host with the element
    index ((b*H + h)*L_q + i)*L_k + j.  Two calls draw fresh masks; eval ignores dropout."""
    p = 0.3
    c = X.case(tag)
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    w = X.T(sub(c, "w/"))
    mod = module_for(c, p).train()
    mask = torch.from_numpy(c["mask"]) if "mask" in c else None
    margs = dict(mask=dev_mask(c))
    qkv = [torch.from_numpy(c[n]) for n in "qkv"]
    gy = torch.from_numpy(c["gy"])
    xs = [t.to(DEV).requires_grad_(True) for t in qkv]
    seed = host_seed(77)
    y = mod(*xs, **margs)
    y.backward(gy.to(DEV))
    keep = S.keep_scales(seed, Bn * H * Lq * Lk, p).reshape(Bn, H, Lq, Lk)
    frac = float((keep > 0).mean())
    assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / keep.size) ** 0.5, frac
    ps = {f"a.{k}": v.double().requires_grad_(True) for k, v in w.items()}
    rs = [t.double().requires_grad_(True) for t in qkv]
    ry = O.mha(ps, "a.", *rs, H, drop_mask=torch.from_numpy(keep).double(), mask=mask)
    ry.backward(gy.double())
    print(f"xattn {tag}: |dy| {(y.detach().cpu().double() - ry.detach()).abs().max().item():.3g}")
    torch.testing.assert_close(y.detach().cpu().double(), ry.detach(), atol=2e-5, rtol=1e-5)
    for a_, b_ in zip(xs, rs):
        torch.testing.assert_close(a_.grad.cpu().double(), b_.grad, atol=2e-5, rtol=1e-4)
    for n, q in mod.named_parameters():
        torch.testing.assert_close(q.grad.cpu().double(), ps[f"a.{n}"].grad, atol=5e-5, rtol=1e-4)
    with torch.no_grad():
        dps = {k: v.detach() for k, v in ps.items()}
        drs = [t.detach() for t in rs]
        # the masks of another seed: far outside the tolerance
        other = O.mha(dps, "a.", *drs, H, mask=mask, drop_mask=torch.from_numpy(
            S.keep_scales(seed + 1, Bn * H * Lq * Lk, p).reshape(Bn, H, Lq, Lk)).double())
        assert (y.detach().cpu().double() - other).abs().max().item() > 1e-3
        # fresh masks per call; eval ignores dropout and is repeatable
        y2, y3 = mod(*xs, **margs), mod(*xs, **margs)
        assert not torch.equal(y2, y3)
        mod.eval()
        e1, e2 = mod(*xs, **margs), mod(*xs, **margs)
        assert torch.equal(e1, e2)
        plain = O.mha(dps, "a.", *drs, H, mask=mask)
        torch.testing.assert_close(e1.cpu().double(), plain, atol=2e-5, rtol=1e-5)


# ----------------------------------------------------------------------------- C-ABI helpers
def x_fwd(q, k, v, Bn, Lq, Lk, H, D, p, seed, mask, P, o):
    _lib.call("ncf_attention_x_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), Bn, Lq, Lk, H, D, p,
              seed, None, None if mask is None else mask.data_ptr(), P.data_ptr(), o.data_ptr(),
              _lib.stream_ptr(DEV))


def x_bwd(q, k, v, P, do, Bn, Lq, Lk, H, D, p, seed, dq, dk, dv):
    _lib.call("ncf_attention_x_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), P.data_ptr(),
              do.data_ptr(), Bn, Lq, Lk, H, D, p, seed, None, dq.data_ptr(), dk.data_ptr(),
              dv.data_ptr(), _lib.stream_ptr(DEV))


def projected(c):
    """q, k, v and dO rows of a case ([B*L, D] each), projected with torch on the device."""
    w = {k: v.to(DEV) for k, v in X.T(sub(c, "w/")).items()}
    D = c["q"].shape[-1]
    x = {n: torch.from_numpy(c[n]).to(DEV).reshape(-1, D) for n in ("q", "k", "v", "gy")}
    q, k, v = (x[n] @ w[f"{n}_proj.weight"].T + w[f"{n}_proj.bias"] for n in "qkv")
    return q.contiguous(), k.contiguous(), v.contiguous(), (x["gy"] @ w["out_proj.weight"]).contiguous()


# ----------------------------------------------------------------------------- 3. equal lengths
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("tag", ["mha5", "mha50"])
def test_equal_lengths_match_the_equal_length_core(tag, p):
    """len_q == len_k through ncf_attention_x_fwd / _x_bwd against ncf_attention_fwd / _bwd on the
    F4 inputs: same P, O, dQ, dK, dV; with dropout on the same seed both read the same stream."""
    f4 = load_npz("f4_ops.npz")
    c = sub(f4, f"{tag}/")
    Bn, L, D, H = [int(x) for x in c["shape"]]
    q, k, v, do = projected(c)
    seed = 0x1234ABCD9E3779B9 % 2 ** 62
    st = _lib.stream_ptr(DEV)
    new = lambda *s: torch.full(s, SENTINEL, device=DEV)   # noqa: E731
    Pa, Pb = new(Bn * H * L * L), new(Bn * H * L * L)
    oa, ob, dqa, dqb, dka, dkb, dva, dvb = (new(Bn * L, D) for _ in range(8))
    dS = new(Bn * H * L * L)
    _lib.call("ncf_attention_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), Bn, L, H, D, p, seed,
              None, Pa.data_ptr(), oa.data_ptr(), st)
    _lib.call("ncf_attention_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), Pa.data_ptr(),
              do.data_ptr(), Bn, L, H, D, p, seed, None, dS.data_ptr(), dqa.data_ptr(),
              dka.data_ptr(), dva.data_ptr(), st)
    x_fwd(q, k, v, Bn, L, L, H, D, p, seed, None, Pb, ob)
    x_bwd(q, k, v, Pb, do, Bn, L, L, H, D, p, seed, dqb, dkb, dvb)
    for n, a, b in (("P", Pa, Pb), ("O", oa, ob), ("dQ", dqa, dqb), ("dK", dka, dkb),
                    ("dV", dva, dvb)):
        torch.testing.assert_close(b, a, atol=2e-5, rtol=1e-4, msg=lambda m, n=n: f"{n}: {m}")
    if p > 0:   # the dropout changed the output: the comparison above did see the masks
        oc = new(Bn * L, D)
        x_fwd(q, k, v, Bn, L, L, H, D, 0.0, 0, None, Pb, oc)
        assert (oc - ob).abs().max().item() > 1e-3


# ----------------------------------------------------------------------------- 4. no stray writes
def placed(t, where):
    """A copy of ``t`` at the very end of its own allocation ("end": behind 61 elements, so the
    pointer is not 16-byte aligned either) or in the middle of a larger one ("mid")."""
    n = t.numel()
    buf = torch.zeros(61 + n if where == "end" else 4 * n + 256, dtype=t.dtype, device=DEV)
    view = buf[61:] if where == "end" else buf[n + 128:2 * n + 128]
    view.copy_(t.reshape(-1))
    return view.view(t.shape)


@pytest.mark.parametrize("tag", ["x3_7", "x7_64_h1", "x3_7@per_head", "x7_64_h1@per_head"])
def test_no_stray_writes_and_placement(tag):
    c = X.case(tag)
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    src = projected(c)
    m8 = None
    if "mask" in c:
        m8 = torch.broadcast_to(torch.from_numpy(c["mask"]) != 0, (Bn, H, Lq, Lk)).to(torch.uint8)
        m8 = m8.contiguous().to(DEV)
    sizes = {"P": Bn * H * Lq * Lk, "o": Bn * Lq * D, "dq": Bn * Lq * D, "dk": Bn * Lk * D,
             "dv": Bn * Lk * D}
    res = {}
    for where in ("end", "mid"):
        q, k, v, do = (placed(t, where) for t in src)
        mask = None if m8 is None else placed(m8, where)
        out = {n: torch.full((s + TAIL,), SENTINEL, device=DEV) for n, s in sizes.items()}
        for p, seed in ((0.0, 0), (0.3, 12345)):
            x_fwd(q, k, v, Bn, Lq, Lk, H, D, p, seed, mask, out["P"], out["o"])
            x_bwd(q, k, v, out["P"], do, Bn, Lq, Lk, H, D, p, seed, out["dq"], out["dk"], out["dv"])
            for n, s in sizes.items():
                assert (out[n][s:] == SENTINEL).all(), (n, where, p)      # the tail: untouched
                assert (out[n][:s] != SENTINEL).all(), (n, where, p)      # every element written
            res[where, p] = {n: out[n][:sizes[n]].clone() for n in sizes}
        # the inputs came back unchanged
        for a, b in zip((q, k, v, do), src):
            assert torch.equal(a, b)
    for p in (0.0, 0.3):
        for n in sizes:
            assert torch.equal(res["end", p][n], res["mid", p][n]), (n, p)


# ----------------------------------------------------------------------------- 5. fully masked row
def test_fully_masked_row_is_nan_like_the_oracle():
    c = X.case("x3_7@per_head")
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    mod = module_for(c)
    mask = torch.from_numpy(c["mask"]).clone()
    mask[0, 0, 0, :] = 0
    qkv = [torch.from_numpy(c[n]) for n in "qkv"]
    with torch.no_grad():
        y = mod(*[t.to(DEV) for t in qkv], mask=mask.to(DEV)).cpu()
        r = O.mha(X.T(sub(c, "w/")), "", *qkv, H, mask=mask)
    assert torch.isnan(y[0]).any() and not torch.isnan(y[1:]).any()
    assert torch.equal(torch.isnan(y), torch.isnan(r))
    torch.testing.assert_close(y[1:], r[1:], atol=2e-5, rtol=1e-5)
    # the rows of group 0 that no NaN reaches
    torch.testing.assert_close(y, r, atol=2e-5, rtol=1e-5, equal_nan=True)


# ----------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_bitwise_reproducible(p):
    c = X.case("x64_33")
    mod = module_for(c, p).train()
    runs = []
    for _ in range(2):
        mod.zero_grad()
        xs = [torch.from_numpy(c[n]).to(DEV).requires_grad_(True) for n in "qkv"]
        host_seed(5)
        y = mod(*xs)
        y.backward(torch.from_numpy(c["gy"]).to(DEV))
        runs.append([y.detach().clone()] + [t.grad.clone() for t in xs] +
                    [q.grad.clone() for q in mod.parameters()])
    assert len(runs[0]) == 12
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_core_bitwise_reproducible_at_the_c_abi():
    c = X.case("x64_33")
    Bn, Lq, Lk, D, H = [int(x) for x in c["shape"]]
    q, k, v, do = projected(c)
    runs = []
    for _ in range(2):
        P = torch.empty(Bn * H * Lq * Lk, device=DEV)
        o, dq = torch.empty(Bn * Lq, D, device=DEV), torch.empty(Bn * Lq, D, device=DEV)
        dk, dv = torch.empty(Bn * Lk, D, device=DEV), torch.empty(Bn * Lk, D, device=DEV)
        x_fwd(q, k, v, Bn, Lq, Lk, H, D, 0.3, 99, None, P, o)
        x_bwd(q, k, v, P, do, Bn, Lq, Lk, H, D, 0.3, 99, dq, dk, dv)
        runs.append((P, o, dq, dk, dv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("Lq,Lk,H,D", [(3, 65, 4, 64), (65, 3, 4, 64), (0, 3, 4, 64), (3, 0, 4, 64),
                                       (3, 7, 4, 16)])
def test_c_abi_refuses_without_a_launch(Lq, Lk, H, D):
    """len_q or len_k outside 1..64 and head dim 4 (as the equal-length entries refuse it): an
    error status (NCF_ERR_ARG), raised as NCFLibraryError, and no buffer is touched."""
    Bn = 2
    bufs = [torch.full((Bn * H * 65 * 65,), SENTINEL, device=DEV) for _ in range(9)]
    q, k, v, P, o, do, dq, dk, dv = bufs
    with pytest.raises(_lib.NCFLibraryError, match="ncf_attention_x_fwd"):
        x_fwd(q, k, v, Bn, Lq, Lk, H, D, 0.0, 0, None, P, o)
    with pytest.raises(_lib.NCFLibraryError, match="ncf_attention_x_bwd"):
        x_bwd(q, k, v, P, do, Bn, Lq, Lk, H, D, 0.0, 0, dq, dk, dv)
    torch.cuda.synchronize()
    for b in bufs:
        assert (b == SENTINEL).all()


def test_degenerate_and_host_refusals():
    # groups = 0: OK, nothing to launch (no buffer needed)
    st = _lib.stream_ptr(DEV)
    assert _lib.call("ncf_attention_x_fwd", None, None, None, 0, 1, 50, 4, 64, 0.0, 0, None, None,
                     None, None, st) == 0
    assert _lib.call("ncf_attention_x_bwd", None, None, None, None, None, 0, 1, 50, 4, 64, 0.0, 0,
                     None, None, None, None, st) == 0
    mod = ncf.MultiHeadAttention(64, 4, dropout=0.0).to(DEV)
    q = torch.randn(3, 2, 64, device=DEV)
    with pytest.raises(RuntimeError, match="value length"):      # as the reference's matmul
        mod(q, torch.randn(3, 9, 64, device=DEV), torch.randn(3, 8, 64, device=DEV))
    with pytest.raises(ValueError, match="batch"):
        mod(q, torch.randn(4, 9, 64, device=DEV), torch.randn(4, 9, 64, device=DEV))
    with pytest.raises(ValueError, match="embedding"):
        mod(q, torch.randn(3, 9, 32, device=DEV), torch.randn(3, 9, 32, device=DEV))
    with pytest.raises(ValueError):                               # L_k = 65: the library's refusal
        mod(q, torch.randn(3, 65, 64, device=DEV), torch.randn(3, 65, 64, device=DEV))
    # a 2-D key/value pair under a 3-D query is one key per group: softmax over one score
    y = mod(q, torch.randn(3, 64, device=DEV), torch.randn(3, 64, device=DEV))
    assert tuple(y.shape) == (3, 2, 64) and torch.isfinite(y).all()


# ----------------------------------------------------------------------------- 8. module level
def test_sequence_attention_gradient_flow():
    """AdvancedNCF.sequence_attention (architecture.py:210-214) called the way it is meant to be:
    one user row over a 50-long item history."""
    torch.manual_seed(4)
    B, D = 6, 64
    model = ncf.AdvancedNCF(40, 30, 5, 24, D, D, 32, [256, 128, 64], 4, 0.0, 4).to(DEV)
    user_row = torch.randn(B, D, device=DEV, requires_grad=True)
    history = torch.randn(B, 50, D, device=DEV, requires_grad=True)
    y = model.sequence_attention(user_row, history, history)
    assert tuple(y.shape) == (B, 1, D)
    y.square().sum().backward()
    for t in (user_row, history):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0
    seen = set()
    for n, p in model.named_parameters():
        if n.startswith("sequence_attention."):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            assert p.grad.abs().sum().item() > 0, n
            seen.add(n)
        else:
            assert p.grad is None or not p.grad.any(), n
    assert len(seen) == 8
