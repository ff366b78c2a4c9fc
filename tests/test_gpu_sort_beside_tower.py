"""The id sort sized to sit beside a tower workgroup (k_onesweep's LDS by the pass's radix, 16-bit
in-tile counts) and the stage-2 reduction with every load in flight: neither may change a bit.
Runs on a real MI355X only (marker ``gpu``)."""
import ctypes

import numpy as np
import pytest
import torch

import _ncf_pkg

pytestmark = pytest.mark.gpu
ncf = _ncf_pkg.load()
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------ dedup, widest digit
@pytest.mark.parametrize("n0,n1", [(5000, 1025), (66000, 3000)])
def test_dedup_widest_digit_many_tiles(n0, n1):
    """The radix form at 2^22 rows: two passes of the widest digit (11 bits), where k_onesweep's
    LDS is largest and its per-wave / per-tile digit counts live in 16 bits.  (5000, 1025): a
    few tiles, predecessors summed directly, a ragged last tile and a tile of one key;
    (66000, 3000): 65 tiles, the chained look-back.  Ids: half Zipf-hot (one digit value holding
    most of a tile: counts near the 1024-key tile size), half uniform over all 2^22 rows (every
    digit value of both passes), and every 7th the last row.  Against np.unique."""
    from ncf_amd import _lib
    rows = 1 << 22
    rng = np.random.default_rng(n0 * 31 + n1)
    ids = []
    for n in (n0, n1):
        x = (rng.zipf(1.2, n) - 1) % rows
        uni = rng.integers(0, rows, n)
        x = np.where(rng.random(n) < 0.5, x, uni)
        x[::7] = rows - 1
        ids.append(torch.from_numpy(x.astype(np.int64)))
    n, D = max(n0, n1), 64
    prev = _lib.query("ncf_dedup_set_small_max", 0)
    try:
        ws = torch.empty(_lib.query("ncf_embedding_bwd_workspace", n, D), dtype=torch.uint8,
                         device=DEV)
        uq = [torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
        slot = [torch.full((rows,), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
        inv = [torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
        nu = torch.full((2,), 99, dtype=torch.int32, device=DEV)
        dv = [t.to(DEV) for t in ids]
        st = _lib.stream_ptr(DEV)
        _lib.call("ncf_dedup_ids2", dv[0].data_ptr(), n0, rows, dv[1].data_ptr(), n1, rows, D,
                  uq[0].data_ptr(), uq[1].data_ptr(), slot[0].data_ptr(), slot[1].data_ptr(),
                  nu.data_ptr(), ws.data_ptr(), ws.numel(), st)
        _lib.call("ncf_dedup_inverse", n0, n1, rows, rows, D, inv[0].data_ptr(),
                  inv[1].data_ptr(), ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
    finally:
        _lib.query("ncf_dedup_set_small_max", prev)
    for k, (x, nk) in enumerate(zip(ids, (n0, n1))):
        u, iv = np.unique(x.numpy(), return_inverse=True)
        assert int(nu[k]) == len(u)
        np.testing.assert_array_equal(uq[k][:len(u)].cpu().numpy(), u)
        np.testing.assert_array_equal(inv[k][:nk].cpu().numpy(), iv.reshape(-1))
        s = slot[k].cpu().numpy()
        np.testing.assert_array_equal(s[u], np.arange(len(u)))
        assert (s == -1).sum() == rows - len(u)


# ------------------------------------------------------------------ stage-2 reduce, by order
def _ordered_sum(x):
    """float32 sum of the rows of x [m, L] in the order of k_reduce_parts (ncf_common.h) and of
    both stages of ncf_reduce_batch: "wave" w takes rows w, w + 4, ...; while four more of its
    rows remain (p + 12 < m) they go one each into accumulators 0..3 (row index j in the wave's
    sequence into accumulator j mod 4); its last, at most three, rows all go into accumulator
    0; then (a0 + a1) + (a2 + a3) per wave and (w0 + w1) + (w2 + w3)."""
    m, L = x.shape
    ws = []
    for w in range(4):
        a = [np.zeros(L, np.float32) for _ in range(4)]
        p = w
        while p + 12 < m:
            for k in range(4):
                a[k] = a[k] + x[p + 4 * k]
            p += 16
        while p < m:
            a[0] = a[0] + x[p]
            p += 4
        ws.append((a[0] + a[1]) + (a[2] + a[3]))
    return (ws[0] + ws[1]) + (ws[2] + ws[3])


def _two_stage(part, P, L):
    """ncf_reduce_batch's documented order for P > 256 partial rows: chunks of 64 rows summed
    each by _ordered_sum (stage 1), then the chunk rows the same way (stage 2)."""
    chunks = [_ordered_sum(part[c:min(P, c + 64), :L]) for c in range(0, P, 64)]
    return _ordered_sum(np.stack(chunks))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("P", [257, 1537, 4200])
def test_reduce_batch_two_stage_bits_follow_the_order(P, accumulate):
    """Multi-chunk descriptors (P > 256: 5, 25 — the C2 step's 2 * 768 + 1 — and 66 chunk rows,
    the last more than one stage-2 batch of 64) of L = 4 and 256 (four columns per lane), 7
    (one per lane) and 4 again behind the 7 (its scratch rows then start off a 16-byte
    boundary: one column per lane), partial rows strided wider than L, scale 0.5 (exact in
    binary, so a fused multiply-add in the store cannot differ).  Bit-equal to the numpy
    float32 restatement of the order above — which the library before stage 2 issued its loads
    ahead of its adds matches bit for bit as well (checked once against that build)."""
    from ncf_amd import _lib
    rng = np.random.default_rng(P)
    Ls = [4, 256, 7, 4]
    lst = _lib.ReduceList()
    keep, want, outs = [], [], []
    for j, L in enumerate(Ls):
        stride = L + 8 if L % 4 == 0 else L + 3
        part = rng.standard_normal((P, stride)).astype(np.float32)
        prev = rng.standard_normal(L).astype(np.float32)
        dp, do = torch.from_numpy(part).to(DEV), torch.from_numpy(prev).to(DEV)
        keep.append(dp)
        outs.append(do)
        d = lst.d[j]
        d.part, d.out, d.stride, d.ldo = dp.data_ptr(), do.data_ptr(), stride, L
        d.L, d.cols, d.P, d.accumulate, d.scale, d.reserved = L, L, P, accumulate, 0.5, 0
        v = np.float32(0.5) * _two_stage(part, P, L)
        want.append(prev + v if accumulate else v)
    lst.count = len(Ls)
    addr = ctypes.addressof(lst)
    need = _lib.query("ncf_reduce_batch_scratch", addr)
    assert need == sum(-(-P // 64) * L for L in Ls)
    scratch = torch.empty(need, dtype=torch.float32, device=DEV)
    _lib.call("ncf_reduce_batch", addr, scratch.data_ptr(), scratch.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    for L, o, wv in zip(Ls, outs, want):
        got, wv = o.cpu().numpy(), wv.astype(np.float32)
        assert got.view(np.uint32).tolist() == wv.view(np.uint32).tolist(), (P, L)
