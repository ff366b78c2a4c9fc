"""The numpy restatement of the dropout stream (tests/dropout_stream.py) by itself, no GPU: it
matches a scalar transcription of the device functions in plain Python integers, its keep rate
is the threshold's, and the streams that one training step uses together (attention weights,
tower layers, the next step's) are uncorrelated at equal indices.  tests/test_gpu_dropout.py
holds the kernels to this restatement bit for bit.

Bounds, from binomial statistics of N = 2^22 fair draws (not from any measured output):
keep rate within 4 sigma = 4 sqrt(p (1 - p) / N) = 7.8e-4 of 1 - round(p 65536) / 65536;
same-index correlation of two independent streams within 4 / sqrt(N) = 1.95e-3.  With base seed
12345 the restatement gives rates 0.800055 (attention and the three layers: identical, see the
XOR-permutation note in dropout_stream.py) and 0.800035 (next step), correlations 2.5e-4 (attention,
layer 0), 8.0e-4 and 6.2e-4 (consecutive layers), 1e-6 (steps t, t + 1).

Last, the premises of the GPU tests that use the restatement, re-measured here without a GPU:
the fp32 oracle's headroom under each case of tests/test_gpu_dropout.py, and what the check of
ncf_adam_table_bf16 (tests/test_gpu_bf16.py) accepts and rejects."""
import numpy as np
import pytest

from tests import dropout_stream as S

N = 1 << 22
P = 0.2
BASE = 12345


def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _scale_scalar(seed, idx, p):
    """ncf_dropout_scale in Python integers, one element at a time."""
    idx4 = idx >> 2
    k = (seed & 0xFFFFFFFF) ^ _mix32(((seed >> 32) & 0xFFFFFFFF) ^ (idx4 >> 32))
    i = idx4 & 0xFFFFFFFF
    z = (_mix32(i ^ k ^ 0x9E3779B9) << 32) | _mix32(i ^ k)
    u = (z >> (16 * (idx & 3))) & 0xFFFF
    return u >= int(np.float32(p) * np.float32(65536) + np.float32(0.5))


@pytest.mark.parametrize("seed", [0, 12345, 2 ** 62 - 1, (0xDEADBEEF << 32) | 77, 2 ** 63 - 1])
@pytest.mark.parametrize("p", [0.2, 0.25, 0.5])
def test_vector_form_equals_scalar_transcription(seed, p):
    got = S.keep_bits(seed, 4099, p)
    assert got.tolist() == [_scale_scalar(seed, i, p) for i in range(4099)]
    # an index past 2^34: the group index's high word enters the key
    start = (1 << 34) + 5
    got = S.keep_bits(seed, 64, p, start=start)
    assert got.tolist() == [_scale_scalar(seed, start + i, p) for i in range(64)]


def test_thresholds_scales_and_seeds():
    assert [S.drop_threshold(p) for p in (0.2, 0.25, 0.5, 0.0)] == [13107, 16384, 32768, 0]
    s = S.keep_scales(BASE, 1000, 0.2)
    assert s.dtype == np.float32
    assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.2)))}
    assert S.keep_scales(BASE, 1000, 0.0).min() == 1.0          # p = 0 keeps everything
    assert S.layer_seed(2 ** 63 - 1, 0) == 0x9E37 - 1           # wraps at 2^63
    assert S.layer_seed(5, 2) == 5 + 3 * 0x9E37
    assert S.clock_seed(BASE, 0) == BASE
    seeds = [S.clock_seed(BASE, t) for t in range(1, 50)]
    assert len(set(seeds)) == 49 and all(0 <= x < 2 ** 62 for x in seeds)
    m = S.step_masks(BASE, 3, 4, 5, [256, 128, 64], 0.2)
    assert m["attn"].shape == (3, 4, 5, 5) and [x.shape for x in m["mlp"]] == [(15, 256), (15, 128), (15, 64)]
    assert np.array_equal(m["attn"].reshape(-1), S.keep_scales(BASE, 300, 0.2))
    assert np.array_equal(m["mlp"][1].reshape(-1), S.keep_scales(BASE + 2 * 0x9E37, 15 * 128, 0.2))


@pytest.fixture(scope="module")
def streams():
    s1, s2 = S.clock_seed(BASE, 1), S.clock_seed(BASE, 2)
    seeds = {"attn": s1, "l0": S.layer_seed(s1, 0), "l1": S.layer_seed(s1, 1),
             "l2": S.layer_seed(s1, 2), "next": s2}
    return {k: S.keep_bits(v, N, P).astype(np.float64) for k, v in seeds.items()}


def test_keep_rate(streams):
    want = 1 - S.drop_threshold(P) / 65536
    for k, v in streams.items():
        assert abs(v.mean() - want) < 4 * (P * (1 - P) / N) ** 0.5, (k, v.mean())


@pytest.mark.parametrize("a,b", [("attn", "l0"), ("l0", "l1"), ("l1", "l2"), ("attn", "next")])
def test_same_index_correlation(streams, a, b):
    c = np.corrcoef(streams[a], streams[b])[0, 1]
    assert abs(c) < 4 / N ** 0.5, (a, b, c)


# ----------------------------------------------------------------------------- the GPU cases' premises
def _headroom_cases():
    from tests import test_gpu_dropout as TD
    # (the bf16-tower cases have premises of their own: tests/test_bf16_tower.py)
    return [k for k, c in TD.CASES.items() if c.get("tower") != "bf16"]


@pytest.mark.parametrize("name", _headroom_cases())
def test_oracle_headroom_of_gpu_case(name):
    """The premises of tests/test_gpu_dropout.py's cases, re-measured without a GPU: with the
    seeds the case will draw and its masks, the fp32 oracle stays within a quarter of each
    tolerance of the float64 oracle (prob / loss 5e-6, gradients rtol 2e-4 / atol 2e-6), the
    masks drop about p, and no float64 tower pre-activation is nearer to 0 than 4 x the recorded
    fp32-vs-float64 pre-activation difference."""
    import torch
    from tests import test_gpu_dropout as TD
    c = TD.CASES[name]
    D, H, M, B, p, steps = (c[k] for k in ("D", "H", "M", "B", "p", "steps"))
    seeds = TD.case_seeds(name, steps)
    geo = TD.geo(c)
    hid, tdim = geo["hid"], geo["tdim"]
    init = {k: v.detach().clone() for k, v in TD.make_model(D, H, M, p, **geo).state_dict().items()}
    if c.get("table_dtype") == "bf16":
        init = TD.bf16_tables(init)
    batches = TD.make_batches(B, M, steps, c["data_seed"])
    r64, _ = TD.oracle_run(init, batches, seeds, H, M, p, torch.float64, hid=hid, tdim=tdim)
    r32, _ = TD.oracle_run(init, batches, seeds, H, M, p, torch.float32, hid=hid, tdim=tdim)
    for seed, a, b in zip(seeds, r64, r32):
        if p > 0:
            m = S.step_masks(seed, B, H, M, hid, p)
            for x in [m["attn"]] + m["mlp"]:
                assert abs(float((x > 0).mean()) - (1 - p)) < 4 * (p * (1 - p) / x.size) ** 0.5
        assert (a["prob"] - b["prob"].double()).abs().max().item() < 5e-6 / 4
        assert abs(float(a["loss"]) - float(b["loss"])) < 5e-6 / 4
        for k, v in a["grads"].items():
            frac = ((v - b["grads"][k].double()).abs() / (2e-6 + 2e-4 * v.abs())).max().item()
            assert frac < 0.25, (k, frac)
        assert min(float(z.abs().min()) for z in a["pre"]) > 4 * c["pre"]


@pytest.mark.parametrize("D", [64, 128])
def test_adam_bf16_check_premises(D):
    """tests/test_gpu_bf16.py's check of ncf_adam_table_bf16, without a GPU: the fp32 CPU Adam
    rounded to bf16 passes it on the chosen inputs; the same update stored by truncation, or
    with a first moment 3e-6 off, does not."""
    import torch
    from tests import test_gpu_bf16 as TB
    TB.check_adam_bf16(D, TB.cpu_adam_apply)

    def truncating(p, m, v, slot, G, grad, t):
        p32, m32, v32 = TB._adam_ref(p, m, v, grad, t, torch.float32)
        return (p32.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16), m32, v32

    def moment_off(p, m, v, slot, G, grad, t):
        p16, m32, v32 = TB.cpu_adam_apply(p, m, v, slot, G, grad, t)
        return p16, m32 * (1 + 3e-6), v32
    for bad in (truncating, moment_off):
        with pytest.raises(AssertionError):
            TB.check_adam_bf16(D, bad)
