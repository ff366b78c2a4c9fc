"""tests/sr_stream.py (the stochastic rounding of the bf16 tables restated in numpy) held to a
scalar transcription and to the statistics the contract promises, and the premises of
tests/test_gpu_bf16_sr.py re-measured without a GPU: its check functions run here on the CPU
stand-in (the fp32 CPU Adam with the restated store in the kernel's place), where they must
pass, and with nearest-even in the store's place, where they must fail."""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import sr_stream as SR

N = 1 << 22
SEED = 0x5EED1234


def test_header_declares_the_dtype_and_the_seed_field():
    import ctypes

    import _ncf_pkg
    _ncf_pkg.load()
    from ncf_amd import _lib
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_BF16_SR) == (0, 1, 2)
    assert ctypes.sizeof(_lib.TablePair) == 96
    assert (_lib.TablePair.param_dtype.offset, _lib.TablePair.param_dtype.size) == (88, 4)
    assert (_lib.TablePair.round_seed.offset, _lib.TablePair.round_seed.size) == (92, 4)
    pr = _lib.TablePair()
    pr.param_dtype, pr.round_seed = 2, SEED - (1 << 32) * (SEED >> 31)
    assert pr.round_seed & 0xFFFFFFFF == SEED


def test_vector_form_is_the_scalar_transcription():
    rng = np.random.default_rng(1)
    e = np.concatenate([np.arange(40, dtype=np.uint64),
                        rng.integers(0, 1 << 33, 200).astype(np.uint64),
                        np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + 1, 6_400_000_000 - 1,
                                  (1 << 40) + 5], dtype=np.uint64)])
    for seed in (0, 1, SEED, 0xFFFFFFFF):
        for kind in (0, 1):
            for step in (1, 2, 140, 65536, (1 << 30) - 1):
                w = SR.word(seed, kind, step, e)
                assert [int(x) for x in w] == [SR.word_scalar(seed, kind, step, int(x)) for x in e]
                for j in (0, 1):
                    r = SR.bits(seed, kind, j, step, e)
                    assert [int(x) for x in r] == [(int(y) >> (16 * j)) & 0xFFFF for y in w]
    x = np.concatenate([rng.standard_normal(300).astype(np.float32) * np.float32(0.1),
                        np.array([0.0, -0.0, 1.0, 1e3, 2.0 ** -120, 2.0 ** -130, 3.3e38, -3.4e38,
                                  np.inf, -np.inf, np.nan], dtype=np.float32)])
    r = rng.integers(0, 65536, x.size).astype(np.uint64)
    assert [int(h) for h in SR.store(x, r)] == [SR.store_scalar(a, int(b)) for a, b in zip(x, r)]


def test_store_keeps_what_bf16_holds_and_rounds_up_with_probability_low16():
    rng = np.random.default_rng(2)
    exact = SR.widen(rng.integers(0, 0x7F80, 500).astype(np.uint16))      # finite, sign +
    exact = np.concatenate([exact, -exact, np.array([np.inf, -np.inf], np.float32)])
    for r in (0, 1, 0x8000, 0xFFFF):
        assert np.array_equal(SR.store(exact, np.full(exact.size, r, np.uint64)),
                              exact.view(np.uint32) >> 16)
    nan = np.array([np.nan, -np.nan], np.float32)
    got = SR.widen(SR.store(nan, np.full(2, 0xFFFF, np.uint64)))
    assert np.isnan(got).all() and np.array_equal(np.signbit(got), np.signbit(nan))
    all_r = np.arange(65536, dtype=np.uint64)
    for x in (np.float32(1.0 - 2.0 ** -12), np.float32(-0.3137), np.float32(1e3 - 1e-3),
              np.float32(2.0 ** -130 * 1.3), np.float32(0.1)):
        low = int(x.view(np.uint32)) & 0xFFFF
        trunc = int(x.view(np.uint32)) >> 16
        h = SR.store(np.full(65536, x, np.float32), all_r).astype(np.int64)
        assert set(np.unique(h)) <= {trunc, trunc + 1}
        assert int((h == trunc + 1).sum()) == low       # over all 65536 r: exactly low16 go up
        # ... so the expectation of the stored value is x
        mean = SR.widen(h.astype(np.uint16)).astype(np.float64).mean()
        assert mean == pytest.approx(float(x), rel=0, abs=abs(float(x)) * 2.0 ** -40)
    # the largest finite magnitudes may reach inf, as under nearest even
    assert SR.store(np.array([3.4e38], np.float32), np.array([0xFFFF], np.uint64))[0] == 0x7F80


def _u(seed, kind, j, step, e0=0):
    e = np.arange(N, dtype=np.uint64) + np.uint64(e0)
    return SR.bits(seed, kind, j, step, e).astype(np.float64)


def test_values_are_uniform():
    """N = 2^22 elements, 4 sigma: the mean (sigma = 65536 / sqrt(12 N)), every bit's frequency
    (sigma = 1 / (2 sqrt(N))) and a chi-square over the 256 values of the top byte (255 degrees
    of freedom, sigma = sqrt(510))."""
    for kind, j, step, e0 in ((0, 0, 1, 0), (0, 1, 1, 0), (1, 0, 7, 0), (1, 1, 140, 1 << 32)):
        r = _u(SEED, kind, j, step, e0)
        assert abs(r.mean() - 32767.5) < 4 * 65536 / (12 * N) ** 0.5, (kind, j)
        ri = r.astype(np.int64)
        for b in range(16):
            assert abs(float(((ri >> b) & 1).mean()) - 0.5) < 4 * 0.5 / N ** 0.5, (kind, j, b)
        counts = np.bincount(ri >> 8, minlength=256)
        chi2 = float(((counts - N / 256) ** 2 / (N / 256)).sum())
        assert abs(chi2 - 255) < 4 * 510 ** 0.5, (kind, j, chi2)


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_no_same_element_correlation():
    """Between consecutive steps, between the two tables of a pair, between the two kinds and
    between two seeds: the correlation of the 16-bit values of the same N = 2^22 elements, and
    of their top bits (the rounding decisions of a value half-way), within 4 / sqrt(N)."""
    base = _u(SEED, 0, 0, 5)
    others = {"next step": _u(SEED, 0, 0, 6), "two steps on": _u(SEED, 0, 0, 7),
              "other table": _u(SEED, 0, 1, 5), "other kind": _u(SEED, 1, 0, 5),
              "other kind, other table": _u(SEED, 1, 1, 5), "other seed": _u(SEED + 1, 0, 0, 5),
              "next 2^32 elements": _u(SEED, 0, 0, 5, 1 << 32)}
    for name, o in others.items():
        assert not np.array_equal(o, base), name
        assert abs(_corr(base, o)) < 4 / N ** 0.5, (name, _corr(base, o))
        assert abs(_corr(base >= 32768, o >= 32768)) < 4 / N ** 0.5, name
    # the two tables at consecutive steps (the halves of two words)
    assert abs(_corr(_u(SEED, 0, 1, 5), others["next step"])) < 4 / N ** 0.5


# ------------------------------------------------------------------ premises of the GPU cases
def _standin(rd=None):
    """check_adam_sr's ``apply`` on the CPU: torch's fp32 Adam (test_gpu_bf16._adam_ref, the
    stand-in its nearest-even case was chosen with), stored through the restated bits."""
    from tests import test_gpu_bf16 as TB

    def apply(kind, j, p0, m0, v0, grad, has, t):
        p32, m32, v32 = TB._adam_ref(p0, m0, v0, grad, t, torch.float32)
        x = p32.numpy()
        out = rd(x) if rd is not None else SR.sr_round(x, SEED, kind, j, t)
        return torch.from_numpy(out).to(torch.bfloat16), m32, v32
    return apply


@pytest.mark.parametrize("D", [64, 128])
def test_premise_one_step_case_holds_for_the_fp32_cpu_adam(D):
    from tests import test_gpu_bf16_sr as G
    report = []
    G.check_adam_sr(D, _standin(), SEED, report)
    worst_nd = max(r[3] for r in report)
    far = max(r[4] for r in report)
    signed = max(abs(r[5]) for r in report)
    print(f"D={D}: at most {worst_nd} elements of {1000 * D} differ, {far:.3g} steps from the "
          f"threshold at the most; |mean signed error| <= {signed:.3g}")
    assert worst_nd <= 1e-3 * 1000 * D
    # nearest even (and truncation) in the stochastic store's place fail the case
    with pytest.raises(AssertionError):
        G.check_adam_sr(D, _standin(SR.nearest), SEED)
    with pytest.raises(AssertionError):
        G.check_adam_sr(D, _standin(lambda x: SR.widen(SR.store(x, np.zeros(x.shape, np.uint64)))),
                        SEED)
    # ... and so do the bits of another seed
    with pytest.raises(AssertionError):
        G.check_adam_sr(D, _standin(), SEED + 1)


def test_premise_stall_expected_values():
    from tests import test_gpu_bf16_sr as G

    def run(stochastic):
        out = []
        for kind in (0, 1):
            tabs = []
            for j in (0, 1):
                p = np.ones((G.STALL_ROWS, G.STALL_D), np.float32)
                m, v = np.zeros_like(p), np.zeros_like(p)
                g = np.ones_like(p)
                has = np.ones(G.STALL_ROWS, bool)
                for t in range(1, G.STALL_STEPS + 1):
                    p, m, v = SR.adam_sr(p, m, v, g, has, G.STALL_LR, t, G.STALL_HP, G.SEED, kind,
                                         j, rd=None if stochastic else SR.nearest)
                tabs.append(p)
            out.append(tabs)
        return out
    means = G.check_stall(run)
    print("stall on the CPU: mean displacement per table", [f"{x:.3f}" for x in means])
    # every step asks for exactly 1/16 of the spacing: the fp32 result of the first step
    s = A.make_scalars(G.STALL_LR, G.STALL_HP, 1)
    p1 = A.adam_step(np.ones(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32),
                     np.ones(4, np.float32), None, None, None, A.F32, s=s)[0]
    assert (p1 == np.float32(1.0 - 2.0 ** -12)).all()
    assert int(p1.view(np.uint32)[0]) & 0xFFFF == 0xF000


def test_premise_fused_step_case_holds_for_the_fp32_oracle():
    """test_one_step_against_the_float64_oracle asks for 99 % of a table's elements to equal
    the restated decision made on the float64 oracle's value: the fp32 oracle with the restated
    store stays within a quarter of that gap (99.75 %), and every element is a neighbour."""
    from tests import test_gpu_bf16_sr as G
    from tests import test_gpu_dropout as TD
    c = G.oracle_case()
    seed = TD.case_seeds(G.ORACLE_CASE, 1)[0]
    sd = TD.make_model(c["D"], c["H"], c["M"], c["p"]).state_dict()
    init = TD.bf16_tables({k: v.detach().clone() for k, v in sd.items()})
    batches = TD.make_batches(c["B"], c["M"], 1, c["data_seed"])
    _, ref64 = TD.oracle_run(init, batches, [seed], c["H"], c["M"], c["p"])
    _, ref32 = TD.oracle_run(init, batches, [seed], c["H"], c["M"], c["p"], dtype=torch.float32)
    stored = {}
    for k, K in TD.TABLE_KEYS.items():
        kind, j = int(k.endswith("item")), int(k.startswith("mlp"))
        stored[K] = torch.from_numpy(SR.sr_round(ref32[K].numpy(), G.STEP_SEED, kind, j, 1))
    worst = G.check_step_tables(stored, ref64, G.STEP_SEED, min_equal=0.9975)
    print(f"fp32 oracle with the restated store: {worst:.4%} equal the restated decision")
    near = {K: torch.from_numpy(SR.nearest(ref32[K].numpy())) for K in TD.TABLE_KEYS.values()}
    with pytest.raises(AssertionError):
        G.check_step_tables(near, ref64, G.STEP_SEED)
