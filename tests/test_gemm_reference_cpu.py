"""The yardstick of tests/test_gemm_f64_gpu.py, checked without a GPU (tests/gemm_reference.py): at the GPU cases' shapes the per-element bound
|got - ref64| <= 2^-20 * S accepts a serial float32 evaluation and the host model of the split GEMM as the kernel implements it (scaled low
half, two accumulators) at every operand scale of the sweep — and rejects each defect a GEMM kernel can plausibly have, the unscaled low half
at small weights among them."""
import numpy as np
import pytest

from tests import gemm_reference as R

M, N = R.SPLIT_M, R.SPLIT_N


def _lin(x, w, b=None, acc0=None):
    ref, S, _ = R.linear_f64(x, w, b, None, acc0)
    return ref, S


# ---- the pieces the models are made of ------------------------------------------------------------------------------------------------------

def test_rn16_is_round_to_nearest_even_with_gradual_underflow_and_overflow():
    v = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 65519.99, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                  2.0 ** -14 + 2.0 ** -25, -3 * 2.0 ** -25], np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, 65504.0, np.inf, 2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -14, -2.0 ** -23], np.float32)
    assert np.array_equal(R.rn16(v), want)


def test_split_halves_carry_the_value():
    rng = np.random.RandomState(0)
    for e in (15, 0, -9, -14, -20, -30):
        v = (rng.randn(4096) * 2.0 ** e).astype(np.float32)
        v = v[np.abs(v) < 65520.0]
        hi, lo = R.split_f16(v)
        rest = np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64) * 2.0 ** -R.LO_SHIFT)
        # lo' is a normal fp16 (relative 2^-11 of a value <= 2^-11 |v|) or a subnormal one (absolute 2^-25 before the 2^-11)
        assert bool((rest <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25 * 2.0 ** -R.LO_SHIFT) * (1 + 1e-9)).all()), e
        assert bool(np.isfinite(lo).all()) and float(np.abs(lo).max()) <= 2.0 ** 15
        hi0, lo0 = R.split_f16(v, 0)
        assert np.array_equal(hi0, hi)
        if e == -14:                                   # the unscaled low half: an fp16 subnormal, absolute 2^-25 whatever |v|
            assert float(np.abs(v.astype(np.float64) - hi0 - lo0).max()) > 2.0 ** -27


def test_shift_rows_is_h_prev():
    b = np.arange(1, 27, dtype=np.float64).reshape(13, 2)
    for shift in (-1, 1, -3, 3):
        want = np.zeros_like(b)
        for r in range(13):
            t = r % 5 + shift
            if 0 <= t < 5 and r + shift < 13:
                want[r] = b[r + shift]
        if 13 % 5 and shift > 0:
            continue                                   # a partial last period under a forward shift is the case ttsc_gemm refuses
        assert np.array_equal(R.shift_rows(b, shift, 5), want)
    full = R.shift_rows(b[:10], 1, 5)
    assert np.array_equal(full[[4, 9]], np.zeros((2, 2))) and np.array_equal(full[[0, 5]], b[[1, 6]])
    back = R.shift_rows(b[:10], -1, 5)
    assert np.array_equal(back[[0, 5]], np.zeros((2, 2))) and np.array_equal(back[[4, 9]], b[[3, 8]])


def test_split_k_plan_of_the_gpu_cases():
    assert R.gemm_splits(130, 70, 1040) == (5, 208)           # 2 tiles -> 5 splits that are no multiple of the period 13
    assert R.gemm_splits(130, 70, 260) == (1, 272) and R.gemm_splits(130, 70, 17) == (1, 32)
    assert [R.colsum_parts(r) for r in (1, 1023, 1024, 1025)] == [1, 1, 4, 5]
    assert [R.matvec_parts(r) for r in (1, 63, 64, 65, 1025)] == [1, 1, 2, 2, 32]


# ---- the bound accepts what it must ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', R.SPLIT_KS)
def test_bound_accepts_float32_at_every_scale_pair(K):
    worst = 0.0
    for sx in R.SPLIT_SX:
        for sw in R.SPLIT_SW:
            x, w, b = R.sweep_operands(K, sx, sw)
            ref, S = _lin(x, w, b)
            got = (R.f32_serial(x, w.T) + b).astype(np.float32)           # bias last, as the kernels' epilogues add it
            assert R.within(got, ref, S), (sx, sw)
            worst = max(worst, R.worst_ratio(got, ref, S))
    assert worst <= R.TAU / 2, R.log2_ratio(worst)           # the yardstick (measured 2^-22.6 .. 2^-21.8): tau is ~4 x its worst ratio


@pytest.mark.parametrize('K', [17, 260, 1040])
def test_bound_accepts_float32_gemm_and_fixed_order_split_k(K):
    rng = np.random.RandomState(K)
    a = rng.randn(130, K).astype(np.float32)
    b = rng.randn(K, 70).astype(np.float32)
    c0 = rng.randn(130, 70).astype(np.float32)
    ref, S = R.gemm_f64(a, b, acc0=c0)
    got = R.f32_serial(a, b, acc0=c0)
    assert R.within(got, ref, S) and R.worst_ratio(got, ref, S) <= R.TAU / 2
    splits, kchunk = R.gemm_splits(130, 70, K)
    got = R.splitk_model(a, b, splits, kchunk, acc0=c0)
    assert R.within(got, ref, S) and R.worst_ratio(got, ref, S) <= R.TAU / 2
    # row-shifted B: the float32 evaluation of the materialised operand
    if K == 1040:
        for shift in (-1, 1, -3, 3):
            ref, S = R.gemm_f64(a, b, shift=shift, period=13)
            assert R.within(R.f32_serial(a, R.shift_rows(b, shift, 13)), ref, S)


def test_bound_accepts_float32_colsum_and_matvec():
    rng = np.random.RandomState(3)
    x = rng.randn(1025, 65).astype(np.float32)
    ref, S = R.colsum_f64(x)
    got = R.f32_serial(np.ones((1, 1025), np.float32), x)[0]
    assert R.within(got, ref, S)
    W = rng.randn(1025, 257).astype(np.float32)
    v = rng.randn(257).astype(np.float32)
    u = rng.randn(1025).astype(np.float32)
    for tr, vec in ((False, v), (True, u)):
        ref, S = R.matvec_f64(W, vec, tr)
        got = R.f32_serial(W.T if tr else W, vec[:, None])[:, 0]
        assert R.within(got, ref, S)


@pytest.mark.parametrize('K', R.SPLIT_KS)
def test_bound_accepts_the_scaled_split_model_at_every_scale_pair(K):
    worst = 0.0
    for sx in R.SPLIT_SX:
        for sw in R.SPLIT_SW:
            x, w, b = R.sweep_operands(K, sx, sw)
            ref, S = _lin(x, w, b)
            got = R.split_linear_model(x, w, b)
            assert R.within(got, ref, S), (sx, sw, R.log2_ratio(R.worst_ratio(got, ref, S)))
            worst = max(worst, R.worst_ratio(got, ref, S))
    for x, w, b in (R.mixed_operands(K), R.edge_operands(K)):
        ref, S = _lin(x, w, b)
        got = R.split_linear_model(x, w, b)
        assert R.within(got, ref, S), R.log2_ratio(R.worst_ratio(got, ref, S))
        worst = max(worst, R.worst_ratio(got, ref, S))
    assert worst <= R.TAU / 2, R.log2_ratio(worst)           # measured 2^-24.1 .. 2^-22.2: the float32 yardstick's class at every scale


# ---- ... and rejects every defect -------------------------------------------------------------------------------------------------------------

def test_bound_rejects_the_unscaled_low_half_at_small_scales():
    """lo = rn16(v - hi) with no scale: below |v| ~ 2^-3 it is an fp16 subnormal and keeps an absolute 2^-25 only"""
    x, w, b = R.sweep_operands(256, 0, -9)
    ref, S = _lin(x, w, b)
    bad = R.split_linear_model(x, w, b, lo_shift=0)
    assert not R.within(bad, ref, S)
    assert R.worst_ratio(bad, ref, S) > 2.0 ** -19
    assert R.within(R.split_linear_model(x, w, b), ref, S)
    # the same for a small x; and the decay with the weight scale that the sweep walks down
    for sx, sw in ((-8, 0), (-12, -3), (0, -11), (0, -14), (10, -11)):
        x, w, b = R.sweep_operands(256, sx, sw)
        ref, S = _lin(x, w, b)
        assert not R.within(R.split_linear_model(x, w, b, lo_shift=0), ref, S), (sx, sw)
    # at the one scale the old test used (w ~ 2^-4 and x ~ 1) the unscaled split does hold the bound: the sweep is what sees the defect
    x, w, b = R.sweep_operands(256, 0, -3)
    ref, S = _lin(x, w, b)
    assert R.within(R.split_linear_model(x, w, b, lo_shift=0), ref, S)


@pytest.mark.parametrize('K,drop', [(256, 5), (36, 2)])
def test_bound_rejects_a_dropped_k_slice(K, drop):
    """a whole 16-wide slice, and the last, partial one (K = 36: columns 32..35)"""
    x, w, b = R.sweep_operands(K, 0, -3)
    ref, S = _lin(x, w, b)
    assert not R.within(R.split_linear_model(x, w, b, drop_slices=(drop,)), ref, S)
    a = np.random.RandomState(K).randn(130, 17).astype(np.float32)
    bm = np.random.RandomState(K + 1).randn(17, 70).astype(np.float32)
    ref, S = R.gemm_f64(a, bm)
    assert not R.within(R.f32_serial(a[:, :16], bm[:16]), ref, S)
    a = np.random.RandomState(K).randn(130, 1040).astype(np.float32)
    bm = np.random.RandomState(K + 1).randn(1040, 70).astype(np.float32)
    ref, S = R.gemm_f64(a, bm)
    assert not R.within(R.splitk_model(a, bm, 5, 208, drop=(4,)), ref, S)


@pytest.mark.parametrize('shift', [-1, 1, -3, 3])
def test_bound_rejects_a_wrong_sequence_edge(shift):
    rng = np.random.RandomState(11)
    K, period = 1040, 13
    a = rng.randn(130, K).astype(np.float32)
    b = rng.randn(K, 70).astype(np.float32)
    ref, S = R.gemm_f64(a, b, shift=shift, period=period)
    good = R.shift_rows(b, shift, period)
    edge = ~good.any(axis=1)
    assert int(edge.sum()) == abs(shift) * (K // period)                  # a zero block at every sequence edge, and only there
    not_zeroed = good.copy()
    not_zeroed[edge] = b[edge]                                             # edge rows keep the unshifted row
    across = np.roll(b, -shift, axis=0)                                    # the shift runs into the neighbouring sequence
    globally = across.copy()
    if shift > 0:
        globally[K - shift:] = 0                                           # zeroed only at the ends of the whole operand
    else:
        globally[:-shift] = 0
    for bad in (not_zeroed, across, globally):
        assert not R.within(R.f32_serial(a, bad), ref, S)
    assert R.within(R.f32_serial(a, good), ref, S)


def test_bound_rejects_one_element_off_by_2_to_the_minus_16():
    x, w, b = R.sweep_operands(256, -8, -11)
    ref, S = _lin(x, w, b)
    got = R.split_linear_model(x, w, b).astype(np.float64)
    assert R.within(got, ref, S)
    got[77, 100] += 2.0 ** -16 * S[77, 100]
    assert not R.within(got, ref, S)
    # no absolute floor: the same defect at products of 2^-26 is seen as well
    x, w, b = R.sweep_operands(36, -12, -14)
    ref, S = _lin(x, w, b)
    got = (R.f32_serial(x, w.T) + b).astype(np.float64)
    got[129, 128] -= 2.0 ** -16 * S[129, 128]
    assert float(S.max()) < 1e-5 and not R.within(got, ref, S)


def test_bound_rejects_swapped_mfma_sub_tiles_and_a_doubled_bias():
    x, w, b = R.sweep_operands(256, 0, 0)
    ref, S = _lin(x, w, b)
    got = R.split_linear_model(x, w, b)
    swapped = got.copy()
    swapped[:, 64:96], swapped[:, 96:128] = got[:, 96:128], got[:, 64:96]  # the two 32-column MFMA tiles of one wave
    assert not R.within(swapped, ref, S)
    y0 = np.random.RandomState(5).randn(M, N).astype(np.float32)
    ref, S = _lin(x, w, b, y0)
    assert R.within(R.split_linear_model(x, w, b, acc0=y0), ref, S)
    twice = (R.split_linear_model(x, w, b, acc0=y0) + b).astype(np.float32)
    assert not R.within(twice, ref, S)
    # accumulate sits inside the activation: y = act(x.w + b + y0), not act(x.w + b) + y0
    ref_t, S_t, pre = R.linear_f64(x, w, b, 'tanh', y0)
    assert R.within(np.tanh(pre).astype(np.float32), ref_t, S_t, act='tanh')
    assert not R.within((np.tanh(pre - y0) + y0).astype(np.float32), ref_t, S_t, act='tanh')
