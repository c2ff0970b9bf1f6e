"""The references of tests/test_conv_infer_f64_gpu.py, checked without a GPU: every "exact" case the GPU tests hold the kernels to bit for bit
really has no rounding (a property of the reference alone), and the float32 yardstick itself meets the derived element-wise bound."""
import pytest
import torch

from tests import conv_reference as R


def _assert_exact_single(c):
    kw = c['kw']
    args = (c['x'], c['w'], c['b'])
    ref = R.conv_f64(*args, resid=c['resid'], acc0=c['acc0'], **kw)
    fwd = R.conv_f32_sequential(*args, resid=c['resid'], acc0=c['acc0'], **kw)
    rev = R.conv_f32_sequential(*args, resid=c['resid'], acc0=c['acc0'], reverse=True, **kw)
    assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref)
    assert R.is_split_exact(R.prologue_f64(c['x'], kw.get('in_scale', 1.0), kw.get('in_slope', 1.0)))
    assert float(c['w'].abs().max()) <= 1.0 and torch.equal(c['w'] * 8, (c['w'] * 8).round())


def _general_exact_cases():
    seen = set()
    for prec in ('f16x3', 'fp32'):
        for layer, transposed, _, lengths in R.general_variants(prec):
            for L in lengths:
                if (layer, transposed, L) not in seen:
                    seen.add((layer, transposed, L))
                    yield layer, transposed, L


@pytest.mark.parametrize('transposed', [False, True])
def test_general_exact_cases_have_no_rounding(transposed):
    n = 0
    for layer, tr, L in _general_exact_cases():
        if tr == transposed:
            _assert_exact_single(R.general_exact(layer, tr, L))
            n += 1
    assert n >= 20
    # the ragged case of the general kernel: [nt + 1, 7]
    for nt in (128, 256, 512):
        c = R.general_exact((32, 32, 11, 5), False, nt + 1)
        for i, n_i in enumerate((nt + 1, 7)):
            _assert_exact_single(dict(c, x=c['x'][i:i + 1, :, :n_i], resid=c['resid'][i:i + 1, :, :n_i], acc0=c['acc0'][i:i + 1, :, :n_i]))


@pytest.mark.parametrize('C', [128, 256])
def test_wide_exact_cases_have_no_rounding(C):
    for C_, k, d, L in R.WIDE_CASES:
        if C_ == C:
            _assert_exact_single(R.exact_case(C, C, k, L, dilation=d, in_slope=0.5))
            _assert_exact_single(R.exact_case(C, C, k, L, dilation=d, resid=True, acc0=True, in_scale=0.5, in_slope=0.25))


def test_tall_and_cout1_exact_cases_have_no_rounding():
    for cin, cout, k, s, L in R.TALL_CASES:
        _assert_exact_single(R.exact_case(cin, cout, k, L, stride=s, transposed=True, in_slope=0.25))
    for cin, L in R.COUT1_CASES:
        _assert_exact_single(R.exact_case(cin, 1, 7, L, resid=True, acc0=True, in_scale=0.5, in_slope=0.25))


@pytest.mark.parametrize('C,k', R.CHAIN_CONFIGS)
def test_chain_exact_cases_have_no_rounding(C, k):
    for il in (True, False):
        nto = R.chain_geometry(C, k, interleaved=il)[3]
        for L in sorted(set(R.chain_lengths(nto))):
            c = R.exact_chain_case(C, k, R.CHAIN_DILS, L)
            ref, entering = R.chain_f64(c['x'], c['layers'], k)
            assert torch.equal(R.chain_f32_sequential(c['x'], c['layers'], k).double(), ref)
            assert torch.equal(R.chain_f32_sequential(c['x'], c['layers'], k, reverse=True).double(), ref)
            assert torch.equal((ref + c['acc0'].double()).float().double(), ref + c['acc0'].double())
            assert all(R.is_split_exact(a) for a in entering)
            assert float(c['x'].min()) >= 0
    # coverage of the sparse weights: every tap and every 16-channel input chunk is used inside every 32-row tile, row sums stay <= 1/2
    for w1, b1, w2, b2, d in c['layers']:
        for w in (w1, w2):
            assert float(w.min()) >= 0 and float(w.sum(dim=(1, 2)).max()) <= 0.5
            for r0 in range(0, C, 32):
                t = w[r0:r0 + 32]
                assert bool((t.sum(dim=(0, 1)) > 0).all()), 'a tap is unused in a 32-row tile'
                assert bool((t.reshape(32, C // 16, 16, k).sum(dim=(0, 2, 3)) > 0).all()), 'an input chunk is unused in a 32-row tile'


@pytest.mark.parametrize('cin,cout,k,L,kw', [
    (80, 128, 7, 129, dict()), (32, 32, 11, 257, dict(dilation=5, resid=True, acc0=True, in_scale=1.0 / 3.0, in_slope=0.1)),
    (20, 24, 3, 65, dict(in_slope=0.1)), (128, 128, 7, 257, dict(dilation=3, resid=True, acc0=True, in_scale=1.0 / 3.0, in_slope=0.1)),
    (64, 32, 4, 130, dict(stride=4, transposed=True, in_slope=0.1)), (32, 16, 16, 33, dict(stride=8, transposed=True, in_slope=0.1)),
    (256, 128, 16, 40, dict(stride=3, transposed=True, in_slope=0.1)), (32, 1, 7, 1025, dict(in_slope=0.01, resid=True, acc0=True)),
    (128, 128, 3, 257, dict(dilation=5, resid=True, acc0=True, in_scale=1.0 / 3.0, in_slope=0.1, init_first=True)),
])
def test_yardstick_meets_the_derived_bound(cin, cout, k, L, kw):
    """|yardstick - ref64| <= (n + 16) 2^-24 A + 2^-24 W element-wise: were this to fail, the derivation (not a kernel) would be wrong"""
    c, ref, yard, A, W = R.cached_random(cin, cout, k, L, **kw)
    n = R.n_terms(cin, k, kw.get('stride', 1), kw.get('transposed', False), True, c['resid'] is not None, c['acc0'] is not None)
    bound = R.derived_bound(n, A, W)
    err = (yard.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) > 0   # (the random cases do round: the bound is not vacuous)


def test_geometry_tables():
    assert [R.mt_class(c) for c in (128, 24, 32, 64, 80, 100)] == [128, 32, 32, 64, 32, 128]
    assert R.mt_class(64, 4, True) == 128 and R.mt_class(32, 4, True) == 128 and R.mt_class(16, 8, True) == 32
    seen = {t for _, _, t, _ in R.general_variants('fp32')}
    assert seen == {(128, 128), (64, 128), (64, 64), (64, 256), (32, 512), (32, 256), (32, 128)}   # all seven fp32 tiles
    assert {t for _, _, t, _ in R.general_variants('f16x3')} == {(64, 256), (64, 128), (32, 128), (32, 512), (32, 256)}
    # (large tile, columns, halo, output columns, interleaved) of the chain's own choice
    assert R.chain_geometry(32, 7) == (False, 512, 36, 440, False)
    assert R.chain_geometry(32, 11) == (True, 1024, 60, 896, True)       # 904 rounded down to a multiple of 32
    assert R.chain_geometry(32, 11, interleaved=False)[3] == 904
    assert R.chain_geometry(64, 7) == (True, 512, 36, 416, True)         # 440 rounded down
    assert R.chain_geometry(128, 3) == (False, 256, 12, 232, True)
