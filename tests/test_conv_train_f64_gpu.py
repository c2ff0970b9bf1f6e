"""GPU: the training convolutions at the kernel level — ttsc_conv_train (csrc/conv_train.hip: conv_f16x3_kernel, folded) forward and data
gradient, and the split-precision weight gradient (csrc/conv_wgrad.hip: wgrad_f16x3_kernel) — held PER ELEMENT to the float64 statement
(tests/conv_train_reference.py) on the tile each case names.

Every case first asks the plan query (ttsc_conv_train_plan / ttsc_conv_wgrad_split_plan: the functions the launchers call) and asserts the
variant it means to reach, then runs, then checks |got - ref64| <= tau * S per element, S the absolute-value companion of the same linear
operation.  tau = 2^-19 for the split-precision kernels and 2^-21 for the exact-fp32 weight gradient: TAU_SPLIT / TAU_EXACT of
tests/test_disc_f64_gpu.py, which holds the same kernels by the same derivation at discriminator shapes.  Outputs are allocated with
torch.empty by the product code; every value must be finite.  The tiles named below are the product's rule: TTSC_TRAIN_NT (the library's
measurement switch, which overrides it) must be unset when the suite runs.

What the shapes reach (tests/test_conv_train_plan_cpu.py pins which of these a real V1 step at b = 16 / b = 128 runs, and asserts that the
lists below name every one of them):
  * the 256-column folded tiles <2,2> and <1,2> at the smallest size that passes the rule ceil(S B / 256) * (CoutP / MT) >= 512, for the
    ResBlock kernels (3, 1), (7, 3), (11, 5) and a 4-tap layer (the transposed layers' data gradient), each beside its neighbour one column
    short of the threshold, which runs the 128-column tile on nearly the same data (test_threshold_pair_*);
  * seams: with B = 3 the utterance boundaries S and 2 S fall at tile columns 1 / 2, 127 / 254 and 255 / 254 of a 256-column tile (and the
    same residues of a 128-column tile), S B = 256 n + 1 leaves a last tile with one column, one case has Lout = 1, and two have a
    padding different from (K - 1) d - padding;
  * thin layers 80 -> 512, 32 -> 1, 1 -> 32;
  * exact cases: the device-side ranging scales by powers of two (pow2_to, conv_kernels.hpp), so integer activations, weights m / 8, a
    power-of-two in_scale and slope 0.5 lose nothing in the fp16 split (proved on the CPU with conv_reference.is_split_exact) and the
    kernel must equal float64 bit for bit on both 256-column tiles;
  * weight gradient: a split that owns several (batch item, chunk) items, straddles batch items, a short last split (items % CH != 0,
    items = want + 1), CH = 3, the tap groups 5 + 5 + 1 (J = 11, step 5), 5 + 5 + 5 + 1 (J = 16), J = 4 with step -1 (the transposed
    layers), rows and columns off the 128 x 64 tile, a chunk with one position, LQ != LP, and the bias gradient riding along at 1, 2, 5
    slices and at the cap.

Measured on an MI355X, worst err / S in units of 2^-24 (test_zz_report_measured prints them): forward <1,1> 4.1, <1,2> 5.7,
<2,1> 3.8, <2,2> 4.9; data gradient 6.5, 4.5, 4.3, 4.6 (bound 32); split weight gradient 1.2 with one and with several items per split (bound
32), the exact-fp32 weight gradient 1.8 (bound 8), the bias gradient riding along 0.15; all six threshold pairs bit-equal."""
import ctypes as C

import pytest
import torch

from tests import conv_reference as CR
from tests import conv_train_reference as R

pytestmark = pytest.mark.gpu

MEASURED = {}
MAGS = (1.0, 1e-6, 1e4)
SCALE, SLOPE = 1.0 / 3.0, 0.1

# ---- ttsc_conv_train, in the kernel's terms: x [B, Cin, Lin] -> y [B, Cout, Lout]; expect = (MI, NJ, tap bucket) ---------------------------
# (id, B, Cin, Cout, K, dilation, padding, Lin, expect)
def _same(K, d):
    return d * (K - 1) // 2


CONV_CASES = []
for _K, _d in ((3, 1), (7, 3), (11, 5)):
    _p = _same(_K, _d)
    # <2,2>: Cout 512 = 8 row tiles; S = Lin + padding = 5376 -> 504 workgroups of 256 columns (stays on <2,1>), 5377 -> 512
    CONV_CASES += [('w22-k%d-below' % _K, 3, 16, 512, _K, _d, _p, 5376 - _p, (2, 1, _K)), ('w22-k%d' % _K, 3, 16, 512, _K, _d, _p, 5377 - _p, (2, 2, _K))]
    # <1,2>: Cout 48 = 2 row tiles of 32 (16 padded rows); S = 21760 -> 510, 21761 -> 512
    CONV_CASES += [('w12-k%d-below' % _K, 3, 32, 48, _K, _d, _p, 21760 - _p, (1, 1, _K)), ('w12-k%d' % _K, 3, 32, 48, _K, _d, _p, 21761 - _p, (1, 2, _K))]
CONV_CASES += [
    # seams of the 256-column tile: S % 256 = 127 (boundaries at columns 127 and 254), 255 (255 and 254); (S = 5377 above: 1 and 2)
    ('w22-seam127', 3, 16, 512, 3, 1, 1, 5503 - 1, (2, 2, 3)),
    ('w22-seam255', 3, 16, 512, 7, 3, 9, 5631 - 9, (2, 2, 7)),
    ('w22-last1', 3, 16, 512, 3, 1, 1, 5547 - 1, (2, 2, 3)),              # S B = 16641 = 65 * 256 + 1: the last tile has one column
    ('w22-pad4', 3, 16, 512, 7, 3, 4, 5500, (2, 2, 7)),                   # padding 4 != (K - 1) d - padding = 14: Lout = Lin - 10, S = Lin + 4
    ('w22-pad14', 3, 16, 512, 7, 3, 14, 5490, (2, 2, 7)),                 # ... and its data-gradient geometry: Lout = Lin + 10 = S
    ('w12-c32', 3, 16, 32, 3, 1, 1, 43606 - 1, (1, 2, 3)),                # one row tile: 256-column tiles from 130 817 columns on
    ('w12-seam127', 3, 32, 48, 11, 5, 25, 21887 - 25, (1, 2, 11)),        # S % 256 = 127
    ('w12-seam255', 3, 32, 48, 3, 1, 1, 22015 - 1, (1, 2, 3)),            # S % 256 = 255
    ('w12-last1', 3, 32, 48, 7, 3, 9, 21931 - 9, (1, 2, 7)),              # S B = 65793 = 257 * 256 + 1
    ('w12-4tap', 3, 40, 48, 4, 1, 0, 21764, (1, 2, 7)),                   # rows u Cout = 5 * 8 -> Cin: the transposed layers' data gradient, M = 4
    ('w22-4tap', 3, 40, 512, 4, 1, 0, 5380, (2, 2, 7)),
    ('w22-1tap', 3, 32, 512, 1, 1, 0, 5377, (2, 2, 3)),                   # M = 1: the K 4, u 4 upsamplers
]
for _tile, _Cin, _Cout in (('n21', 24, 80), ('n11', 24, 32)):      # the 128-column tiles, small: S % 128 = 1, 127, 65 and S B = 128 n + 1
    _mi = 2 if _Cout >= 64 else 1
    CONV_CASES += [
        ('%s-seam1' % _tile, 3, _Cin, _Cout, 3, 1, 1, 129 - 1, (_mi, 1, 3)),
        ('%s-seam127' % _tile, 3, _Cin, _Cout, 7, 3, 9, 255 - 9, (_mi, 1, 7)),
        ('%s-seam65' % _tile, 3, _Cin, _Cout, 11, 5, 25, 193 - 25, (_mi, 1, 11)),
        ('%s-last1' % _tile, 3, _Cin, _Cout, 7, 1, 3, 171 - 3, (_mi, 1, 7)),           # S B = 513
        ('%s-pad4' % _tile, 3, _Cin, _Cout, 7, 3, 4, 200, (_mi, 1, 7)),
        ('%s-pad14' % _tile, 3, _Cin, _Cout, 7, 3, 14, 190, (_mi, 1, 7)),
        ('%s-lout1' % _tile, 3, _Cin, _Cout, 3, 1, 0, 3, (_mi, 1, 3)),                 # Lout = 1
        ('%s-k16' % _tile, 2, _Cin, _Cout, 16, 1, 8, 150, (_mi, 1, 16)),
    ]
CONV_CASES += [
    ('thin-80-512', 2, 80, 512, 7, 1, 3, 50, (2, 1, 7)),                  # conv_pre
    ('thin-32-1', 2, 32, 1, 7, 1, 3, 257, (1, 1, 7)),                     # conv_post
    ('thin-1-32', 2, 1, 32, 7, 1, 3, 257, (1, 1, 7)),                     # conv_post's data gradient
    ('thin-512-80', 2, 512, 80, 7, 1, 3, 50, (2, 1, 7)),
]
CONV_IDS = [c[0] for c in CONV_CASES]

# the same layer on either side of the threshold: (below, at)
PAIRS = [('w22-k%d-below' % k, 'w22-k%d' % k) for k in (3, 7, 11)] + [('w12-k%d-below' % k, 'w12-k%d' % k) for k in (3, 7, 11)]

EXACT_CASES = ['w22-k7', 'w12-k11', 'w22-4tap', 'w12-k3']

# ---- split weight gradient through autograd._wgrad: P [N, A, LP], Q [N, Bc, LQ] -> G [A, Bc, J] ----------------------------------------------
# (id, N, A, Bc, LP, LQ, J, base, step, expect = (CH, splits, tap groups))
WG_CASES = [
    ('straddle', 3, 256, 256, 1450, 1450, 3, -1, 1, (2, 35, (3,))),        # 23 chunks per item (odd): pairs straddle batch items; the last split owns one item
    ('c512', 4, 512, 512, 400, 400, 3, -1, 1, (2, 14, (3,))),              # CH > 1 on a 512 x 512 layer
    ('want+1', 5, 256, 256, 800, 800, 3, -1, 1, (2, 33, (3,))),            # items 65 = want + 1: 32 splits of two items, the last of one
    ('ch3', 6, 512, 512, 512, 512, 3, -1, 1, (3, 16, (3,))),               # three of an item's eight chunks per split
    ('ch6', 24, 512, 512, 251, 251, 3, -1, 1, (6, 16, (3,))),               # a split owns one and a half batch items of four chunks (the last: 59 positions)
    ('ups0-ch6', 40, 1280, 512, 53, 50, 4, 0, -1, (6, 7, (4,))),           # the first upsampler: one chunk per item, six batch items per split, the last split four
    ('k7d3', 3, 256, 256, 1450, 1450, 7, -9, 3, (2, 35, (5, 2))),
    ('k11d5', 3, 256, 256, 1450, 1450, 11, -25, 5, (2, 35, (5, 5, 1))),
    ('j16', 3, 256, 256, 1450, 1450, 16, -8, 1, (2, 35, (5, 5, 5, 1))),
    ('j4-back', 3, 256, 256, 1450, 1447, 4, 0, -1, (2, 35, (4,))),         # ConvTranspose1d: P = dyP [u Cout rows, Lin + M - 1], Q = x [Cin, Lin], taps run backwards
    ('j6-back', 3, 384, 256, 1200, 1195, 6, 0, -1, (2, 29, (5, 1))),       # K 16, u 3: M = 6
    ('j1', 3, 256, 128, 2900, 2900, 1, 0, -1, (2, 69, (1,))),              # K 4, u 4: M = 1
    ('ragged-ch2', 3, 160, 40, 5505, 5505, 3, -1, 1, (2, 131, (3,))),      # rows / columns off the 128 x 64 tile, a last chunk with one position, CH = 2
    ('ragged', 2, 160, 40, 257, 257, 3, -1, 1, (1, 10, (3,))),
    ('lq', 3, 128, 64, 129, 133, 5, 0, 1, (1, 9, (5,))),                   # LQ != LP (no padding: LP = LQ - (J - 1))
    ('c64', 2, 64, 64, 16100, 16100, 7, -3, 1, (1, 504, (5, 2))),          # one tile: want = 512, 504 items
    ('c64-ch2', 2, 64, 64, 16500, 16500, 3, -1, 1, (2, 258, (3,))),        # ... 516 items
]
WG_IDS = [c[0] for c in WG_CASES]

# bias gradient riding in the weight-gradient launches: (N, A, Bc, LP, J, slices)
BIAS_CASES = [(2, 64, 64, 1024, 3, 1), (2, 64, 64, 1025, 3, 2), (2, 64, 32, 5000, 3, 5), (2, 512, 64, 4000, 3, 2), (3, 256, 256, 1450, 7, 2)]


def conv_case(cid):
    return CONV_CASES[CONV_IDS.index(cid)]


def conv_plan(B, Cin, Cout, K, Lin, padding, dilation, groups=1):
    from ttscube_amd import _lib
    info = (C.c_int32 * 10)()
    _lib.check(_lib.lib().ttsc_conv_train_plan(B, Cin, Cout, K, Lin, padding, dilation, groups, info), 'ttsc_conv_train_plan')
    return dict(zip(('MI', 'NJ', 'bucket', 'S', 'cols', 'gx', 'gy', 'lds', 'CinP', 'CoutP'), list(info)))


def wgrad_plan(N, A, Bc, LP, J, step):
    from ttscube_amd import _lib
    info = (C.c_int32 * 9)()
    _lib.check(_lib.lib().ttsc_conv_wgrad_split_plan(N, A, Bc, LP, J, step, info), 'ttsc_conv_wgrad_split_plan')
    d = dict(zip(('chunks', 'items', 'tiles', 'CH', 'splits', 'jt_max', 'launches', 'last', 'bias_slices'), list(info)))
    d['groups'] = tuple([d['jt_max']] * (d['launches'] - 1) + [d['last']])
    return d


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), v)


def _bound(label, got, ref, S, tau):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), label + ': non-finite'
    r = float(((got - ref).abs() / S.clamp(min=1e-300)).max())
    _note(label.split(':')[0], r * 2 ** 24)
    print('%s max err / S = %.3f * 2^-24 (bound %.0f)' % (label, r * 2 ** 24, tau * 2 ** 24))
    assert r <= tau, '%s: max err / S = %.3g * 2^-24 > %.3g * 2^-24' % (label, r * 2 ** 24, tau * 2 ** 24)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def fwd_inputs(cid, mag=1.0):
    """x, w, b, resid of a forward case (CPU, float32)"""
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    g = _gen(CONV_IDS.index(cid) * 7 + 1)
    Lout = R.out_len(Lin, K, pad, d)
    x = torch.randn(B, Cin, Lin, generator=g) * mag
    w = torch.randn(Cout, Cin, K, generator=g) / (Cin * K) ** 0.5
    b = torch.randn(Cout, generator=g) * mag
    r = torch.randn(B, Cout, Lout, generator=g) * mag
    return x, w, b, r


def dgrad_inputs(cid, mag=1.0):
    """dy, w ([Cin, Cout, K]: the forward weight of the differentiated layer), gate of a data-gradient case"""
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    g = _gen(CONV_IDS.index(cid) * 7 + 2)
    Lout = R.out_len(Lin, K, pad, d)
    dy = torch.randn(B, Cin, Lin, generator=g) * mag
    w = torch.randn(Cin, Cout, K, generator=g) / (Cout * K) ** 0.5
    gate = torch.randn(B, Cout, Lout, generator=g)
    return dy, w, gate


def _run_fwd(cid, x, w, b, r, scale=SCALE, slope=SLOPE):
    from ttscube_amd.hifigan.autograd import _conv_split
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    return _conv_split(x.cuda(), w.cuda(), b.cuda(), r.cuda(), None, Cin, Cout, K, pad, d, 0, in_scale=scale, in_slope=slope)


def _run_dgrad(cid, dy, w, gate, scale=SCALE, slope=SLOPE):
    from ttscube_amd.hifigan.autograd import _conv_split
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    return _conv_split(dy.cuda(), w.cuda(), None, None, gate.cuda(), Cin, Cout, K, pad, d, 1, out_scale=scale, gate_slope=slope)


def _assert_plan(cid):
    _, B, Cin, Cout, K, d, pad, Lin, expect = conv_case(cid)
    p = conv_plan(B, Cin, Cout, K, Lin, pad, d)
    assert (p['MI'], p['NJ'], p['bucket']) == expect, (cid, p)
    assert p['S'] == max(Lin + pad, R.out_len(Lin, K, pad, d)) and p['cols'] == p['S'] * B
    return p


def _family(cid):
    return '<%d,%d>' % conv_case(cid)[8][:2]


@pytest.mark.parametrize('mag', MAGS)
@pytest.mark.parametrize('cid', CONV_IDS)
def test_forward_per_element(cid, mag):
    """bias + residual + prologue (in_scale 1/3, slope 0.1)"""
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    _assert_plan(cid)
    x, w, b, r = fwd_inputs(cid, mag)
    y = _run_fwd(cid, x, w, b, r)
    ref = R.launch_fwd(x, w, b, r, pad, d, SCALE, SLOPE)
    S = R.launch_fwd(x, w, b, r, pad, d, SCALE, SLOPE, absolute=True)
    assert tuple(y.shape) == tuple(ref.shape)
    _bound('forward %s: %s mag %g' % (_family(cid), cid, mag), y, ref, S, R.TAU_SPLIT)


@pytest.mark.parametrize('mag', MAGS)
@pytest.mark.parametrize('cid', CONV_IDS)
def test_data_gradient_per_element(cid, mag):
    """flip = 1 on the forward weight, gate, out_scale 1/3, gate_slope 0.1"""
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    _assert_plan(cid)
    dy, w, gate = dgrad_inputs(cid, mag)
    dx = _run_dgrad(cid, dy, w, gate)
    ref = R.launch_dgrad(dy, w, gate, pad, d, SCALE, SLOPE)
    S = R.launch_dgrad(dy, w, gate, pad, d, SCALE, SLOPE, absolute=True)
    assert tuple(dx.shape) == tuple(ref.shape)
    _bound('dgrad %s: %s mag %g' % (_family(cid), cid, mag), dx, ref, S, R.TAU_SPLIT)


@pytest.mark.parametrize('below,at', PAIRS)
def test_threshold_pair_common_prefix(below, at):
    """the same layer one column below the 512-workgroup rule (128-column tile) and at it (256-column tile), the shorter input a prefix of the
    longer one (the largest magnitude planted in the prefix, so both launches derive the same power-of-two ranges): both meet the bound
    (test_forward_per_element); here their outputs must agree bit for bit on the part of utterance 0 no tap of which sees the difference"""
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(at)
    assert conv_case(below)[1:7] == conv_case(at)[1:7] and conv_case(below)[7] == Lin - 1
    assert _assert_plan(below)['NJ'] == 1 and _assert_plan(at)['NJ'] == 2
    x, w, b, r = fwd_inputs(at)
    x[0, 0, 0] = 8.0
    y_at = _run_fwd(at, x, w, b, r)
    y_lo = _run_fwd(below, x[:, :, :Lin - 1].contiguous(), w, b, r[:, :, :r.shape[2] - 1].contiguous())
    n = r.shape[2] - 1 - (K - 1) * d
    a, c = y_at[0, :, :n], y_lo[0, :, :n]
    same = torch.equal(a, c)
    dist = float((a.double() - c.double()).abs().max())
    print('threshold pair %s / %s: bit-equal %s, max |difference| %.3g' % (below, at, same, dist))
    _note('pair %s differs' % at, 0.0 if same else 1.0)
    assert same, (below, at, dist)      # measured bit-equal on the MI355X and promised in docs/KERNELS.md


def _pow2_to(m, target):
    """conv_kernels.hpp::pow2_to for a normal float m"""
    import math
    return 2.0 ** (target - math.frexp(m)[1])


def exact_inputs(cid):
    _, B, Cin, Cout, K, d, pad, Lin, _ = conv_case(cid)
    g = _gen(CONV_IDS.index(cid) + 1000)
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float()
    Lout = R.out_len(Lin, K, pad, d)
    return dict(x=ints((B, Cin, Lin), -8, 8), w=ints((Cout, Cin, K), -8, 8) / 8.0, b=ints((Cout,), -5, 5), r=ints((B, Cout, Lout), -9, 9),
                dy=ints((B, Cin, Lin), -8, 8), wt=ints((Cin, Cout, K), -8, 8) / 8.0, gate=ints((B, Cout, Lout), -8, 8))


def exact_is_exact(c, scale=0.5, slope=0.5):
    """the CPU proof: both operands of both launches survive the fp16 hi / lo split under the kernel's power-of-two ranges"""
    a = R.lrelu(c['x'].double() * scale, slope)
    sx = _pow2_to(float(c['x'].abs().max()) * scale, 15)
    ok = CR.is_split_exact(a * sx) and CR.is_split_exact(c['w'].double() * _pow2_to(float(c['w'].abs().max()), 10))
    sd = _pow2_to(float(c['dy'].abs().max()), 15)
    return ok and CR.is_split_exact(c['dy'].double() * sd) and CR.is_split_exact(c['wt'].double() * _pow2_to(float(c['wt'].abs().max()), 10))


@pytest.mark.parametrize('cid', EXACT_CASES)
def test_exact_inputs_equal_float64_bit_for_bit(cid):
    """integer activations, weights m / 8, in_scale 1/2, slope 1/2: every product and every partial sum is a multiple of 2^-5 below 2^11, nothing
    rounds in fp16, fp32 or float64 — the kernel's output must BE the float64 result"""
    _, B, Cin, Cout, K, d, pad, Lin, expect = conv_case(cid)
    assert _assert_plan(cid)['NJ'] == 2
    c = exact_inputs(cid)
    assert exact_is_exact(c)
    y = _run_fwd(cid, c['x'], c['w'], c['b'], c['r'], 0.5, 0.5)
    ref = R.launch_fwd(c['x'], c['w'], c['b'], c['r'], pad, d, 0.5, 0.5)
    assert torch.equal(y.double().cpu(), ref), float((y.double().cpu() - ref).abs().max())
    dx = _run_dgrad(cid, c['dy'], c['wt'], c['gate'], 0.5, 0.5)
    ref = R.launch_dgrad(c['dy'], c['wt'], c['gate'], pad, d, 0.5, 0.5)
    assert torch.equal(dx.double().cpu(), ref), float((dx.double().cpu() - ref).abs().max())


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------------
def wg_inputs(wid, mag=1.0):
    _, N, A, Bc, LP, LQ, J, base, step, _ = WG_CASES[WG_IDS.index(wid)]
    g = _gen(WG_IDS.index(wid) * 11 + 3)
    return torch.randn(N, A, LP, generator=g) * mag, torch.randn(N, Bc, LQ, generator=g)


@pytest.mark.parametrize('mag', (1.0, 1e-6))
@pytest.mark.parametrize('wid', WG_IDS)
def test_split_weight_gradient_per_element(wid, mag):
    from ttscube_amd.hifigan import autograd as AG
    _, N, A, Bc, LP, LQ, J, base, step, expect = WG_CASES[WG_IDS.index(wid)]
    p = wgrad_plan(N, A, Bc, LP, J, step)
    assert (p['CH'], p['splits'], p['groups']) == expect, (wid, p)
    assert p['items'] == N * -(-LP // 64) and (p['splits'] - 1) * p['CH'] < p['items'] <= p['splits'] * p['CH']
    P, Q = wg_inputs(wid, mag)
    assert AG.SPLIT_TRAIN
    G = AG._wgrad(P.cuda(), Q.cuda(), A, Bc, J, base, step, SCALE, SLOPE)
    ref = R.wgrad(P, Q, J, base, step, SCALE, SLOPE)
    S = R.wgrad(P, Q, J, base, step, SCALE, SLOPE, absolute=True)
    assert tuple(G.shape) == tuple(ref.shape)
    _bound('wgrad split CH %d: %s mag %g' % (min(p['CH'], 2), wid, mag), G, ref, S, R.TAU_SPLIT)
    try:      # the exact-fp32 kernel on the same inputs
        AG.SPLIT_TRAIN = False
        G32 = AG._wgrad(P.cuda(), Q.cuda(), A, Bc, J, base, step, SCALE, SLOPE)
    finally:
        AG.SPLIT_TRAIN = True
    _bound('wgrad exact: %s mag %g' % (wid, mag), G32, ref, S, R.TAU_EXACT)


@pytest.mark.parametrize('N,A,Bc,LP,J,slices', BIAS_CASES)
def test_bias_gradient_riding_along(N, A, Bc, LP, J, slices):
    """db from the weight-gradient launches: the bits of ttsc_bias_grad, the weight gradient unchanged, and float64 per element"""
    from ttscube_amd.hifigan.autograd import TrainConv, _bias_grad, _wgrad
    p = wgrad_plan(N, A, Bc, LP, J, 1)
    assert p['bias_slices'] == slices, p
    g = _gen(N + A + LP)
    P = torch.randn(N, A, LP, generator=g)
    Q = torch.randn(N, Bc, LP, generator=g)
    dbl = []
    G1 = _wgrad(P.cuda(), Q.cuda(), A, Bc, J, -(J // 2), 1, SCALE, SLOPE, db=dbl)
    G0 = _wgrad(P.cuda(), Q.cuda(), A, Bc, J, -(J // 2), 1, SCALE, SLOPE)
    assert len(dbl) == 1 and torch.equal(G0, G1)
    assert torch.equal(dbl[0], _bias_grad(TrainConv(Bc, A, J, padding=J // 2), P.cuda()))
    # (a sum of N LP / slices <= 10 000 terms over 1024 accumulators: at most 3 sequential adds, 2 to join a thread's four accumulators, 6 shuffle
    # levels, 3 to join the waves, 4 to join the slices: 18 roundings, each at most 2^-24 S — bound 2^-19 S)
    _bound('wgrad bias: slices %d' % slices, dbl[0], P.double().sum((0, 2)), P.double().abs().sum((0, 2)), 2.0 ** -19)
    ref = R.wgrad(P, Q, J, -(J // 2), 1, SCALE, SLOPE)
    _bound('wgrad split with bias: A %d LP %d' % (A, LP), G1, ref, R.wgrad(P, Q, J, -(J // 2), 1, SCALE, SLOPE, absolute=True), R.TAU_SPLIT)


def test_zz_report_measured():
    """prints the worst measured err / S per path (units of 2^-24)"""
    for k in sorted(MEASURED):
        print('MEASURED %-40s %.3f' % (k, MEASURED[k]))
