"""CPU: the launch rules of the training convolutions (csrc/conv_train.hip::conv_train_plan and csrc/conv_wgrad.hip::wgrad_split_plan with its
tap grouping, through the queries ttsc_conv_train_plan / ttsc_conv_wgrad_split_plan — the functions the launchers themselves call) against
a Python restatement: on either side of every threshold, and over every convolution of the HiFi-GAN V1 generator (forward, data gradient,
weight gradient, as hifigan/autograd.py::HipConvFn dispatches them) at the trainer's crop (50 frames, training.cubegan_training_step) and
batch sizes 16 and 128.  REACHED_* pin what those two steps run; the last tests assert that the GPU case lists of
tests/test_conv_train_f64_gpu.py name every row, so a tile or a split shape the trainer reaches cannot be left without a float64 check.

TTSC_TRAIN_NT (the library's measurement switch, read once per process inside conv_train_plan) must be UNSET when the suite runs: the
restatement mirrors it, so query and restatement still agree under it, but the pinned tables, the threshold values and every tile a GPU case
names state the product's rule, which the switch overrides."""
import ctypes as C
import os

import pytest

from oracle import hifigan_ref
from tests import test_conv_train_f64_gpu as G

NT_ENV = int(os.environ.get('TTSC_TRAIN_NT', '0') or 0)   # (measurement switch of the library, read once per process: mirrored, never set here)
CROP = 50


def _cdiv(a, b):
    return -(-a // b)


def _up(a, b):
    return _cdiv(a, b) * b


def train_mt(Cout, groups, K):
    cout_g = Cout // groups
    if K > 21:
        return 0 if (groups > 1 and not (cout_g % 32 == 0 or 32 % cout_g == 0)) else 32
    mt = 64 if Cout >= 64 else 32
    if groups > 1:
        mt = 64 if cout_g % 64 == 0 else 32
        if not (cout_g % mt == 0 or mt % cout_g == 0):
            return 0
    return mt


def plan_conv(B, Cin, Cout, K, Lin, padding, dilation, groups=1):
    MT = train_mt(Cout, groups, K)
    MI = MT // 32
    cin_g, cout_g = Cin // groups, Cout // groups
    cin_tile = (MT // cout_g if MT > cout_g else 1) * cin_g if groups > 1 else Cin
    CinP, CoutP = _up(cin_tile, 16), _up(Cout, MT)
    Lout = Lin + 2 * padding - dilation * (K - 1)
    S = max(Lin + padding, Lout)
    cols = S * B
    wg256 = _cdiv(cols, 256) * (CoutP // MT)
    nt = 128 if K > 16 else (NT_ENV if NT_ENV else (256 if wg256 >= 512 else 128))
    NJ = 2 if nt == 256 else 1
    bucket = 41 if K > 21 else next(t for t in (3, 7, 11, 16, 21) if K <= t)
    return dict(MI=MI, NJ=NJ, bucket=bucket, S=S, cols=cols, gx=_cdiv(cols, 128 * NJ), gy=CoutP // MT,
                lds=(nt + (K - 1) * dilation) * 64 + K * MI * 2048, CinP=CinP, CoutP=CoutP)


def plan_wgrad(N, A, Bc, LP, J, step):
    chunks = _cdiv(LP, 64)
    items = N * chunks
    tiles = _cdiv(A, 128) * _cdiv(Bc, 64)
    want = min(max(_cdiv(512, tiles), 1), items)
    CH = _cdiv(items, want)
    splits = _cdiv(items, CH)
    jt_max = min(5, 64 // abs(step) + 1)
    launches = _cdiv(J, jt_max)
    last = J - (launches - 1) * jt_max
    s = min(_cdiv(LP, 1024), _cdiv(1024, A))
    return dict(chunks=chunks, items=items, tiles=tiles, CH=CH, splits=splits, jt_max=jt_max, launches=launches, last=last,
                bias_slices=max(s, 1), groups=tuple([jt_max] * (launches - 1) + [last]))


def _supported(Cin, Cout, K, d):
    from ttscube_amd import _lib
    return bool(_lib.lib().ttsc_conv_train_supported(Cin, Cout, K, d, 1))


def _wg_supported(A, Bc, J, step):
    from ttscube_amd import _lib
    return bool(_lib.lib().ttsc_conv_wgrad_split_supported(A, Bc, J, step))


CONV_THRESHOLDS = [  # B, Cin, Cout, K, Lin, padding, dilation
    (3, 16, 512, 3, 5375, 1, 1), (3, 16, 512, 3, 5376, 1, 1),           # 504 / 512 workgroups of 256 columns
    (1, 32, 64, 3, 511 * 256 - 1, 1, 1), (1, 32, 64, 3, 511 * 256, 1, 1),   # 511 / 512 with one row tile
    (2, 32, 64, 16, 70000, 8, 1), (2, 32, 64, 17, 70000, 8, 1),         # K 16 / 17: 17+ taps stay on 128 columns
    (2, 32, 64, 21, 300, 10, 1), (2, 32, 64, 22, 300, 10, 1),           # K 21 / 22: bucket 21 / 41, 32-row tiles
    (2, 32, 63, 3, 300, 1, 1), (2, 32, 64, 3, 300, 1, 1),               # Cout 63 / 64: 32- / 64-row tiles
    (2, 32, 64, 3, 300, 1, 1), (2, 32, 64, 4, 300, 1, 1), (2, 32, 64, 7, 300, 3, 1), (2, 32, 64, 8, 300, 3, 1), (2, 32, 64, 11, 300, 5, 1),
    (2, 32, 64, 12, 300, 5, 1),                                         # bucket edges 3 / 7 / 11
]


@pytest.mark.parametrize('B,Cin,Cout,K,Lin,pad,d', CONV_THRESHOLDS)
def test_conv_plan_at_thresholds(B, Cin, Cout, K, Lin, pad, d):
    assert G.conv_plan(B, Cin, Cout, K, Lin, pad, d) == plan_conv(B, Cin, Cout, K, Lin, pad, d)


def test_conv_plan_threshold_values():
    """the pairs above really sit on either side"""
    p = lambda *a: plan_conv(*a)
    assert (p(3, 16, 512, 3, 5375, 1, 1)['NJ'], p(3, 16, 512, 3, 5376, 1, 1)['NJ']) == (1, 2)
    assert (p(1, 32, 64, 3, 511 * 256 - 1, 1, 1)['NJ'], p(1, 32, 64, 3, 511 * 256, 1, 1)['NJ']) == (1, 2)
    assert _cdiv(511 * 256, 256) == 511 and _cdiv(511 * 256 + 1, 256) == 512
    assert (p(2, 32, 64, 16, 70000, 8, 1)['NJ'], p(2, 32, 64, 17, 70000, 8, 1)['NJ']) == (2, 1)
    assert (p(2, 32, 64, 21, 300, 10, 1)['bucket'], p(2, 32, 64, 22, 300, 10, 1)['bucket']) == (21, 41)
    assert (p(2, 32, 64, 21, 300, 10, 1)['MI'], p(2, 32, 64, 22, 300, 10, 1)['MI']) == (2, 1)
    assert (p(2, 32, 63, 3, 300, 1, 1)['MI'], p(2, 32, 64, 3, 300, 1, 1)['MI']) == (1, 2)


def test_conv_plan_refuses_what_the_launch_refuses():
    from ttscube_amd import _lib
    info = (C.c_int32 * 10)()
    L = _lib.lib()
    assert L.ttsc_conv_train_plan(2, 64, 64, 41, 300, 40, 2, 1, info) < 0          # receptive field beyond the staged window
    assert L.ttsc_conv_train_plan(2, 64, 64, 7, 10, 0, 3, 1, info) < 0             # no output position
    assert L.ttsc_conv_train_plan(0, 64, 64, 3, 10, 1, 1, 1, info) < 0
    assert L.ttsc_conv_wgrad_split_plan(2, 32, 64, 100, 3, 1, (C.c_int32 * 9)()) < 0   # fewer than 64 rows


WG_THRESHOLDS = [  # N, A, Bc, LP, J, step
    (4, 256, 256, 16 * 64, 3, 1), (5, 256, 256, 13 * 64, 3, 1),         # 8 tiles: want 64; items 64 = want, 65 = want + 1
    (2, 512, 512, 8 * 64, 3, 1), (1, 512, 512, 17 * 64, 3, 1),          # 32 tiles: want 16; items 16, 17
    (1, 64, 64, 512 * 64, 3, 1), (1, 64, 64, 513 * 64, 3, 1),           # one tile: want 512
    (2, 128, 64, 1024, 5, 1), (2, 128, 64, 1025, 6, 1), (2, 128, 64, 100, 11, 5), (2, 128, 64, 100, 16, 1), (2, 128, 64, 100, 4, -1),
    (2, 128, 64, 100, 5, 16), (2, 128, 64, 100, 5, 17), (2, 128, 64, 100, 3, 32), (2, 128, 64, 100, 3, 33), (2, 128, 64, 100, 2, 64),
    (2, 64, 32, 5000, 3, 1), (2, 512, 64, 4000, 3, 1), (2, 1024, 64, 4000, 3, 1), (2, 1025, 64, 4000, 3, 1),
]


@pytest.mark.parametrize('N,A,Bc,LP,J,step', WG_THRESHOLDS)
def test_wgrad_plan_at_thresholds(N, A, Bc, LP, J, step):
    assert G.wgrad_plan(N, A, Bc, LP, J, step) == plan_wgrad(N, A, Bc, LP, J, step)


def test_wgrad_plan_threshold_values():
    assert (plan_wgrad(4, 256, 256, 1024, 3, 1)['CH'], plan_wgrad(5, 256, 256, 832, 3, 1)['CH']) == (1, 2)
    assert plan_wgrad(5, 256, 256, 832, 3, 1)['splits'] == 33
    assert (plan_wgrad(2, 512, 512, 512, 3, 1)['CH'], plan_wgrad(1, 512, 512, 17 * 64, 3, 1)['CH']) == (1, 2)
    assert (plan_wgrad(1, 64, 64, 512 * 64, 3, 1)['CH'], plan_wgrad(1, 64, 64, 513 * 64, 3, 1)['CH']) == (1, 2)
    assert plan_wgrad(2, 128, 64, 100, 11, 5)['groups'] == (5, 5, 1) and plan_wgrad(2, 128, 64, 100, 16, 1)['groups'] == (5, 5, 5, 1)
    assert plan_wgrad(2, 128, 64, 100, 5, 16)['groups'] == (5,) and plan_wgrad(2, 128, 64, 100, 5, 17)['groups'] == (4, 1)
    assert plan_wgrad(2, 128, 64, 100, 3, 32)['groups'] == (3,) and plan_wgrad(2, 128, 64, 100, 3, 33)['groups'] == (2, 1)
    assert [plan_wgrad(2, 64, 32, LP, 3, 1)['bias_slices'] for LP in (1024, 1025, 5000)] == [1, 2, 5]
    assert plan_wgrad(2, 512, 64, 4000, 3, 1)['bias_slices'] == 2 and plan_wgrad(2, 1025, 64, 4000, 3, 1)['bias_slices'] == 1


# ---- the V1 generator at the trainer's crop -----------------------------------------------------------------------------------------------
def v1_launches(b, h=None):
    """(name, leg, kind, arguments of the plan query) for every convolution of the generator as HipConvFn runs it: Conv1d forward / data gradient
    on ttsc_conv_train, weight gradient on the split kernel where it is supported; ConvTranspose1d backward on the de-interleaved gradient"""
    h = h or hifigan_ref.CONFIG_V1
    out = []

    def conv1d(name, Cin, Cout, K, d, L):
        p = d * (K - 1) // 2
        assert _supported(Cin, Cout, K, d) and _supported(Cout, Cin, K, d)
        out.append((name, 'fwd', 'conv', (b, Cin, Cout, K, L, p, d)))
        out.append((name, 'dgrad', 'conv', (b, Cout, Cin, K, L, d * (K - 1) - p, d)))
        if _wg_supported(Cout, Cin, K, d):
            out.append((name, 'wgrad', 'wg', (b, Cout, Cin, L, K, d)))

    ch, L = h['upsample_initial_channel'], CROP
    conv1d('conv_pre', h['num_mels'], ch, 7, 1, L)
    for i, (u, k) in enumerate(zip(h['upsample_rates'], h['upsample_kernel_sizes'])):
        p = (k - u) // 2
        m_lo, m_hi = (0 - p) // u, (k - 1 - p) // u
        M = m_hi - m_lo + 1
        co = ch // 2
        if _supported(u * co, ch, M, 1):
            out.append(('ups.%d' % i, 'dgrad', 'conv', (b, u * co, ch, M, L + M - 1, 0, 1)))
        if _wg_supported(u * co, ch, M, -1):
            out.append(('ups.%d' % i, 'wgrad', 'wg', (b, u * co, ch, L + M - 1, M, -1)))
        ch, L = co, (L - 1) * u - 2 * p + k
        for kr, ds in zip(h['resblock_kernel_sizes'], h['resblock_dilation_sizes']):
            for d in ds:
                conv1d('rb%d.k%d.c1.d%d' % (i, kr, d), ch, ch, kr, d, L)
                conv1d('rb%d.k%d.c2' % (i, kr), ch, ch, kr, 1, L)
    conv1d('conv_post', ch, 1, 7, 1, L)
    return out


def test_crop_lengths():
    # K 16, u 5, p 5 gives 5 L + 1; K 16, u 3, p 6 gives 3 L + 1; K 4, u 4 gives 4 L
    ls = [a[4] for n, leg, kind, a in v1_launches(16) if leg == 'fwd' and (n.endswith('k3.c1.d1') or n == 'conv_post')]
    assert ls == [251, 754, 3016, 12064, 12064]


@pytest.mark.parametrize('b', [16, 128])
def test_query_equals_restatement_over_the_generator(b):
    for name, leg, kind, a in v1_launches(b):
        if kind == 'conv':
            assert G.conv_plan(*a) == plan_conv(*a), (name, leg, a)
        else:
            assert G.wgrad_plan(*a) == plan_wgrad(*a), (name, leg, a)


# what the two steps reach: {(MI, NJ, tap bucket)} of ttsc_conv_train, and for the weight gradients whose splits own more than one item
# {(tap groups, taps run backwards)}
# b = 16: the 512- .. 64-channel stages and every upsampler's data gradient on <2,1>, the 32-channel stage and conv_post on <1,2>;
# b = 128: the 256-, 128- and 64-channel stages and the last three upsamplers' data gradients on <2,2> (conv_pre, the first upsampler stay on <2,1>)
REACHED_TILES = {
    16: {(2, 1, 3), (2, 1, 7), (2, 1, 11), (1, 2, 3), (1, 2, 7), (1, 2, 11)},
    128: {(2, 1, 3), (2, 1, 7), (2, 2, 3), (2, 2, 7), (2, 2, 11), (1, 2, 3), (1, 2, 7), (1, 2, 11)},
}
# b = 16: CH = 2 on the 64-channel stage and the upsamplers (CH = 3 on the first: 16 items of one chunk each over 6 splits);
# b = 128: CH = 8 / 6 / 12 on the 256- / 128- / 64-channel stages, 19 / 12 / 12 / 12 on the upsamplers, 2 on conv_pre
REACHED_SPLITS = {b: {((3,), False), ((5, 2), False), ((5, 5, 1), False), ((1,), True), ((4,), True), ((5, 1), True)} for b in (16, 128)}
REACHED_MAX_CH = {16: 3, 128: 19}
# (CH, splits) of every weight gradient whose splits own more than one item, per layer class (the eighteen layers of a ResBlock stage share one
# shape; the 32-channel stage and conv_post have fewer than 64 rows and run the exact-fp32 kernel; everything not listed has CH = 1)
REACHED_CH_SPLITS = {
    16: {'ups.0': (3, 6), 'ups.1': (2, 32), 'ups.2': (2, 96), 'rb2': (2, 384), 'ups.3': (2, 384)},
    128: {'conv_pre': (2, 64), 'ups.0': (19, 7), 'rb0': (8, 64), 'ups.1': (12, 43), 'rb1': (6, 256), 'ups.2': (12, 128), 'rb2': (12, 512),
          'ups.3': (12, 512)},
}


def _reached(b):
    tiles, splits, short_last, max_ch = set(), set(), False, 1
    for name, leg, kind, a in v1_launches(b):
        if kind == 'conv':
            p = plan_conv(*a)
            tiles.add((p['MI'], p['NJ'], p['bucket']))
        else:
            p = plan_wgrad(*a)
            if p['CH'] > 1:
                splits.add((p['groups'], a[5] < 0))
                short_last |= p['items'] % p['CH'] != 0
                max_ch = max(max_ch, p['CH'])
    return tiles, splits, short_last, max_ch


@pytest.mark.parametrize('b', [16, 128])
def test_pinned_table_of_what_a_step_reaches(b):
    tiles, splits, _, _ = _reached(b)
    assert tiles == REACHED_TILES[b], sorted(tiles)
    assert splits == REACHED_SPLITS[b], sorted(splits)
    assert _reached(b)[3] == REACHED_MAX_CH[b]
    per_class = {}
    for name, leg, kind, a in v1_launches(b):
        if kind == 'wg':
            p = plan_wgrad(*a)
            if p['CH'] > 1:
                per_class.setdefault(name.split('.k')[0], set()).add((p['CH'], p['splits']))
    assert per_class == {k: {v} for k, v in REACHED_CH_SPLITS[b].items()}, per_class


def test_gpu_cases_name_every_reached_row():
    """tests/test_conv_train_f64_gpu.py asserts each case's plan before it runs, so naming a row there means running it"""
    conv_named = {c[8] for c in G.CONV_CASES}
    wg_named = {(c[9][2], c[8] < 0) for c in G.WG_CASES if c[9][0] > 1}
    for b in (16, 128):
        assert REACHED_TILES[b] <= conv_named, sorted(REACHED_TILES[b] - conv_named)
        assert REACHED_SPLITS[b] <= wg_named, sorted(REACHED_SPLITS[b] - wg_named)
    # among the cases: a short last split (items % CH != 0), a split whose items straddle batch items (chunks % CH != 0), a split that owns
    # several whole batch items (CH > chunks: the first upsampler at b = 128 has 19 one-chunk items per split; a tensor of a few MB reaches 6 — CH =
    # ceil(items / ceil(512 / tiles)) and items = positions / 64)
    short = [c for c in G.WG_CASES if c[9][0] > 1 and (c[1] * _cdiv(c[4], 64)) % c[9][0] != 0]
    assert short and any(c[9][0] > 1 and _cdiv(c[4], 64) % c[9][0] != 0 for c in G.WG_CASES)
    assert any(c[9][0] >= 6 and _cdiv(c[4], 64) == 1 for c in G.WG_CASES) and any(c[9][0] >= 6 and _cdiv(c[4], 64) > 1 for c in G.WG_CASES)
    assert any(_reached(b)[2] for b in (16, 128))      # (the real steps do have short last splits)


def test_gpu_case_expectations_equal_the_restatement():
    """the expectation each GPU case carries is what the rule gives (the GPU test asserts it against the query again before it runs)"""
    for cid, B, Cin, Cout, K, d, pad, Lin, expect in G.CONV_CASES:
        p = plan_conv(B, Cin, Cout, K, Lin, pad, d)
        assert (p['MI'], p['NJ'], p['bucket']) == expect, (cid, p)
        assert G.conv_plan(B, Cin, Cout, K, Lin, pad, d) == p, cid
    for wid, N, A, Bc, LP, LQ, J, base, step, expect in G.WG_CASES:
        p = plan_wgrad(N, A, Bc, LP, J, step)
        assert (p['CH'], p['splits'], p['groups']) == expect, (wid, p)
        assert G.wgrad_plan(N, A, Bc, LP, J, step) == p, wid
    for N, A, Bc, LP, J, slices in G.BIAS_CASES:
        assert plan_wgrad(N, A, Bc, LP, J, 1)['bias_slices'] == slices
    for lo, hi in G.PAIRS:
        assert plan_conv(*_args(lo))['NJ'] == 1 and plan_conv(*_args(hi))['NJ'] == 2
        assert plan_conv(*_args(hi))['gx'] * plan_conv(*_args(hi))['gy'] == 512


def _args(cid):
    _, B, Cin, Cout, K, d, pad, Lin, _ = G.conv_case(cid)
    return B, Cin, Cout, K, Lin, pad, d
