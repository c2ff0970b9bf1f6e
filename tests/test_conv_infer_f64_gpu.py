"""Every tile variant of the inference convolutions against float64 (tests/conv_reference.py), at the lengths around its tile seams.

Three assertions per variant:
 (a) on inputs whose right answer has no rounding (tests/test_conv_reference_cpu.py proves that of the reference alone) the kernel equals
     float64 bit for bit: a misplaced tap, halo column, phase row, seam or channel chunk cannot hide behind rounding;
 (b) on N(0,1) data the element-wise bound  |y - ref64| <= (n + 16) 2^-24 A + 2^-24 W  derived in DESIGN.md;
 (c) on the same data, max and RMS error at most 4 x those of the sequential float32 restatement.
The general kernels' tiles are forced with TTSC_CONV_TILE (a tile the layer cannot take is an error, so the variant named is the variant run),
the wide and tall kernels with TTSC_CONV_WIDE=2, the chain kernels by their own rule (shape = -1) with and without TTSC_CHAIN_IL=0.
Each test prints 'RATIO <variant> <case> <max ratio> <rms ratio>' for (c); DESIGN.md holds the table of their maxima."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import conv_reference as R

pytestmark = pytest.mark.gpu

YARD = 4.0        # the project's convention for a float32 restatement as the yardstick (pitch, cepstra)
CANARY = 7.0


def _conv(cin, cout, k, kw, prec):
    from ttscube_amd.hip_layers import Conv1dHip
    return Conv1dHip(cin, cout, k, stride=kw.get('stride', 1), padding=kw['padding'], dilation=kw.get('dilation', 1),
                     transposed=kw.get('transposed', False)).set_precision(prec)


def _layer_of(c, prec):
    w = c['w']
    tr = c['kw'].get('transposed', False)
    cin, cout = (w.shape[0], w.shape[1]) if tr else (w.shape[1], w.shape[0])
    conv = _conv(cin, cout, w.shape[2], c['kw'], prec)
    conv.set_weight(w, c['b'])
    return conv


def _run(conv, c):
    kw = c['kw']
    out = c['acc0'].clone().cuda() if c['acc0'] is not None else None
    y = conv(c['x'].cuda(), resid=c['resid'].cuda() if c['resid'] is not None else None, out=out, in_scale=kw.get('in_scale', 1.0),
             in_slope=kw.get('in_slope', 1.0), out_scale=c.get('out_scale', 1.0), act=c.get('act'), accumulate=out is not None)
    return y.cpu()


def _planned(conv, c):
    """{(kernel family, tile rows, tile columns)} over the phases of the launch _run(conv, c) makes, from ttsc_conv1d_plan — the selection the
    launcher itself calls, under the environment as it is now"""
    from ttscube_amd import _lib
    from ttscube_amd.hip_layers import ACT
    kw = c['kw']
    ep = _lib.Conv1dEpilogue(kw.get('in_scale', 1.0), kw.get('in_slope', 1.0), c.get('out_scale', 1.0), ACT[c.get('act')], int(c['acc0'] is not None), None, 1.0)
    B, _, L = c['x'].shape
    g = conv.cfg
    info = (C.c_int32 * 10)()
    out = set()
    for ph in range(g.stride if g.transposed and g.out_channels % 32 else 1):
        fam = _lib.lib().ttsc_conv1d_plan(conv._h, B, L, C.byref(ep), ph, info)
        assert fam >= 0, _lib.lib().ttsc_last_error()
        out.add((fam, info[0], info[1]))
    return out - {(R.PATH_NONE, 0, 0)}


def _ref64(c):
    return R.conv_f64(c['x'], c['w'], c['b'], resid=c['resid'], acc0=c['acc0'], out_scale=c.get('out_scale', 1.0), act=c.get('act'), **c['kw'])


def _check_exact(conv, c, what):
    y = _run(conv, c)
    ref = _ref64(c)
    assert y.shape == ref.shape, what
    bad = (y.double() != ref)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist(), float((y.double() - ref).abs().max()))


def _check_random(variant, conv, cin, cout, k, L, bound=True, **kw):
    """(b) and (c) on one cached random case"""
    c, ref, yard, A, W = R.cached_random(cin, cout, k, L, **kw)
    y = _run(conv, c)
    assert y.shape == ref.shape
    err = (y.double() - ref).abs()
    if bound:
        n = R.n_terms(cin, k, kw.get('stride', 1), kw.get('transposed', False), True, c['resid'] is not None, c['acc0'] is not None)
        lim = R.derived_bound(n, A, W, kw.get('out_scale', 1.0))
        assert bool((err <= lim).all()), (variant, L, 'derived bound', float((err / lim).max()))
    _check_yardstick(variant, (cin, cout, k, L, tuple(sorted(kw.items()))), y, yard, ref)
    return y


def _check_yardstick(variant, case, y, yard, ref, measure_only=False):
    km, kr = R.err_stats(y, ref)
    ym, yr = R.err_stats(yard, ref)
    print('RATIO %s %s max %.3f rms %.3f (kernel %.3e / %.3e, yardstick %.3e / %.3e)' % (variant, case, km / ym, kr / yr, km, kr, ym, yr))
    assert measure_only or (km <= YARD * ym and kr <= YARD * yr), (variant, case, km / ym, kr / yr)


def _layer_kw(layer, transposed):
    cin, cout, k, ds = layer
    return dict(stride=ds, transposed=True) if transposed else dict(dilation=ds)


# ---- the general split kernel and the fp32 kernel, every tile ---------------------------------------------------------------------------------

_GENERAL = {'f16x3': R.PATH_F16X3, 'fp32': R.PATH_FP32}

def _general_params():
    out = []
    for prec in ('f16x3', 'fp32'):
        for layer, tr, tile, lengths in R.general_variants(prec):
            out.append(pytest.param(prec, layer, tr, tile, lengths, id='%s-%s%s-%dx%d' % (prec, 'T' if tr else 'C', '_'.join(map(str, layer)), tile[0], tile[1])))
    return out


@pytest.mark.parametrize('prec,layer,transposed,tile,lengths', _general_params())
def test_general_kernel_tile(prec, layer, transposed, tile, lengths, monkeypatch):
    monkeypatch.setenv('TTSC_CONV_TILE', '%dx%d' % tile)
    cin, cout, k, ds = layer
    variant = '%s-%dx%d%s' % (prec, tile[0], tile[1], '-transposed' if transposed else '')
    conv = None
    planned = {(_GENERAL[prec],) + tile}
    for L in lengths:
        c = R.general_exact(layer, transposed, L)
        conv = conv or _layer_of(c, prec)
        assert _planned(conv, c) == planned, (variant, layer, L)
        _check_exact(conv, c, (variant, layer, L))
    kw = dict(in_slope=0.1, **_layer_kw(layer, transposed))
    conv = _layer_of(R.cached_random(cin, cout, k, lengths[0], **kw)[0], prec)   # (the weights of a layer do not depend on L)
    for L in lengths:
        assert _planned(conv, R.cached_random(cin, cout, k, L, **kw)[0]) == planned, (variant, layer, L)
        _check_random(variant, conv, cin, cout, k, L, **kw)


def _ragged(conv, x, lens, Lout_lens, cout, ep):
    from ttscube_amd import _lib
    B, _, L = x.shape
    Lo = conv.out_len(L)
    y = torch.full((B, cout, Lo), CANARY, device='cuda')
    xd = x.cuda()
    il = torch.tensor(lens, dtype=torch.int32).cuda()
    ol = torch.tensor(Lout_lens, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().ttsc_conv1d_forward_ragged(conv._h, _lib.dev_ptr(xd), B, L, _lib.dev_ptr(y), None, C.byref(ep), _lib.dev_ptr(il),
                                                     _lib.dev_ptr(ol), _lib.current_stream()), 'ragged')
    return y.cpu()


def _check_ragged_conv(conv, c, lens, nt, what):
    """a stride-1 'same' layer on a ragged batch: every utterance equals itself run alone (float64 of it, on exact data), and the tail follows
    the rule the kernels implement — a column tile that holds valid positions is stored whole, computed from the utterance's input read as
    zero beyond its length (the dense call on the zero-extended input, bit for bit); tiles wholly beyond the length are skipped and keep what
    the buffer held."""
    from ttscube_amd import _lib
    kw = c['kw']
    x = c['x']
    B, _, L = x.shape
    cout = c['w'].shape[0]
    ep = _lib.Conv1dEpilogue(kw.get('in_scale', 1.0), kw.get('in_slope', 1.0), 1.0, _lib.ACT_NONE, 0, None, 1.0)
    y = _ragged(conv, x, lens, lens, cout, ep)
    xz = x.clone()
    for i, n in enumerate(lens):
        xz[i, :, n:] = 0
    dense = conv(xz.cuda(), in_scale=kw.get('in_scale', 1.0), in_slope=kw.get('in_slope', 1.0)).cpu()
    solo = R.conv_f64_ragged(x, lens, c['w'], c['b'], **kw)
    for i, n in enumerate(lens):
        alone = conv(x[i:i + 1, :, :n].contiguous().cuda(), in_scale=kw.get('in_scale', 1.0), in_slope=kw.get('in_slope', 1.0)).cpu()
        assert torch.equal(y[i:i + 1, :, :n], alone), (what, i, 'ragged != the utterance alone')
        if c.get('exact'):
            assert torch.equal(y[i:i + 1, :, :n].double(), solo[i]), (what, i, 'ragged != float64')
        end = min(L, -(-n // nt) * nt)
        assert torch.equal(y[i, :, n:end], dense[i, :, n:end]), (what, i, 'tail inside the last tile')
        assert bool((y[i, :, end:] == CANARY).all()), (what, i, 'tail beyond the last tile was written')


@pytest.mark.parametrize('prec', ['f16x3', 'fp32'])
def test_general_kernel_ragged_and_tails(prec, monkeypatch):
    for layer in ((32, 32, 11, 5), (80, 128, 7, 1), (64, 64, 7, 3)):
        for tile in R.tiles_of(prec, R.mt_class(layer[1])):
            monkeypatch.setenv('TTSC_CONV_TILE', '%dx%d' % tile)
            nt = tile[1]
            c = dict(R.general_exact(layer, False, nt + 1), resid=None, acc0=None, exact=True)
            conv = _layer_of(c, prec)
            assert _planned(conv, c) == {(_GENERAL[prec],) + tile}, (prec, layer, tile)
            _check_ragged_conv(conv, c, [nt + 1, 7], nt, (prec, layer, tile, 'exact'))
            c = R.cached_random(layer[0], layer[1], layer[2], nt + 1, in_slope=0.1, dilation=layer[3])[0]
            conv = _layer_of(c, prec)
            assert _planned(conv, c) == {(_GENERAL[prec],) + tile}, (prec, layer, tile)
            _check_ragged_conv(conv, c, [nt + 1, 7], nt, (prec, layer, tile, 'random'))


def test_forced_tile_the_layer_cannot_take_is_an_error(monkeypatch):
    from ttscube_amd._lib import TTSCError
    x32 = torch.zeros(1, 32, 40).cuda()
    x80 = torch.zeros(1, 80, 40).cuda()
    for prec in ('f16x3', 'fp32'):
        c32 = _conv(32, 32, 3, dict(padding=1), prec)
        c32.set_weight(torch.zeros(32, 32, 3))
        c128 = _conv(80, 128, 7, dict(padding=3), prec)
        c128.set_weight(torch.zeros(128, 80, 7))
        for conv, x, bad in ((c32, x32, ('64x256', '64x128', '128x128', '32x64', '32x1024')), (c128, x80, ('32x512', '32x256', '128x256', '16x128'))):
            for t in bad:
                monkeypatch.setenv('TTSC_CONV_TILE', t)
                with pytest.raises(TTSCError, match='TTSC_CONV_TILE'):
                    conv(x)
            for t in ('64', 'x', '64x', '64x256x2', 'big'):
                monkeypatch.setenv('TTSC_CONV_TILE', t)
                with pytest.raises(TTSCError, match='TTSC_CONV_TILE'):
                    conv(x)
            for t in R.tiles_of(prec, R.mt_class(conv.cfg.out_channels)):
                monkeypatch.setenv('TTSC_CONV_TILE', '%dx%d' % t)
                assert bool((conv(x) == 0).all())
    # each precision has tiles the other lacks: 64x64 is fp32 only, 32x128 at 128 rows split only
    c128 = _conv(80, 128, 7, dict(padding=3), 'f16x3')
    c128.set_weight(torch.zeros(128, 80, 7))
    monkeypatch.setenv('TTSC_CONV_TILE', '64x64')
    with pytest.raises(TTSCError, match='TTSC_CONV_TILE'):
        c128(x80)
    c128.set_precision('fp32')
    monkeypatch.setenv('TTSC_CONV_TILE', '32x128')
    with pytest.raises(TTSCError, match='TTSC_CONV_TILE'):
        c128(x80)


# ---- wide, tall and single-output-channel kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C_,k,d,L', R.WIDE_CASES)
def test_wide_kernel(C_, k, d, L, monkeypatch):
    monkeypatch.setenv('TTSC_CONV_WIDE', '2')
    monkeypatch.setenv('TTSC_CONV_TILE', '32x512')   # not a tile of this layer: the wide kernel does not read the switch
    variant = 'wide-%d' % C_
    c = R.exact_case(C_, C_, k, L, dilation=d, in_slope=0.5)
    conv = _layer_of(c, 'f16x3')
    assert _planned(conv, c) == {(R.PATH_WIDE, 128, 256)}
    _check_exact(conv, c, (variant, k, d, L, 'plain'))
    c = R.exact_case(C_, C_, k, L, dilation=d, resid=True, acc0=True, in_scale=0.5, in_slope=0.25)
    assert _planned(conv, c) == {(R.PATH_WIDE, 128, 256)}
    _check_exact(conv, c, (variant, k, d, L, 'acc_init'))
    if L in (5, 257):   # (one full length per (C, K, d) pays for the yardstick: about a second at 256 channels with K = 11)
        conv = _layer_of(R.cached_random(C_, C_, k, L, dilation=d, in_slope=0.1)[0], 'f16x3')
        _check_random(variant, conv, C_, C_, k, L, dilation=d, in_slope=0.1)
        if d != 1:
            # residual + running sum + bias are the INITIAL value of this layer's accumulators: the yardstick is the float32 sum in that order
            # (DESIGN.md derives why the plain order, whose ratio is printed beside it, is no fair yardstick here); the element-wise bound is
            # order-free and holds as it stands
            kw = dict(dilation=d, resid=True, acc0=True, in_scale=1.0 / 3.0, in_slope=0.1)
            y = _check_random(variant + '-acc_init', conv, C_, C_, k, L, init_first=True, **kw)
            _, ref, yard, _, _ = R.cached_random(C_, C_, k, L, **kw)
            _check_yardstick(variant + '-acc_init-vs-plain-order', (C_, k, d, L), y, yard, ref, measure_only=True)


@pytest.mark.parametrize('C_', [128, 256])
def test_wide_kernel_ragged_tails(C_, monkeypatch):
    monkeypatch.setenv('TTSC_CONV_WIDE', '2')
    c = dict(R.exact_case(C_, C_, 7, 257, dilation=3, in_slope=0.5), exact=True)
    _check_ragged_conv(_layer_of(c, 'f16x3'), c, [257, 7], 256, ('wide', C_, 'exact'))
    c = dict(R.exact_case(C_, C_, 3, 513, dilation=5, in_slope=0.5), exact=True)
    _check_ragged_conv(_layer_of(c, 'f16x3'), c, [255, 513], 256, ('wide', C_, 'exact, short first'))


@pytest.mark.parametrize('C_,k', [(C_, k) for C_ in (128, 256) for k in (3, 7, 11)])
def test_batch_size_never_changes_a_bit_on_the_wide_layers(C_, k, monkeypatch):
    """docs/KERNELS.md: on the layers the wide kernel may take, the fill rule (wide kernel or any tile of the general split kernel, which mirrors
    its arithmetic) never changes a bit — plain and with residual + running sum + in_scale as the accumulators' initial value"""
    d, L = {3: 5, 7: 3, 11: 1}[k], 257
    for extra in (dict(in_slope=0.1), dict(resid=True, acc0=True, in_scale=1.0 / 3.0, in_slope=0.1)):
        c = R.cached_random(C_, C_, k, L, dilation=d, **extra)[0]
        conv = _layer_of(c, 'f16x3')
        monkeypatch.setenv('TTSC_CONV_WIDE', '2')
        monkeypatch.delenv('TTSC_CONV_TILE', raising=False)
        assert _planned(conv, c) == {(R.PATH_WIDE, 128, 256)}
        wide = _run(conv, c)
        monkeypatch.setenv('TTSC_CONV_WIDE', '1')   # the default: a problem this small goes to the general kernel
        assert _planned(conv, c) == {(R.PATH_F16X3, 32, 128)}   # (and to its smallest tile: 8 and 16 workgroups of the larger ones)
        for tile in R.tiles_of('f16x3', R.mt_class(C_)):
            monkeypatch.setenv('TTSC_CONV_TILE', '%dx%d' % tile)
            assert _planned(conv, c) == {(R.PATH_F16X3,) + tile}
            y = _run(conv, c)
            assert torch.equal(y, wide), (C_, k, tile, sorted(extra), float((y - wide).abs().max()))


@pytest.mark.parametrize('prec', ['f16x3', 'fp32'])
def test_tiles_of_the_general_kernels_agree_bit_for_bit(prec, monkeypatch):
    """the other general-kernel layers and the fp32 tiles: every tile accumulates a given output in the same order (16-channel chunks, taps inside a
    chunk), so the fill rule — and with it the batch size — does not change a bit there either"""
    for layer, tr in [(l, False) for l in R.GENERAL_CONV[:4]] + [(l, True) for l in R.GENERAL_TRANS]:
        cin, cout, k, ds = layer
        L = 257
        c = R.cached_random(cin, cout, k, L, in_slope=0.1, **_layer_kw(layer, tr))[0]
        conv = _layer_of(c, prec)
        outs = []
        for tile in R.tiles_of(prec, R.mt_class(cout, ds, tr)):
            monkeypatch.setenv('TTSC_CONV_TILE', '%dx%d' % tile)
            outs.append((tile, _run(conv, c)))
        for tile, y in outs[1:]:
            print('TILES', prec, layer, tr, outs[0][0], tile, 'max diff %.3e' % float((y - outs[0][1]).abs().max()))
        for tile, y in outs[1:]:
            assert torch.equal(y, outs[0][1]), (prec, layer, tr, outs[0][0], tile, float((y - outs[0][1]).abs().max()))


@pytest.mark.parametrize('cin,cout,k,s,L', R.TALL_CASES)
def test_tall_kernel(cin, cout, k, s, L, monkeypatch):
    monkeypatch.setenv('TTSC_CONV_WIDE', '2')
    monkeypatch.setenv('TTSC_CONV_TILE', '32x512')   # not a tile of this layer: the tall kernel does not read the switch
    c = R.exact_case(cin, cout, k, L, stride=s, transposed=True, in_slope=0.25)
    conv = _layer_of(c, 'f16x3')
    assert _planned(conv, c) == {(R.PATH_TALL,) + ((256, 128) if cin == 512 else (128, 256))}
    _check_exact(conv, c, ('tall', cin, L))           # the whole output: every phase
    conv = _layer_of(R.cached_random(cin, cout, k, L, stride=s, transposed=True, in_slope=0.1)[0], 'f16x3')
    _check_random('tall-%d' % cin, conv, cin, cout, k, L, stride=s, transposed=True, in_slope=0.1)


@pytest.mark.parametrize('prec', ['f16x3', 'fp32'])
@pytest.mark.parametrize('cin,L', R.COUT1_CASES)
def test_cout1_kernel(cin, L, prec):
    c = R.exact_case(cin, 1, 7, L, resid=True, acc0=True, in_scale=0.5, in_slope=0.25)
    conv = _layer_of(c, prec)
    assert _planned(conv, c) == {(R.PATH_COUT1, 1, 1024)}
    _check_exact(conv, c, ('cout1', cin, L))
    kw = dict(resid=True, acc0=True, in_slope=0.01)
    conv = _layer_of(R.cached_random(cin, 1, 7, L, **kw)[0], prec)
    _check_random('cout1', conv, cin, 1, 7, L, **kw)
    _check_random('cout1-tanh', conv, cin, 1, 7, L, bound=False, in_scale=1.0 / 3.0, out_scale=0.5, act='tanh', **kw)   # (tanh: yardstick only)
    if L == 1025:
        # tiles of 1024 positions: the second utterance ends inside the first tile
        c = dict(R.exact_case(cin, 1, 7, L, in_slope=0.5), exact=True)
        _check_ragged_conv(_layer_of(c, prec), c, [1025, 7], 1024, ('cout1', cin))


# ---- ResBlock chain kernels ---------------------------------------------------------------------------------------------------------------------

def _chain_handles(layers, C_, k):
    from ttscube_amd.hip_layers import Conv1dHip
    c1s, c2s = [], []
    for w1, b1, w2, b2, d in layers:
        c1 = Conv1dHip(C_, C_, k, padding=d * (k - 1) // 2, dilation=d).set_precision('f16x3')
        c2 = Conv1dHip(C_, C_, k, padding=(k - 1) // 2).set_precision('f16x3')
        c1.set_weight(w1, b1)
        c2.set_weight(w2, b2)
        c1s.append(c1)
        c2s.append(c2)
    return c1s, c2s


def _chain_call(c1s, c2s, xd, y, accumulate, lens=None, shape=-1):
    from ttscube_amd import _lib
    n = len(c1s)
    a1 = (C.c_void_p * n)(*[c._h for c in c1s])
    a2 = (C.c_void_p * n)(*[c._h for c in c2s])
    L_ = _lib.lib()
    assert L_.ttsc_rbchain_supported(a1, a2, n) == 1
    B, _, L = xd.shape
    _lib.check(L_.ttsc_rbchain_forward(a1, a2, n, _lib.dev_ptr(xd), B, L, _lib.dev_ptr(y), accumulate,
                                       _lib.dev_ptr(lens) if lens is not None else None, shape, _lib.current_stream()), 'ttsc_rbchain_forward')


def _assert_same(y, ref, what):
    bad = y.double() != ref
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist(), float((y.double() - ref).abs().max()))


@pytest.mark.parametrize('il', ['1', '0'])
@pytest.mark.parametrize('C_,k', R.CHAIN_CONFIGS)
def test_chain_kernel_production_instantiations(C_, k, il, monkeypatch):
    """shape = -1, as the generator calls it: (32, k7) is the plain small tile, (32, k11) the interleaved large tile with 6-step groups, 64 channels
    with K = 7 / 11 the large tile; TTSC_CHAIN_IL=0 gives the plain small and large tiles at every channel count"""
    monkeypatch.setenv('TTSC_CHAIN_IL', il)
    large, ncol, halo, nto, interleaved = R.chain_geometry(C_, k, interleaved=il == '1')
    variant = 'chain-%d-k%d-%s%s' % (C_, k, 'large' if large else 'small', '-il' if interleaved else '')
    lengths = R.chain_lengths(nto)
    assert any(L % 4 for L in lengths) and any(L % 4 == 0 for L in lengths)
    c1s = c2s = None
    for L in lengths:
        c = R.exact_chain_case(C_, k, R.CHAIN_DILS, L)
        if c1s is None:
            c1s, c2s = _chain_handles(c['layers'], C_, k)   # (the weights do not depend on L: the generator draws them first)
        ref = R.chain_f64(c['x'], c['layers'], k)[0]
        xd = c['x'].cuda()
        for accumulate in (0, 1):
            y = c['acc0'].clone().cuda()
            _chain_call(c1s, c2s, xd, y, accumulate)
            _assert_same(y.cpu(), ref + c['acc0'].double() if accumulate else ref, (variant, L, accumulate))
    # ragged, exact data: the short utterance ends one column either side of the first tile seam, at lengths that are no multiple of the vector width
    L = 2 * nto + 1
    c = R.exact_chain_case(C_, k, R.CHAIN_DILS, L)
    xd = c['x'].cuda()
    for n in (nto - 1, nto + 1):
        assert n % 4
        lens = [n, L]
        y = torch.full_like(xd, CANARY)
        _chain_call(c1s, c2s, xd, y, 0, torch.tensor(lens, dtype=torch.int32).cuda())
        y = y.cpu()
        for i, ref in enumerate(R.chain_f64_ragged(c['x'], lens, c['layers'], k)):
            _assert_same(y[i:i + 1, :, :lens[i]], ref, (variant, 'ragged', n, i))
            assert bool((y[i, :, lens[i]:] == CANARY).all()), (variant, 'the tail was written', n, i)
    # random data: yardstick only (the kernel's input of the inner layers is not known to the test)
    layers = R.random_chain_layers(C_, k, R.CHAIN_DILS, seed=100 * k + C_)
    r1, r2 = _chain_handles(layers, C_, k)
    for L in (nto + 1, 2 * nto + 1):
        x, s0 = R._mk((2, C_, L), 5), R._mk((2, C_, L), 6)
        ref = R.chain_f64(x, layers, k)[0] + s0.double()
        yard = (R.chain_f32_sequential(x, layers, k) + s0)
        y = s0.clone().cuda()
        _chain_call(r1, r2, x.cuda(), y, 1)
        _check_yardstick(variant, L, y.cpu(), yard, ref)


@pytest.mark.parametrize('k', [7, 11])
def test_chain_split_into_two_launches(k):
    """the generator's cut chains at 64 channels (1 + 2 pairs for K = 7, 2 + 1 for K = 11, through a workspace): float64 bit for bit on exact data"""
    C_ = 64
    nf = 2 if k == 11 else 1
    # the first launch's own tile
    nto = R.chain_geometry(C_, k, R.CHAIN_DILS[:nf])[3]
    L = nto + 1
    c = R.exact_chain_case(C_, k, R.CHAIN_DILS, L)
    c1s, c2s = _chain_handles(c['layers'], C_, k)
    ref = R.chain_f64(c['x'], c['layers'], k)[0]
    xd = c['x'].cuda()
    for accumulate in (0, 1):
        ws = torch.full_like(xd, CANARY)
        y = c['acc0'].clone().cuda()
        _chain_call(c1s[:nf], c2s[:nf], xd, ws, 0)
        _chain_call(c1s[nf:], c2s[nf:], ws, y, accumulate)
        _assert_same(y.cpu(), ref + c['acc0'].double() if accumulate else ref, ('split chain', k, accumulate))
    layers = R.random_chain_layers(C_, k, R.CHAIN_DILS, seed=7)
    r1, r2 = _chain_handles(layers, C_, k)
    x = R._mk((2, C_, L), 5)
    ws, y = torch.empty(2, C_, L, device='cuda'), torch.empty(2, C_, L, device='cuda')
    _chain_call(r1[:nf], r2[:nf], x.cuda(), ws, 0)
    _chain_call(r1[nf:], r2[nf:], ws, y, 0)
    _check_yardstick('chain-split-64-k%d' % k, L, y.cpu(), R.chain_f32_sequential(x, layers, k), R.chain_f64(x, layers, k)[0])


@pytest.mark.parametrize('k', [3, 11])
def test_chain_with_fused_conv_post(k):
    """ttsc_rbchain_post_forward ends in tanh: yardstick only.  Its tile: 1024 interleaved columns, halo + conv_post's 3 columns rounded up to the
    vector width"""
    from ttscube_amd import _lib
    C_ = 32
    halo = (sum((d + 1) * (k - 1) // 2 for d in R.CHAIN_DILS) + 3 + 3) // 4 * 4
    nto = (1024 - 2 * halo) & ~31
    layers = R.random_chain_layers(C_, k, R.CHAIN_DILS, seed=3 * k)
    c1s, c2s = _chain_handles(layers, C_, k)
    pw, pb = R._mk((1, C_, 7), 91, 1.0 / (C_ * 7) ** 0.5), R._mk((1,), 92, 0.1)
    post = _conv(C_, 1, 7, dict(padding=3), 'f16x3')
    post.set_weight(pw, pb)
    n = len(c1s)
    a1 = (C.c_void_p * n)(*[c._h for c in c1s])
    a2 = (C.c_void_p * n)(*[c._h for c in c2s])
    L_ = _lib.lib()
    assert L_.ttsc_rbchain_post_supported(a1, a2, n, post._h) == 1
    pkw = dict(in_scale=1.0 / 3.0, in_slope=0.01, out_scale=1.0, act='tanh')
    ep = _lib.Conv1dEpilogue(pkw['in_scale'], pkw['in_slope'], 1.0, _lib.ACT_TANH, 0, None, 1.0)
    for L in (nto - 4, nto, nto + 4, 2 * nto + 4):
        x, ysum = R._mk((2, C_, L), 5), R._mk((2, C_, L), 6)
        ref = R.chain_f64(x, layers, k, post=(pw, pb), post_kw=pkw, ysum=ysum)[0]
        yard = R.chain_f32_sequential(x, layers, k, post=(pw, pb), post_kw=pkw, ysum=ysum)
        xd, yd = x.cuda(), ysum.cuda()
        wav = torch.full((2, 1, L), CANARY, device='cuda')
        _lib.check(L_.ttsc_rbchain_post_forward(a1, a2, n, _lib.dev_ptr(xd), 2, L, _lib.dev_ptr(yd), post._h, C.byref(ep), _lib.dev_ptr(wav), None,
                                                _lib.current_stream()), 'ttsc_rbchain_post_forward')
        _check_yardstick('chain-post-32-k%d' % k, L, wav.cpu(), yard, ref)


# ---- the whole generator ------------------------------------------------------------------------------------------------------------------------

def _generator(h, sd, precision):
    from ttscube_amd.hifigan.env import AttrDict
    from ttscube_amd.hifigan.models import Generator
    g = Generator(AttrDict(h))
    g.load_state_dict(sd, strict=True)
    if precision:
        g.set_precision(precision)
    return g.cuda().eval()


def _check_generator(variant, h, sd, mels, precisions):
    from oracle import hifigan_ref as O
    w = O.fold_state_dict(sd)
    w64 = {k_: v.double() for k_, v in w.items()}
    refs = [(m, O.generator_forward(w64, h, m.double()), O.generator_forward(w, h, m)) for m in mels]
    for precision in precisions:
        g = _generator(h, sd, precision)
        for mel, ref, yard in refs:
            with torch.no_grad():
                out = g(mel.cuda()).cpu()
            assert out.shape == ref.shape
            _check_yardstick('%s-%s' % (variant, precision or 'default'), tuple(mel.shape), out, yard, ref)


def test_generator_golden_config_against_float64(golden_dir):
    z = np.load(os.path.join(golden_dir, 'hifigan_c32_r3544.npz'))
    h = json.loads(str(z['cfg_json']))
    sd = {k_[3:]: torch.from_numpy(z[k_]) for k_ in z.files if k_.startswith('sd/')}
    mels = [torch.from_numpy(z['mel/%d' % T]) for T in sorted(int(k_[4:]) for k_ in z.files if k_.startswith('mel/'))]
    _check_generator('generator-c32', h, sd, mels, ('f16x3', 'fp32'))


def test_generator_full_v1_against_float64():
    from oracle import hifigan_ref as O
    h = dict(O.CONFIG_V1)
    sd = O.synthetic_state_dict(h, seed=21)
    _check_generator('generator-v1', h, sd, [O.synthetic_mel(2, 20, seed=22)], ('f16x3', 'fp32'))
