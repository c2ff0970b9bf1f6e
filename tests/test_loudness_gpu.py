"""GPU: the loudness kernels (csrc/loudness.hip) against the float64 statement tests/loudness_reference.py, at the smallest shapes where they can
go wrong: row ends around CHUNK, the 100 ms sub-block, the 400 ms block and the TILE, several tiles, NaN behind every row."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import loudness_reference as R

pytestmark = pytest.mark.gpu

SR = 24000
TARGET = -16.0            # the rows read -17 LUFS or so: the two with the burst then meet the -1 dB ceiling, the others do not
# Distance of the chunked scheme from the sequential recursion in float64, measured on the CPU with the numpy emulation
# (loudness_reference.chunked_sub_energies at CHUNK = 64, TILE = 16384) on the rows below: 3.33e-13 of a row's largest sub-block energy and 3.33e-13
# of zbar (the DC offset and the step of the rows keep the high-pass state far above its output: the output is a small difference of large
# numbers, in either scheme).  The kernels get 64 times that measured figure, 2.13e-11, for contraction and order differences; anything near
# 1e-9 would be a float32 state or sum.  In dB: 10 log10(1 + 2.13e-11) = 9.3e-11.  The emulation itself is held under a rounded ceiling.
EMU_MEASURED = 3.33e-13
EMU_CEILING = 3.5e-13
BOUND = 64 * EMU_MEASURED


def _mod():
    from ttscube_amd.io_utils import loudness
    return loudness


def _lengths():
    M = _mod()
    c, t = M.CHUNK, M.TILE
    return [0, 1, c - 1, c, c + 1, 2399, 2400, 2401, 9599, 9600, 9601, t - 1, t, t + 1, 3 * t + 17]


@functools.lru_cache(maxsize=None)
def _batch():
    """-> (x [B, Lmax] float32 with NaN behind each row, lengths)"""
    M = _mod()
    lens = _lengths()
    rng = np.random.default_rng(20240611)
    Lmax = max(lens) + 6                                       # odd: the rows start at every offset from a 16-byte boundary
    x = np.full((len(lens), Lmax), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        r = 0.1 * rng.standard_normal(n) + 0.05               # noise on a DC offset
        r[n // 3:] += 0.2                                      # a step
        if n > M.TILE:                                         # a burst across the first tile edge
            r[M.TILE - 40:M.TILE + 40] += 0.5 * rng.standard_normal(80)[:n - M.TILE + 40]
        x[b, :n] = r
    return x, lens


@functools.lru_cache(maxsize=None)
def _ref():
    x, lens = _batch()
    return [R.measure(x[b, :n], SR) for b, n in enumerate(lens)]


@functools.lru_cache(maxsize=None)
def _gpu():
    M = _mod()
    x, lens = _batch()
    xd = torch.from_numpy(x).cuda()
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    m = M.LoudnessMeter('cuda:0')
    st = m.measure_device(xd, ld, SR, target=TARGET, peak_db=-1.0)
    return m, xd, ld, {k: v.cpu().numpy() for k, v in st.items()}, st


def test_emulated_scheme_is_within_its_recorded_distance():
    M = _mod()
    x, lens = _batch()
    worst_sub = worst_z = 0.0
    for b, n in enumerate(lens):
        if n == 0:
            continue
        sub, _ = R.chunked_sub_energies(x[b, :n], SR, M.CHUNK, M.TILE)
        ref = _ref()[b]
        worst_sub = max(worst_sub, np.abs(sub - ref['sub']).max() / ref['sub'].max())
        g = R.gate(R.blocks(sub, n, SR))
        assert (g['blocks'], g['gated']) == (ref['blocks'], ref['gated'])
        worst_z = max(worst_z, abs(g['zbar'] - ref['zbar']) / ref['zbar'])
    print('emulation vs recursion: sub-blocks %.3e, zbar %.3e' % (worst_sub, worst_z))
    assert max(worst_sub, worst_z) <= EMU_CEILING
    assert abs(max(worst_sub, worst_z) - EMU_MEASURED) <= 0.01 * EMU_MEASURED      # the recorded figure is the measured one
    assert BOUND < 1e-9


def test_sub_block_energies_and_zbar():
    _, _, _, st, _ = _gpu()
    _, lens = _batch()
    worst_sub = worst_z = 0.0
    for b, n in enumerate(lens):
        ref = _ref()[b]
        nsub = ref['sub'].size
        got = st['sub'][b]
        assert np.all(got[nsub:] == 0.0)
        if n == 0:
            assert st['zbar'][b] == 0.0
            continue
        worst_sub = max(worst_sub, np.abs(got[:nsub] - ref['sub']).max() / ref['sub'].max())
        worst_z = max(worst_z, abs(st['zbar'][b] - ref['zbar']) / ref['zbar'])
    print('kernels vs recursion: sub-blocks %.3e, zbar %.3e (bound %.3e)' % (worst_sub, worst_z, BOUND))
    assert worst_sub <= BOUND and worst_z <= BOUND


def test_gates_and_counts_are_the_restatements():
    _, _, _, st, _ = _gpu()
    for b, ref in enumerate(_ref()):
        assert R.gate_margin(ref['z']) > 1e-6                  # no block of these inputs sits at a threshold
        assert (st['blocks'][b], st['gated'][b], bool(st['silent'][b])) == (ref['blocks'], ref['gated'], ref['silent']), b
    assert [r['blocks'] for r in _ref()][:8] == [0, 1, 1, 1, 1, 1, 1, 1]
    assert _ref()[10]['blocks'] == 1 and _ref()[9]['blocks'] == 1 and _ref()[8]['blocks'] == 1     # 9599 < 9600 = 400 ms: short; 9600, 9601: one whole block


def test_tech3341_case4_shortened():
    M = _mod()
    x = R.tone_sequence([(-72, 1), (-36, 1), (-23, 6), (-36, 1), (-72, 1)], SR).astype(np.float32)
    ref = R.measure(x, SR)
    assert (ref['blocks'], ref['gated']) == (97, 63) and abs(ref['lufs'] - (-23.201)) < 1e-3
    assert R.gate_margin(ref['z']) > 1e-6
    m = M.LoudnessMeter('cuda:0')
    st = m.measure_device(torch.from_numpy(x[None]).cuda(), torch.tensor([x.size], dtype=torch.int32).cuda(), SR)
    assert (int(st['blocks'][0]), int(st['gated'][0]), int(st['silent'][0])) == (97, 63, 0)
    z = float(st['zbar'][0])
    assert abs(z - ref['zbar']) <= BOUND * ref['zbar']
    assert abs(float(M.lufs(z)) - ref['lufs']) < 1e-9
    assert abs(m.integrated_loudness(x, SR) - ref['lufs']) < 1e-9


def test_peaks():
    _, _, _, st, _ = _gpu()
    x, lens = _batch()
    for b, n in enumerate(lens):
        tp, bound = R.true_peak(x[b, :n])
        assert st['sample_peak'][b] == (np.abs(x[b, :n]).max() if n else 0.0)
        print('row %d: |true peak - float64| %.3e, bound %.3e' % (b, abs(float(st['true_peak'][b]) - tp), bound))
        assert abs(float(st['true_peak'][b]) - tp) <= bound, (b, st['true_peak'][b], tp, bound)


def test_gain_and_ceiling():
    m, _, _, st, dev = _gpu()
    _, lens = _batch()
    limited = 0
    for b, ref in enumerate(_ref()):
        g, lim = R.gain(ref['zbar'], max(ref['sample_peak'], ref['true_peak']), ref['silent'], TARGET, -1.0)
        assert abs(float(st['gain'][b]) - float(g)) <= 2.0 ** -23 * float(g), b
        assert bool(st['limited'][b]) == lim
        limited += lim
    assert st['gain'][0] == 1.0 and st['silent'][0] == 1
    assert 0 < limited < len(lens)                             # both branches occur
    g2, l2 = m.gains_device(dev, TARGET, peak_db=-1.0)
    assert np.array_equal(g2.cpu().numpy(), st['gain']) and np.array_equal(l2.cpu().numpy(), st['limited'])
    targets = [-30.0 + b for b in range(len(lens))]
    g3, _ = m.gains_device(dev, targets, peak_db=-6.0, max_gain_db=3.0)
    for b, ref in enumerate(_ref()):
        g, _ = R.gain(ref['zbar'], max(ref['sample_peak'], ref['true_peak']), ref['silent'], targets[b], -6.0, 3.0)
        assert abs(float(g3[b]) - float(g)) <= 2.0 ** -23 * float(g), b


def _bits(st):
    return {k: st[k].cpu().numpy().copy() for k in ('sub', 'zbar', 'sample_peak', 'true_peak', 'blocks', 'gated', 'silent')}


def test_a_row_has_the_same_bits_alone_reversed_padded_and_twice():
    M = _mod()
    m, xd, ld, st, _ = _gpu()
    x, lens = _batch()
    S = SR // 10
    again = _bits(m.measure_device(xd, ld, SR))
    for k, v in again.items():
        assert np.array_equal(v, st[k]), k
    rev = _bits(m.measure_device(xd.flip(0).contiguous(), ld.flip(0).contiguous(), SR))
    for k, v in rev.items():
        assert np.array_equal(v[::-1], st[k]), k
    pad = torch.full((len(lens), x.shape[1] + 1001), float('nan'), device='cuda')
    pad[:, :x.shape[1]] = xd
    wide = _bits(m.measure_device(pad, ld, SR))
    for k, v in wide.items():
        w = v[:, :st['sub'].shape[1]] if k == 'sub' else v
        assert np.array_equal(w, st[k]), k
    for b, n in enumerate(lens):
        one = _bits(m.measure_device(xd[b:b + 1, :max(n, 1)].contiguous(), ld[b:b + 1].contiguous(), SR))
        nsub = -(-n // S)
        assert np.array_equal(one['sub'][0, :nsub], st['sub'][b, :nsub]), b
        for k in ('zbar', 'sample_peak', 'true_peak', 'blocks', 'gated', 'silent'):
            assert one[k][0] == st[k][b], (b, k)


def test_apply():
    m, xd, ld, st, dev = _gpu()
    x, lens = _batch()
    g = dev['gain']
    want = st['gain'][:, None] * x                             # numpy's float32 product
    y = m.apply_device(xd, ld, g).cpu().numpy()
    buf = torch.full((x.size + 1,), 7.0, device='cuda')
    off = buf[1:].view(x.shape)                                # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    m.apply_device(xd, ld, g, out=off)
    inplace = xd.clone()
    assert m.apply_device(inplace, ld, g, out=inplace) is inplace
    for b, n in enumerate(lens):
        for got in (y[b], off[b].cpu().numpy(), inplace[b].cpu().numpy()):
            assert np.array_equal(got[:n].view(np.uint32), want[b, :n].view(np.uint32)), b
        assert np.all(y[b, n:] == 0.0) and np.all(off[b, n:].cpu().numpy() == 7.0) and np.all(np.isnan(inplace[b, n:].cpu().numpy()))
    assert float(buf[0]) == 7.0


def test_another_rate_48k_sine():
    M = _mod()
    n = M.TILE + 1
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(n) / 48000.0).astype(np.float32)
    m = M.LoudnessMeter('cuda:0')
    got = m.integrated_loudness(x, 48000)
    ref = R.measure(x, 48000)
    print('48 kHz, %d samples of a 997 Hz sine: %.5f LUFS (restatement %.5f)' % (n, got, ref['lufs']))
    assert abs(got - ref['lufs']) < 1e-9
    assert abs(got - (-3.01)) <= 0.005


def test_refused_arguments_leave_the_outputs_untouched():
    from ttscube_amd import _lib
    M = _mod()
    L = _lib.lib()
    B, Lmax = 2, 5000
    x = torch.zeros((B, Lmax), device='cuda')
    ld = torch.tensor([Lmax, 10], dtype=torch.int32).cuda()
    nsub = -(-Lmax // 2400)
    sub = torch.full((B, nsub), 3.0, dtype=torch.float64, device='cuda')
    sp, tp = torch.full((B,), 3.0, device='cuda'), torch.full((B,), 3.0, device='cuda')
    ws = torch.zeros(4096, dtype=torch.float64, device='cuda')
    k, taps = M.kernel_constants(SR), np.ascontiguousarray(M.true_peak_taps())
    p = lambda t: C.c_void_p(t.data_ptr())
    kp, tpp = k.ctypes.data_as(C.c_void_p), taps.ctypes.data_as(C.c_void_p)

    def call(sr=SR, b=B, n=nsub, wsb=ws.numel() * 8):
        return L.ttsc_loudness_measure(p(x), p(ld), b, Lmax, sr, kp, tpp, p(sub), n, p(sp), p(tp), p(ws), wsb, _lib.current_stream())
    assert call(sr=22055) != 0 and b'multiple of 10' in L.ttsc_last_error()
    assert call(sr=630) != 0                                   # sr / 10 < CHUNK
    assert call(b=0) != 0 and call(n=nsub - 1) != 0 and call(wsb=8) != 0
    zb = torch.full((B,), 3.0, dtype=torch.float64, device='cuda')
    cnt = [torch.full((B,), 3, dtype=torch.int32, device='cuda') for _ in range(3)]
    assert L.ttsc_loudness_finish(p(sub), p(ld), B, Lmax, nsub, 22055, p(sp), p(tp), M.ABS_GATE, None, None, 0.0, p(zb), p(cnt[0]), p(cnt[1]),
                                  p(cnt[2]), None, None, _lib.current_stream()) != 0
    y = torch.full((B, Lmax), 3.0, device='cuda')
    assert L.ttsc_loudness_apply(p(x), p(ld), p(sp), 0, Lmax, p(y), _lib.current_stream()) != 0
    assert L.ttsc_loudness_apply(p(x), p(ld), None, B, Lmax, p(y), _lib.current_stream()) != 0
    torch.cuda.synchronize()
    for t in [sub, sp, tp, zb, y] + cnt:
        assert bool((t == 3).all())
    m = M.LoudnessMeter('cuda:0')
    for sr in (22055, 630, 0):
        with pytest.raises(ValueError):
            m.measure_device(x, ld, sr)
    assert call() == 0                                         # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((sp == 0).all())
