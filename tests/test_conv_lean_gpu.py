"""GPU: the lean variants of conv_f16x3_wide_kernel / conv_f16x3_tall_kernel (staging loads through a buffer descriptor with hardware zero padding,
zero taps of the transposed phases skipped) against the kernels as they were (TTSC_CONV_LEAN=0, bit for bit) and against torch.

Shapes are the smallest at which each mechanism can go wrong: inputs shorter than the tap count, one partial tile, a second tile of one position,
windows wider than the data on both sides, ragged batches, and an input that starts one float into a larger allocation."""
import ctypes as C_

import pytest
import torch
import torch.nn.functional as F

from tests.test_conv1d_gpu import F16X3_TOL, _mk

pytestmark = pytest.mark.gpu


def _both(monkeypatch, fn):
    """fn() with the lean kernels (default) and with TTSC_CONV_LEAN=0 (the switch is read at every launch)"""
    monkeypatch.setenv('TTSC_CONV_WIDE', '2')   # force the wide / tall kernels for problems too small to pick them by themselves
    monkeypatch.delenv('TTSC_CONV_LEAN', raising=False)
    lean = fn()
    monkeypatch.setenv('TTSC_CONV_LEAN', '0')
    plain = fn()
    monkeypatch.delenv('TTSC_CONV_LEAN', raising=False)
    return lean, plain


def _ragged(conv, xd, lens_in, lens_out, Lout):
    from ttscube_amd import _lib
    B, _, L = xd.shape
    y = torch.zeros(B, conv.cfg.out_channels, Lout, device='cuda')
    il = torch.tensor(lens_in, dtype=torch.int32).cuda()
    ol = torch.tensor(lens_out, dtype=torch.int32).cuda()
    ep = _lib.Conv1dEpilogue(1.0, 0.1, 1.0, _lib.ACT_NONE, 0, None, 1.0)
    _lib.check(_lib.lib().ttsc_conv1d_forward_ragged(conv._h, _lib.dev_ptr(xd), B, L, _lib.dev_ptr(y), None, C_.byref(ep), _lib.dev_ptr(il),
                                                     _lib.dev_ptr(ol), _lib.current_stream()), 'ragged')
    return y


@pytest.mark.parametrize('cin,cout,k,s,pad,L,B,lens', [
    (512, 256, 16, 5, 5, 3, 1, None),            # shorter than J = 4
    (512, 256, 16, 5, 5, 37, 1, None),           # one partial tile
    (512, 256, 16, 5, 5, 129, 2, None),          # the second tile holds one position: the taps reach across the tile edge
    (512, 256, 16, 5, 5, 300, 2, [223, 300]),    # ragged
    (256, 128, 16, 3, 6, 5, 1, None),            # shorter than J = 6
    (256, 128, 16, 3, 6, 259, 1, None),          # one tile plus three positions
    (256, 128, 16, 3, 6, 600, 2, [523, 600]),    # ragged
])
def test_tall_kernel_lean_keeps_the_bits(cin, cout, k, s, pad, L, B, lens, monkeypatch):
    """ups.0 / ups.1 of HiFi-GAN V1: the row tiles of phases 1.. run J - 1 taps per chunk.  The WHOLE output is compared, i.e. the samples of every
    phase: a skipped real tap or a weight-slot parity slip shows in 4 of 5 (2 of 3) samples."""
    from ttscube_amd.hip_layers import Conv1dHip
    w = _mk((cin, cout, k), 11, 1.0 / (cin * k / s) ** 0.5)
    b = _mk((cout,), 12, 0.1)
    x = _mk((B, cin, L), 13)
    conv = Conv1dHip(cin, cout, k, stride=s, padding=pad, transposed=True).set_precision('f16x3')
    conv.set_weight(w, b)
    xd = x.cuda()
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.1), w, b, stride=s, padding=pad)
    lean, plain = _both(monkeypatch, lambda: conv(xd, in_slope=0.1))
    err = float((lean.cpu() - ref).abs().max())
    print('tall %s L=%d B=%d: max |lean - torch| = %.3e, equal to TTSC_CONV_LEAN=0: %s' % ((cin, cout, k, s), L, B, err, torch.equal(lean, plain)))
    assert lean.shape == ref.shape
    assert torch.equal(lean, plain)
    assert err < F16X3_TOL
    if lens is not None:
        Lout = conv.out_len(L)
        lens_out = [conv.out_len(n) for n in lens]
        rl, rp = _both(monkeypatch, lambda: _ragged(conv, xd, lens, lens_out, Lout))
        assert torch.equal(rl, rp)
        monkeypatch.setenv('TTSC_CONV_WIDE', '2')
        n, no = lens[0], lens_out[0]
        solo = conv(x[:1, :, :n].contiguous().cuda(), in_slope=0.1)
        assert torch.equal(rl[:1, :, :no], solo)          # ragged == the utterance run alone, bit for bit
        assert torch.equal(rl[1:], lean[1:])
        ref0 = F.conv_transpose1d(F.leaky_relu(x[:1, :, :n], 0.1), w, b, stride=s, padding=pad)
        assert float((rl[:1, :, :no].cpu() - ref0).abs().max()) < F16X3_TOL


def _wide_case(C, k, d, x, monkeypatch, lens=None, xd=None):
    """one wide layer with residual and running sum (as test_conv1d_f16x3_wide_tile_kernel) and plain, lean against TTSC_CONV_LEAN=0 and torch.
    The residual and the running sum are N(0, 1/16): they are the accumulators' initial value, so the K * C / 16 accumulation steps round at the
    magnitude of the whole sum, and F16X3_TOL is an absolute bound for O(1) outputs — the operands keep the sum O(1)."""
    from ttscube_amd.hip_layers import Conv1dHip
    B, _, L = x.shape
    pad = d * (k - 1) // 2
    w = _mk((C, C, k), 1, 1.0 / (C * k) ** 0.5)
    b = _mk((C,), 2, 0.1)
    r = _mk((B, C, L), 4, 0.25)
    s0 = _mk((B, C, L), 5, 0.25)
    conv = Conv1dHip(C, C, k, padding=pad, dilation=d).set_precision('f16x3')
    conv.set_weight(w, b)
    xd = x.cuda() if xd is None else xd
    rd = r.cuda()

    def run_acc():
        out = s0.clone().cuda()
        conv(xd, resid=rd, out=out, in_scale=1.0 / 3.0, in_slope=0.1, accumulate=True)
        return out

    lean, plain = _both(monkeypatch, run_acc)
    ref = s0 + F.conv1d(F.leaky_relu(x / 3.0, 0.1), w, b, padding=pad, dilation=d) + r
    err = float((lean.cpu() - ref).abs().max())
    print('wide C=%d k=%d d=%d L=%d B=%d: max |lean - torch| = %.3e (resid + running sum), equal: %s' % (C, k, d, L, B, err, torch.equal(lean, plain)))
    assert torch.equal(lean, plain)
    assert err < F16X3_TOL
    yl, yp = _both(monkeypatch, lambda: conv(xd, in_slope=0.1))
    ref = F.conv1d(F.leaky_relu(x, 0.1), w, b, padding=pad, dilation=d)
    err = float((yl.cpu() - ref).abs().max())
    print('    plain call: max |lean - torch| = %.3e, equal: %s' % (err, torch.equal(yl, yp)))
    assert torch.equal(yl, yp)
    assert err < F16X3_TOL
    if lens is not None:
        rl, rp = _both(monkeypatch, lambda: _ragged(conv, xd, lens, lens, L))
        assert torch.equal(rl, rp)
        monkeypatch.setenv('TTSC_CONV_WIDE', '2')
        n = lens[0]
        solo = conv(x[:1, :, :n].contiguous().cuda(), in_slope=0.1)
        assert torch.equal(rl[:1, :, :n], solo)           # positions at or beyond `lin` are outside, although the memory behind them is readable
        assert torch.equal(rl[1:], yl[1:])


@pytest.mark.parametrize('C,k,d,L,B,lens', [
    (256, 3, 1, 5, 2, None),              # every staged position left of 0 or right of lin for some lane
    (256, 3, 5, 129, 1, None),
    (256, 11, 5, 131, 2, None),           # window wider than the data on both sides
    (128, 7, 3, 257, 2, [180, 257]),      # ragged
    (128, 11, 1, 513, 1, None),
])
def test_wide_kernel_lean_keeps_the_bits(C, k, d, L, B, lens, monkeypatch):
    _wide_case(C, k, d, _mk((B, C, L), 3), monkeypatch, lens=lens)


def test_wide_kernel_lean_never_reads_outside_its_utterance(monkeypatch):
    """the input is a view that starts one float into a larger allocation filled with 1e30 around it: a load that reaches outside its utterance shows
    as a wrong value (1e30 overflows the fp16 split), not as a fault"""
    B, C, L = 2, 256, 5
    x = _mk((B, C, L), 3)
    big = torch.full((B * C * L + 4096,), 1e30, device='cuda')
    big[1:1 + B * C * L] = x.flatten().cuda()
    xd = big[1:1 + B * C * L].view(B, C, L)
    assert xd.is_contiguous() and xd.data_ptr() == big.data_ptr() + 4
    _wide_case(C, 3, 1, x, monkeypatch, xd=xd)
