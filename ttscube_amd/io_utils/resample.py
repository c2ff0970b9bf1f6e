"""Sample-rate conversion on the GPU: what `scipy.signal.resample_poly(x, up, down)` computes with its defaults (a Kaiser-5 windowed-sinc low-pass of
20 max(up, down) + 1 taps, applied as a polyphase filter), for a whole batch of ragged rows in one HIP launch (csrc/resample.hip).
tests/resample_reference.py states it in float64:

    y[n] = sum_i x[i] h[n down - i up + half]   over |n down - i up| <= half,   half = 10 max(up, down),   n < ceil(L up / down)

scipy's default is matched; librosa's soxr resampler, which the reference's `librosa.load(path, sr=...)` would use, is not.  The filter is designed
here in float64 with numpy alone, rounded to float32 once and kept on the device per (up, down).  No CPU path."""
import ctypes as C
from math import gcd

import numpy as np
import torch

from .. import _lib

TILE = 256          # outputs per workgroup of the kernel (csrc/resample.hip::RESAMPLE_TILE); the tests place row ends around its multiples
MAX_RATE = 1024     # largest up or down after reduction: 44 101 Hz -> 24 kHz would be a filter of 882 021 taps


def ratio(orig_sr, target_sr):
    """-> coprime (up, down); a ratio the kernel refuses raises here, before anything is launched"""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr <= 0 or target_sr <= 0:
        raise ValueError('resample: sample rates must be positive, got %d -> %d' % (orig_sr, target_sr))
    g = gcd(orig_sr, target_sr)
    return _checked(target_sr // g, orig_sr // g, ' (%d Hz -> %d Hz)' % (orig_sr, target_sr))


def _checked(up, down, what=''):
    up, down = int(up), int(down)
    if up <= 0 or down <= 0:
        raise ValueError('resample: up and down must be positive, got up=%d down=%d' % (up, down))
    g = gcd(up, down)
    up, down = up // g, down // g
    if max(up, down) > MAX_RATE:
        raise ValueError('resample: up=%d down=%d%s: the reduced rates must not exceed %d (the filter has 20 max(up, down) + 1 taps)'
                         % (up, down, what, MAX_RATE))
    return up, down


def half_length(up, down):
    return 10 * max(up, down)


def design_filter(up, down):
    """-> np.float64 [2 half + 1]: scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up"""
    half = half_length(up, down)
    fc = 1.0 / max(up, down)
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = fc * np.sinc(fc * k) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def out_len(L, up, down):
    return -(-int(L) * int(up) // int(down))


def padded_taps(up, down):
    """-> np.float32 [up * K4]: the filter behind zeros up to K4 = ceil((2 half + 1) / up) rounded up to a multiple of 4 taps per phase (the
    kernel's layout: phase p of the filter is h[p], h[p + up], ...)"""
    h = design_filter(up, down)
    K4 = (-(-h.size // up) + 3) // 4 * 4
    t = np.zeros(up * K4, dtype=np.float32)
    t[:h.size] = h
    return t


def _p(t):
    return C.c_void_p(t.data_ptr())


class Resampler:
    def __init__(self, device='cuda:0'):
        self._device = torch.device(device)
        self._taps = {}

    def taps(self, up, down):
        t = self._taps.get((up, down))
        if t is None:
            t = self._taps[(up, down)] = torch.from_numpy(padded_taps(up, down)).to(self._device)
        return t

    def resample_poly_device(self, x, lengths, up, down):
        """x [B, Lmax] float32 and lengths [B] int32, both on the device -> y [B, out_len(Lmax)] float32 (zeros behind a row's own length),
        out_lengths [B] int64 and peak [B] float32 = max |y| of each row, all on the device (one launch)"""
        up, down = _checked(up, down)
        _lib.require_gpu()
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
        assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() == x.shape[0]
        B, Lmax = x.shape
        Omax = out_len(Lmax, up, down)
        taps = self.taps(up, down)
        y = torch.empty((B, Omax), dtype=torch.float32, device=x.device)
        peak = torch.empty((B,), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_resample_poly(_p(x), _p(lengths), B, Lmax, up, down, _p(taps), taps.numel(), _p(y), Omax, _p(peak),
                                                     _lib.current_stream()), 'ttsc_resample_poly')
        out_lengths = torch.div(lengths.clamp(0, Lmax).to(torch.int64) * up + (down - 1), down, rounding_mode='floor')
        return y, out_lengths, peak

    def resample_device(self, x, lengths, orig_sr, target_sr):
        """the same by sample rates.  Equal rates launch nothing: (x, lengths, None) comes back"""
        if int(orig_sr) == int(target_sr):
            return x, lengths, None
        up, down = ratio(orig_sr, target_sr)
        return self.resample_poly_device(x, lengths, up, down)

    def resample_poly(self, x, up, down, lengths=None):
        """x: 1-D array / tensor, or [B, L] with `lengths` (default: every row is L long) -> np.float32 [out_len(L)], or [B, out_len(L)] with zeros
        behind out_len(lengths[b])"""
        up, down = _checked(up, down)
        if up == down:                                            # (1, 1): scipy hands back a copy, nothing to filter
            return np.array(x.cpu() if torch.is_tensor(x) else x, dtype=np.float32)
        _lib.require_gpu()
        t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32)
        single = t.dim() == 1
        if single:
            t = t.unsqueeze(0)
        if t.dim() != 2:
            raise ValueError('Resampler: expected a 1-D signal or a [B, L] batch, got shape %s' % (tuple(t.shape),))
        B, L = t.shape
        if lengths is None:
            lengths = [L] * B
        lengths = [int(v) for v in lengths]
        if len(lengths) != B or any(v < 0 or v > L for v in lengths):
            raise ValueError('Resampler: lengths must hold one value in [0, %d] per row' % L)
        if B == 0 or L == 0:
            out = np.zeros((B, 0), dtype=np.float32)
            return out[0] if single else out
        y, _, _ = self.resample_poly_device(t.to(self._device).contiguous(), torch.tensor(lengths, dtype=torch.int32).to(self._device), up, down)
        out = y.cpu().numpy()
        return out[0] if single else out

    def __call__(self, x, orig_sr, target_sr, lengths=None):
        """x at orig_sr: 1-D or [B, L] as for resample_poly -> np.float32 at target_sr.  Equal rates give the input back untouched"""
        if int(orig_sr) == int(target_sr):
            return x
        up, down = ratio(orig_sr, target_sr)
        return self.resample_poly(x, up, down, lengths=lengths)


_RESAMPLERS = {}


def resample_poly(x, up, down, device='cuda:0'):
    """The call shape of `scipy.signal.resample_poly` with its defaults (axis 0 of a 1-D signal, the Kaiser-5 filter, zero padding) -> np.float32"""
    r = _RESAMPLERS.get(str(device))
    if r is None:
        r = _RESAMPLERS[str(device)] = Resampler(device)
    return r.resample_poly(x, up, down)
