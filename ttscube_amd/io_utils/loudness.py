"""Loudness normalisation on the GPU: ITU-R BS.1770-4 / EBU R 128 integrated loudness (K-weighting, 400 ms blocks at a 100 ms step, the absolute
and the relative gate), a 4x true peak and one static gain per row, for a ragged batch of mono rows (csrc/loudness.hip).
tests/loudness_reference.py states all of it in float64.

Definition.
  K-weighting at any rate sr: the two biquads are re-designed from their analogue prototypes by the bilinear transform (`k_weighting`); the 48 kHz
  table of the Recommendation comes out to 1e-15 and is not reused at other rates (applied unchanged at 24 kHz it reads a full-scale 997 Hz sine
  at -0.64 LUFS instead of -2.98).  The re-design itself drifts a little: that sine reads -3.01027 LUFS at 48 kHz, -2.98433 at 24 kHz, -2.97004 at
  16 kHz, as in every meter that re-designs.
  Sub-block k: the sum of squares of the K-weighted row over samples [k sr/10, (k+1) sr/10).  sr is a positive multiple of 10 with sr / 10 >= CHUNK.
  Block j: z_j = (sub-blocks j .. j+3) / (4 sr/10).  Departure: a row of 0 < L < 4 sr/10 samples has ONE block, the mean square of the whole row
  (the Recommendation leaves it undefined; a TTS meter sees one-word sentences).  A row of 0 samples has no block.
  Gates, strict, in the energy domain: z_j > ABS_GATE = 10^((-70 + 0.691) / 10), then also z_j > 0.1 mean(z over the absolute gate).
  zbar = mean z over both gates, L = -0.691 + 10 log10(zbar).  No block passes: L = -inf, the row is silent and its gain is 1.
  True peak: max |y| of the row oversampled 4x with resample.design_filter(4, 1) rounded to float32, zeros beyond the ends.  Departure: this is the
  project's own 81-tap filter, not the 48-tap table of Annex 2.  The ceiling acts on max(sample peak, true peak).
  Gain: g = sqrt(10^((target + 0.691) / 10) / zbar), g = min(g, 10^(peak_db / 20) / peak), optionally g = min(g, 10^(max_gain_db / 20)); the
  output is fl32(fl32(g) x), one product rounded once.  No logarithm on the device.

No CPU path: a missing kernel is an error."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from . import resample

CHUNK = 64                  # samples a thread filters (csrc/loudness.hip::LOUD_CHUNK)
TILE = 256 * CHUNK          # samples of a workgroup (LOUD_TILE); tiles count from a row's own first sample
LEVELS = 8                  # log2(TILE / CHUNK): levels of the in-workgroup scan
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)

_SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)
_SHELF_VB_EXP = 0.4996667741545416
_HIGHPASS = (38.13547087602444, 0.5003270373238773)


def check_rate(sr):
    if int(sr) != sr or sr <= 0 or int(sr) % 10 != 0 or int(sr) // 10 < CHUNK:
        raise ValueError('loudness: sr=%r: the rate must be a positive multiple of 10 with sr / 10 >= %d (100 ms sub-blocks of whole samples, no '
                         'shorter than a chunk)' % (sr, CHUNK))
    return int(sr)


def k_weighting(sr):
    """-> np.float64 [2, 6]: (b0, b1, b2, 1, a1, a2) of the shelf and of the high-pass at rate sr (scipy's `sos` layout)"""
    sr = float(sr)
    f0, G, Q = _SHELF
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** _SHELF_VB_EXP
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = _HIGHPASS
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], dtype=np.float64)


def cascade_step(sos, s, x):
    """one sample through the two transposed direct-form-II biquads: -> (y, new state); s = (s1, s2 of the shelf, s1, s2 of the high-pass).
    The order of the operations is the kernel's"""
    (b0, b1, b2, _, a1, a2), (c0, c1, c2, _, d1, d2) = sos
    u = b0 * x + s[0]
    n0 = (b1 * x - a1 * u) + s[1]
    n1 = b2 * x - a2 * u
    y = c0 * u + s[2]
    n2 = (c1 * u - d1 * y) + s[3]
    n3 = c2 * u - d2 * y
    return y, (n0, n1, n2, n3)


def state_matrix(sos):
    """-> np.float64 [4, 4]: A with s_next = A s at x = 0"""
    A = np.zeros((4, 4))
    for i in range(4):
        e = [0.0] * 4
        e[i] = 1.0
        A[:, i] = cascade_step(sos, e, 0.0)[1]
    return A


def state_powers(sos):
    """-> np.float64 [LEVELS + 1, 4, 4]: A^(CHUNK 2^k), k = 0 .. LEVELS (the last one is A^TILE), by repeated squaring in float64"""
    M = state_matrix(sos)
    for _ in range(int(math.log2(CHUNK))):
        M = M @ M
    out = [M]
    for _ in range(LEVELS):
        out.append(out[-1] @ out[-1])
    return np.stack(out)


def kernel_constants(sr):
    """-> np.float64 [154]: what ttsc_loudness_measure takes as kweight_host"""
    sos = k_weighting(check_rate(sr))
    return np.ascontiguousarray(np.concatenate([sos[:, [0, 1, 2, 4, 5]].reshape(-1), state_powers(sos).reshape(-1)]))


TP_UP = 4
TP_HALF = 10                # input samples the 4x filter reaches to either side
TP_TAPS = 2 * TP_HALF + 1   # taps per phase


def true_peak_taps():
    """-> np.float32 [4, 21]: entry [p][d + 10] = fl32(h[4 d + p + 40]) of h = resample.design_filter(4, 1), 0 where that index is outside h:
    output 4 m + p of the oversampled row is sum_d x[m - d] h[4 d + p + 40]"""
    h = resample.design_filter(TP_UP, 1).astype(np.float32)
    half = resample.half_length(TP_UP, 1)
    t = np.zeros((TP_UP, TP_TAPS), dtype=np.float32)
    for p in range(TP_UP):
        for d in range(-TP_HALF, TP_HALF + 1):
            i = TP_UP * d + p + half
            if 0 <= i < h.size:
                t[p, d + TP_HALF] = h[i]
    return t


def lufs(zbar):
    """-0.691 + 10 log10(zbar) elementwise; -inf at 0"""
    z = np.asarray(zbar, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return -0.691 + 10.0 * np.log10(z)


def target_energy(target):
    return 10.0 ** ((np.asarray(target, dtype=np.float64) + 0.691) / 10.0)


def host_gain(zbar, peak, silent, target, peak_db=-1.0, max_gain_db=None):
    """the gain of one row in float64 -> (np.float32 gain, peak_limited)"""
    if silent:
        return np.float32(1.0), False
    g = math.sqrt(float(target_energy(target)) / float(zbar))
    limited = False
    if peak > 0.0:
        c = 10.0 ** (float(peak_db) / 20.0) / float(peak)
        if c < g:
            g, limited = c, True
    if max_gain_db is not None:
        g = min(g, 10.0 ** (float(max_gain_db) / 20.0))
    return np.float32(g), limited


def _p(t):
    return C.c_void_p(t.data_ptr())


def _per_row(v, B, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, B)
    if a.size != B or not np.all(np.isfinite(a)):
        raise ValueError('loudness: %s must be one finite value, or one per row (%d), got %r' % (name, B, v))
    return a


class LoudnessMeter:
    def __init__(self, device='cuda:0'):
        self._device = torch.device(device)
        self._k = {}
        self._taps = np.ascontiguousarray(true_peak_taps())

    def _constants(self, sr):
        k = self._k.get(sr)
        if k is None:
            k = self._k[sr] = kernel_constants(sr)
        return k

    @staticmethod
    def _check_batch(x, lengths):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()):
            raise ValueError('loudness: x must be a contiguous [B, Lmax] float32 device tensor')
        if not (torch.is_tensor(lengths) and lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() == x.shape[0]
                and lengths.is_contiguous()):
            raise ValueError('loudness: lengths must be a contiguous [B] int32 device tensor')
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError('loudness: empty batch %s' % (tuple(x.shape),))

    def measure_device(self, x, lengths, sr, target=None, peak_db=-1.0, max_gain_db=None):
        """x [B, Lmax] float32, lengths [B] int32, on the device -> dict of device tensors: zbar f64, sample_peak, true_peak f32, blocks, gated,
        silent int32, sub [B, nsub] f64 (the sub-block energies); with a target also gain f32 and limited int32, from the same finish launch.
        No host synchronisation."""
        sr = check_rate(sr)
        self._check_batch(x, lengths)
        _lib.require_gpu()
        B, Lmax = x.shape
        dev = x.device
        nsub = -(-Lmax // (sr // 10))
        L = _lib.lib()
        sub = torch.empty((B, nsub), dtype=torch.float64, device=dev)
        sp = torch.empty((B,), dtype=torch.float32, device=dev)
        tp = torch.empty((B,), dtype=torch.float32, device=dev)
        st = {'sub': sub, 'sample_peak': sp, 'true_peak': tp, 'zbar': torch.empty((B,), dtype=torch.float64, device=dev)}
        for n in ('blocks', 'gated', 'silent'):
            st[n] = torch.empty((B,), dtype=torch.int32, device=dev)
        te = pl = gain = lim = None
        mg = 0.0
        if target is not None:
            te, pl, mg = self._gain_args(B, target, peak_db, max_gain_db, dev)
            gain = st['gain'] = torch.empty((B,), dtype=torch.float32, device=dev)
            lim = st['limited'] = torch.empty((B,), dtype=torch.int32, device=dev)
        k = self._constants(sr)
        with _lib.on_device(dev):
            nbytes = int(L.ttsc_loudness_workspace_bytes(B, Lmax, sr))
            ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
            stream = _lib.current_stream()
            _lib.check(L.ttsc_loudness_measure(_p(x), _p(lengths), B, Lmax, sr, k.ctypes.data_as(C.c_void_p), self._taps.ctypes.data_as(C.c_void_p),
                                               _p(sub), nsub, _p(sp), _p(tp), _p(ws), nbytes, stream), 'ttsc_loudness_measure')
            _lib.check(L.ttsc_loudness_finish(_p(sub), _p(lengths), B, Lmax, nsub, sr, _p(sp), _p(tp), ABS_GATE, _p(te) if te is not None else None,
                                              _p(pl) if pl is not None else None, mg, _p(st['zbar']), _p(st['blocks']), _p(st['gated']),
                                              _p(st['silent']), _p(gain) if gain is not None else None, _p(lim) if lim is not None else None,
                                              stream), 'ttsc_loudness_finish')
        return st

    @staticmethod
    def _gain_args(B, target, peak_db, max_gain_db, dev):
        te = target_energy(_per_row(target, B, 'target'))
        pl = 10.0 ** (_per_row(peak_db, B, 'peak_db') / 20.0)
        mg = 0.0 if max_gain_db is None else 10.0 ** (float(max_gain_db) / 20.0)
        both = torch.from_numpy(np.stack([te, pl])).pin_memory().to(dev, non_blocking=True)
        return both[0], both[1], mg

    def gains_device(self, stats, target, peak_db=-1.0, max_gain_db=None):
        """stats of measure_device -> (gain [B] float32, limited [B] int32) on the device for `target` LUFS (a scalar or one per row) under the peak
        ceiling `peak_db` dBTP and, when given, the largest gain `max_gain_db`; 1 for a silent row"""
        z = stats['zbar']
        B, dev = z.numel(), z.device
        te, pl, mg = self._gain_args(B, target, peak_db, max_gain_db, dev)
        gain = torch.empty((B,), dtype=torch.float32, device=dev)
        lim = torch.empty((B,), dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ttsc_loudness_gain(_p(z), _p(stats['sample_peak']), _p(stats['true_peak']), _p(stats['silent']), _p(te), _p(pl), mg,
                                                     B, _p(gain), _p(lim), _lib.current_stream()), 'ttsc_loudness_gain')
        return gain, lim

    def apply_device(self, x, lengths, gain, out=None):
        """-> y [B, Lmax] with y[b, n] = fl32(gain[b] x[b, n]) for n < lengths[b]; out=x works in place; nothing is written behind a row's length
        (a fresh `out` starts as zeros)"""
        self._check_batch(x, lengths)
        if not (torch.is_tensor(gain) and gain.is_cuda and gain.dtype == torch.float32 and gain.numel() == x.shape[0] and gain.is_contiguous()):
            raise ValueError('loudness: gain must be a contiguous [B] float32 device tensor')
        if out is None:
            out = torch.zeros_like(x)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()):
            raise ValueError('loudness: out must be a contiguous float32 device tensor shaped like x')
        _lib.require_gpu()
        B, Lmax = x.shape
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_loudness_apply(_p(x), _p(lengths), _p(gain), B, Lmax, _p(out), _lib.current_stream()), 'ttsc_loudness_apply')
        return out

    def normalize_device(self, x, lengths, sr, target, peak_db=-1.0, max_gain_db=None, inplace=True):
        """measure, finish and apply without a host synchronisation in between -> (y, stats)"""
        st = self.measure_device(x, lengths, sr, target=target, peak_db=peak_db, max_gain_db=max_gain_db)
        return self.apply_device(x, lengths, st['gain'], out=x if inplace else None), st

    # ---- host conveniences -------------------------------------------------------------------------------------------------------------
    def _pad(self, rows):
        rows = [np.asarray(r.detach().cpu() if torch.is_tensor(r) else r, dtype=np.float32).reshape(-1) for r in rows]
        lens = [r.size for r in rows]
        x = np.zeros((len(rows), max(max(lens), 1)), dtype=np.float32)
        for i, r in enumerate(rows):
            x[i, :r.size] = r
        return torch.from_numpy(x).to(self._device), torch.tensor(lens, dtype=torch.int32).to(self._device), lens

    def integrated_loudness(self, x, sr):
        """one 1-D signal -> LUFS (float; -inf for silence)"""
        xd, ld, _ = self._pad([x])
        return float(lufs(self.measure_device(xd, ld, sr)['zbar'].cpu().numpy())[0])

    def normalize(self, rows, sr, target=-23.0, peak_db=-1.0, max_gain_db=None):
        """rows: 1-D float signals at rate sr -> (list of np.float32 rows, list of reports {lufs_in, lufs_out, gain_db, peak_limited, silent}).
        target and peak_db: a scalar or one per row.  Silent rows come back unscaled.  lufs_out is lufs_in + gain_db, what a static gain does."""
        if len(rows) == 0:
            return [], []
        xd, ld, lens = self._pad(rows)
        y, st = self.normalize_device(xd, ld, sr, target, peak_db=peak_db, max_gain_db=max_gain_db)
        y = y.cpu().numpy()
        zin = lufs(st['zbar'].cpu().numpy())
        gain, lim, sil = st['gain'].cpu().numpy(), st['limited'].cpu().numpy(), st['silent'].cpu().numpy()
        out, rep = [], []
        for i, n in enumerate(lens):
            gdb = 20.0 * math.log10(float(gain[i]))
            rep.append({'lufs_in': float(zin[i]), 'lufs_out': float(zin[i] + gdb), 'gain_db': gdb, 'peak_limited': bool(lim[i]),
                        'silent': bool(sil[i])})
            out.append(y[i, :n].copy())
        return out, rep


_METERS = {}


def meter(device='cuda:0'):
    """the LoudnessMeter of a device, made once"""
    m = _METERS.get(str(device))
    if m is None:
        m = _METERS[str(device)] = LoudnessMeter(device)
    return m
