"""Complex STFT, inverse STFT and Griffin-Lim on the GPU (csrc/stft_fft.hip: a radix-4 Stockham FFT held in LDS), device tensors in and out:
what `librosa.stft` / `librosa.istft` compute as MelVocoder calls them (cube/io_utils/vocoder.py:69-75) and the loop of
`MelVocoder._griffinlim` (vocoder.py:104-124).  tests/griffinlim_reference.py states all of it in float64.

Conventions: periodic Hann of length n_fft, centred frames over n_fft/2 samples of reflect padding, nb = n_fft/2 + 1 bins, F = 1 + L // hop
frames, the inverse returns hop (F - 1) samples; n_fft in SIZES, 1 <= hop <= n_fft.  Spectra are frame-major, [B, F, nb] (librosa's are
[nb, F]).  Batches are ragged: `lengths` / `frames` give every row its own size, a row's bits do not depend on the batch around it, and
whatever lies behind a row's own end is never read and comes back as zeros.

Twiddles and window are built here in float64, rounded to float32 once and kept on the device per (n_fft, device).  No CPU path."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import melspec

SIZES = (256, 512, 1024, 2048)

_tables = {}
_pinv = {}


def window(n_fft):
    """np.float64 [n_fft]: the periodic Hann window (scipy.signal.get_window('hann', n_fft))"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


def twiddles(n_fft):
    """np.complex128 [n_fft]: entry Ns + k = exp(-2 pi i k / (2 Ns)) for Ns = 1, 2, 4 .. n_fft/2 and k < Ns — stage Ns of the kernel's
    transform reads its own contiguous run; entry 0 is unused"""
    t = np.zeros(n_fft, dtype=np.complex128)
    Ns = 1
    while Ns < n_fft:
        t[Ns:2 * Ns] = np.exp(-2j * np.pi * np.arange(Ns, dtype=np.float64) / (2 * Ns))
        Ns *= 2
    return t


def host_tables(n_fft):
    """np.float32 [3 n_fft]: the twiddles as (re, im) pairs, then the window (the `tables_dev` of the C ABI)"""
    t = twiddles(n_fft)
    return np.concatenate([np.stack([t.real, t.imag], axis=1).reshape(-1), window(n_fft)]).astype(np.float32)


def tables(n_fft, dev):
    key = (n_fft, str(dev))
    if key not in _tables:
        _tables[key] = torch.from_numpy(host_tables(n_fft)).to(dev)
    return _tables[key]


def check_args(n_fft, hop, frames):
    """the argument checks of the C ABI, made before anything is allocated: -> TTSCError"""
    if n_fft not in SIZES:
        raise _lib.TTSCError('stft: n_fft=%r is not supported %r' % (n_fft, SIZES))
    if not 1 <= hop <= n_fft:
        raise _lib.TTSCError('stft: hop=%r outside [1, n_fft=%d]' % (hop, n_fft))
    for b, f in enumerate(frames):
        if f < 1 or hop * (f - 1) < n_fft // 2 + 1:
            raise _lib.TTSCError('stft: row %d has %d frames = %d samples at hop %d; reflect padding of n_fft/2 = %d needs at least %d samples'
                                 % (b, f, hop * max(f - 1, 0), hop, n_fft // 2, n_fft // 2 + 1))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_device(t, who):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.TTSCError('%s: input must be a tensor on a HIP device; no CPU path' % who)


class _Rows:
    """the per-row sizes of a ragged batch: a host copy for the argument checks and a device copy for the kernels (both None: every row is full)"""

    def __init__(self, values, B, vmax, dev, what):
        self.host = self.dev = None
        self.list = [vmax] * B
        if values is not None:
            v = [int(x) for x in (values.tolist() if torch.is_tensor(values) else values)]
            if len(v) != B or any(x > vmax for x in v):
                raise _lib.TTSCError('stft: %s must hold one value <= %d per row, got %r' % (what, vmax, v))
            self.list = v
            self.host = (C.c_int32 * B)(*v)
            self.dev = torch.tensor(v, dtype=torch.int32).to(dev)


def _batch(t, dims):
    single = t.dim() == dims - 1
    return (t.unsqueeze(0) if single else t), single


def _analyze(sig, rows, Fmax, n_fft, hop):
    B, Lpad = sig.shape
    spec = torch.empty((B, Fmax, n_fft // 2 + 1, 2), dtype=torch.float32, device=sig.device)
    _lib.check(_lib.lib().ttsc_stft_analyze(_p(sig), Lpad, rows.host, _p(rows.dev), B, Fmax, n_fft, hop, _p(tables(n_fft, sig.device)), _p(spec),
                                            _lib.current_stream()), 'ttsc_stft_analyze')
    return spec


def _synthesize(spec, rows, n_fft, hop):
    B, Fmax = spec.shape[:2]
    fr = torch.empty((B, Fmax, n_fft), dtype=torch.float32, device=spec.device)
    _lib.check(_lib.lib().ttsc_stft_synthesize(_p(spec), rows.host, _p(rows.dev), B, Fmax, n_fft, hop, _p(tables(n_fft, spec.device)), _p(fr),
                                               _lib.current_stream()), 'ttsc_stft_synthesize')
    return fr


def _project(sig, mag, rows, n_fft, hop, fr):
    B, Fmax = mag.shape[:2]
    _lib.check(_lib.lib().ttsc_stft_project(_p(sig), sig.shape[1], _p(mag), rows.host, _p(rows.dev), B, Fmax, n_fft, hop,
                                            _p(tables(n_fft, mag.device)), _p(fr), _lib.current_stream()), 'ttsc_stft_project')


def _overlap_add(fr, rows, n_fft, hop, padded, out=None):
    B, Fmax = fr.shape[:2]
    ldo = hop * (Fmax - 1) + (n_fft if padded else 0)
    if out is None:
        out = torch.empty((B, ldo), dtype=torch.float32, device=fr.device)
    _lib.check(_lib.lib().ttsc_stft_overlap_add(_p(fr), rows.host, _p(rows.dev), B, Fmax, n_fft, hop, _p(tables(n_fft, fr.device)), int(padded),
                                                _p(out), ldo, _lib.current_stream()), 'ttsc_stft_overlap_add')
    return out


def stft(y, lengths=None, n_fft=1024, hop=256):
    """y [B, L] (or [L]) float32 on a HIP device, lengths [B] samples per row (default: L) -> complex64 [B, F, nb], F = 1 + L // hop; row b
    has 1 + lengths[b] // hop frames, zeros behind them"""
    _need_device(y, 'stft')
    y, single = _batch(y, 2)
    y = y.float().contiguous()
    B, L = y.shape
    check_args(n_fft, hop, [])
    Fmax = 1 + L // hop
    lens = _Rows(lengths, B, L, y.device, 'lengths')
    frames = _Rows(None if lengths is None else [1 + v // hop for v in lens.list], B, Fmax, y.device, 'frames')
    check_args(n_fft, hop, frames.list)
    Lpad = L + n_fft
    sig = torch.empty((B, Lpad), dtype=torch.float32, device=y.device)
    with _lib.on_device(y.device):
        _lib.check(_lib.lib().ttsc_stft_reflect_pad(_p(y), lens.host, _p(lens.dev), B, L, n_fft, _p(sig), Lpad, _lib.current_stream()),
                   'ttsc_stft_reflect_pad')
        spec = torch.view_as_complex(_analyze(sig, frames, Fmax, n_fft, hop))
    return spec[0] if single else spec


def _spec_args(spec, frames, n_fft, hop, who, dims=3):
    _need_device(spec, who)
    spec, single = _batch(spec, dims)
    B, Fmax, nb = spec.shape
    if n_fft is None:
        n_fft = 2 * (nb - 1)
    if nb != n_fft // 2 + 1:
        raise _lib.TTSCError('%s: %d bins do not belong to n_fft=%r' % (who, nb, n_fft))
    rows = _Rows(frames, B, Fmax, spec.device, 'frames')
    check_args(n_fft, hop, rows.list)
    return spec, single, rows, n_fft


def istft(spec, frames=None, n_fft=None, hop=256):
    """spec complex64 [B, F, nb] (or [F, nb]) on a HIP device, frames [B] per row (default: F) -> float32 [B, hop (F - 1)]; row b holds
    hop (frames[b] - 1) samples, zeros behind them"""
    spec, single, rows, n_fft = _spec_args(spec, frames, n_fft, hop, 'istft')
    if not spec.is_complex():
        raise _lib.TTSCError('istft: expected a complex spectrum')
    sp = torch.view_as_real(spec.to(torch.complex64).contiguous())
    with _lib.on_device(spec.device):
        y = _overlap_add(_synthesize(sp, rows, n_fft, hop), rows, n_fft, hop, False)
    return y[0] if single else y


def draw_angles(nb, F, rng=None):
    """the reference's starting phases (vocoder.py:108 on a [nb, F] spectrogram): rand(nb, F), bin-major, from numpy's global generator (or
    `rng`), exp(2 pi i u) in float64 -> np.complex64 [F, nb]"""
    u = (np.random if rng is None else rng).rand(nb, F)
    return np.ascontiguousarray(np.exp(2j * np.pi * u).T).astype(np.complex64)


def griffinlim(mag, frames=None, n_iter=100, n_fft=None, hop=256, angles=None, rng=None):
    """MelVocoder._griffinlim: mag [B, F, nb] (or [F, nb]) float32 on a HIP device — its absolute value is taken, as the reference does —
    -> float32 audio [B, hop (F - 1)].  angles: complex64 [B, F, nb] starting phases; None draws them as the reference does, one
    `draw_angles` per row in row order.  One launch for the first inverse transform, then two per iteration (overlap-add that writes the next
    reflect-padded signal; forward transform + phase projection + inverse transform in one), all queued on the current stream with no host
    synchronisation in between, then the last overlap-add."""
    mag, single, rows, n_fft = _spec_args(mag, frames, n_fft, hop, 'griffinlim')
    if mag.is_complex():
        raise _lib.TTSCError('griffinlim: expected a magnitude, got a complex spectrum')
    n_iter = int(n_iter)
    if n_iter < 0:
        raise _lib.TTSCError('griffinlim: n_iter=%d' % n_iter)
    mag = mag.float().contiguous()
    B, Fmax, nb = mag.shape
    if angles is None:
        angles = torch.from_numpy(np.stack([draw_angles(nb, Fmax, rng) for _ in range(B)])).to(mag.device)
    else:
        _need_device(angles, 'griffinlim')
        angles = angles.to(torch.complex64).reshape(B, Fmax, nb)
    with _lib.on_device(mag.device):
        sp = torch.view_as_real((mag.abs() * angles).contiguous())
        fr = _synthesize(sp, rows, n_fft, hop)
        sig = torch.empty((B, hop * (Fmax - 1) + n_fft), dtype=torch.float32, device=mag.device) if n_iter else None
        for _ in range(n_iter):
            _overlap_add(fr, rows, n_fft, hop, True, out=sig)
            _project(sig, mag, rows, n_fft, hop, fr)
        y = _overlap_add(fr, rows, n_fft, hop, False)
    return y[0] if single else y


def mel_pinv(sample_rate, num_mels, n_fft=1024):
    """np.float64 [nb, num_mels]: the pseudo-inverse of melspec.mel_filterbank (computed once per key)"""
    key = (int(sample_rate), int(num_mels), int(n_fft))
    if key not in _pinv:
        _pinv[key] = np.linalg.pinv(melspec.mel_filterbank(sample_rate, n_fft, num_mels).astype(np.float64))
    return _pinv[key]


def mel_to_linear(mel_log10, sample_rate, num_mels, n_fft=1024):
    """mel_log10 [B, F, num_mels] (or [F, num_mels]) on a HIP device -> linear magnitude [B, F, nb] = max(0, pinv(mel_basis) . 10**mel).

    NOT in the reference: MelVocoder.griffinlim takes a linear spectrogram and the reference never inverts its mel basis.  This is what makes
    Griffin-Lim usable on this project's 80-bin log10-mel features (the least-squares linear spectrum of the mel, negative entries clamped).
    The product runs through ttsc_linear_forward; the pseudo-inverse is float64 on the host, rounded once."""
    _need_device(mel_log10, 'mel_to_linear')
    m, single = _batch(mel_log10, 3)
    B, F, K = m.shape
    if K != num_mels:
        raise _lib.TTSCError('mel_to_linear: %d mel bins, num_mels=%d' % (K, num_mels))
    nb = n_fft // 2 + 1
    key = ('pinv', int(sample_rate), int(num_mels), int(n_fft), str(m.device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.ascontiguousarray(mel_pinv(sample_rate, num_mels, n_fft).astype(np.float32))).to(m.device)
    w = _tables[key]                                              # [nb, num_mels]: y = x . w^T
    x = torch.pow(10.0, m.float()).contiguous()
    y = torch.empty((B, F, nb), dtype=torch.float32, device=m.device)
    with _lib.on_device(m.device):
        _lib.check(_lib.lib().ttsc_linear_forward(_p(x), _p(w), None, _p(y), B * F, nb, K, K, nb, _lib.ACT_RELU, 0, _lib.current_stream()),
                   'ttsc_linear_forward')
    return y[0] if single else y
