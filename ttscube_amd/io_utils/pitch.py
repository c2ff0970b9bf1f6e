"""Per-frame F0 of the processed corpus' `<id>.pitch` files: what the reference's importer gets from `pysptk.rapt` (scripts/import_textgrid.py:178),
here two HIP launches for a whole batch of ragged utterances (csrc/pitch.hip).

The algorithm is a single-rate restatement of RAPT (Talkin 1995, "A robust algorithm for pitch tracking") with its published structure and constants:
a normalised cross-correlation over every lag of [sr / fmax, sr / fmin] on a 7.5 ms window every hop, the 20 largest peaks above 0.3 of the frame's
maximum as voiced candidates beside one unvoiced state, and a Viterbi pass through time.  tests/pitch_reference.py states it in float64.  pysptk is
not matched number for number, and two parts of RAPT are left out on purpose:
  * the decimated first pass — it prunes the lag search for a CPU; the GPU evaluates every lag at the full rate;
  * the spectral-stationarity term of the voicing transitions — it needs an LPC analysis of every frame.  The transitions keep RAPT's fixed cost
    and its rms-ratio term.
An utterance of L samples gets L // hop frames: at most the `.mgc` frame count 1 + L // hop, so CubeganCollate's mel-length pitch row holds it."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib

N_CANDS = 20
WINDOW_S = 0.0075


def lag_range(sample_rate, fmin, fmax):
    """-> n (window in samples), kmin, kmax"""
    return int(round(WINDOW_S * sample_rate)), int(math.floor(sample_rate / fmax)), int(math.ceil(sample_rate / fmin))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def nccf(x, lengths, sample_rate, hop_size, fmin=60, fmax=400, want_phi=False):
    """x [B, Lmax] float32 device tensor, lengths [B] int32 device tensor -> dict of the candidate tables (ttsc_pitch_nccf): cand_lag, cand_val
    [B, F, 20], ncand [B, F] int32, maxphi, rms [B, F], and phi [B, F, K] with want_phi; F = Lmax // hop_size."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
    assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.numel() == x.shape[0]
    n, kmin, kmax = lag_range(sample_rate, fmin, fmax)
    B, Lmax = x.shape
    F = Lmax // hop_size
    dev = x.device
    out = {'cand_lag': torch.empty((B, F, N_CANDS), dtype=torch.float32, device=dev),
           'cand_val': torch.empty((B, F, N_CANDS), dtype=torch.float32, device=dev),
           'ncand': torch.empty((B, F), dtype=torch.int32, device=dev),
           'maxphi': torch.empty((B, F), dtype=torch.float32, device=dev),
           'rms': torch.empty((B, F), dtype=torch.float32, device=dev),
           'phi': torch.empty((B, F, kmax - kmin + 1), dtype=torch.float32, device=dev) if want_phi else None}
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ttsc_pitch_nccf(_p(x), _p(lengths), B, Lmax, hop_size, n, kmin, kmax, _p(out['cand_lag']), _p(out['cand_val']),
                                              _p(out['ncand']), _p(out['maxphi']), _p(out['rms']), _p(out['phi']), _lib.current_stream()),
                   'ttsc_pitch_nccf')
    return out


def track(cand_lag, cand_val, ncand, maxphi, rms, nframes, kmax, sample_rate):
    """the Viterbi pass over candidate tables (ttsc_pitch_track; the tables may be injected ones) -> f0 [B, F] float32 device tensor"""
    B, F = ncand.shape
    dev = ncand.device
    for t, dt in ((cand_lag, torch.float32), (cand_val, torch.float32), (ncand, torch.int32), (maxphi, torch.float32), (rms, torch.float32),
                  (nframes, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous()
    assert cand_lag.shape == (B, F, N_CANDS) and cand_val.shape == (B, F, N_CANDS) and nframes.numel() == B
    f0 = torch.empty((B, F), dtype=torch.float32, device=dev)
    if F == 0:
        return f0
    L = _lib.lib()
    nbytes = int(L.ttsc_pitch_track_workspace_bytes(B, F))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.ttsc_pitch_track(_p(cand_lag), _p(cand_val), _p(ncand), _p(maxphi), _p(rms), _p(nframes), B, F, kmax, float(sample_rate), _p(ws),
                                      nbytes, _p(f0), _lib.current_stream()), 'ttsc_pitch_track')
    return f0


class PitchTracker:
    def __init__(self, device='cuda:0'):
        self._device = torch.device(device)

    def f0_device(self, x, lengths, sample_rate, hop_size, fmin=60, fmax=400):
        """x [B, Lmax] float32 and lengths [B] int32, both on the device -> f0 [B, Lmax // hop_size] float32 on the device (two launches)"""
        _, _, kmax = lag_range(sample_rate, fmin, fmax)
        tab = nccf(x, lengths, sample_rate, hop_size, fmin, fmax)
        nframes = torch.div(lengths, hop_size, rounding_mode='floor').to(torch.int32)
        return track(tab['cand_lag'], tab['cand_val'], tab['ncand'], tab['maxphi'], tab['rms'], nframes, kmax, sample_rate)

    def __call__(self, y, sample_rate, hop_size, fmin=60, fmax=400, lengths=None):
        """y: 1-D array / tensor in [-1, 1], or [B, L] with `lengths` (default: every row is L long) -> np.float64 [L // hop_size], or
        [B, L // hop_size] with zeros behind lengths[b] // hop_size"""
        t = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y, dtype=torch.float32)
        single = t.dim() == 1
        if single:
            t = t.unsqueeze(0)
        if t.dim() != 2:
            raise ValueError('PitchTracker: expected a 1-D signal or a [B, L] batch, got shape %s' % (tuple(t.shape),))
        B, L = t.shape
        if lengths is None:
            lengths = [L] * B
        lengths = [int(v) for v in lengths]
        if len(lengths) != B or any(v < 0 or v > L for v in lengths):
            raise ValueError('PitchTracker: lengths must hold one value in [0, %d] per row' % L)
        if L // hop_size == 0:
            out = np.zeros((B, 0), dtype=np.float64)
            return out[0] if single else out
        x = t.to(self._device).contiguous()
        f0 = self.f0_device(x, torch.tensor(lengths, dtype=torch.int32).to(self._device), sample_rate, hop_size, fmin, fmax)
        out = f0.cpu().numpy().astype(np.float64)
        return out[0] if single else out


_TRACKERS = {}


def rapt(x, fs, hopsize, min=60, max=400, otype='f0', device='cuda:0'):
    """The call shape of `pysptk.rapt` as the reference's scripts use it: x on the int16 scale (floats in [-32768, 32767]) -> np.float64 [len(x) //
    hopsize], 0 where unvoiced.  Only otype='f0'."""
    if otype != 'f0':
        raise NotImplementedError("rapt: only otype='f0' is provided, not %r" % (otype,))
    tracker = _TRACKERS.get(str(device))
    if tracker is None:
        tracker = _TRACKERS[str(device)] = PitchTracker(device)
    return tracker(np.asarray(x, dtype=np.float32) / 32768.0, fs, hopsize, fmin=min, fmax=max)
