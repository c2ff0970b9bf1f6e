"""float64 statement of the complex STFT, the inverse STFT and the Griffin-Lim loop (csrc/stft_fft.hip, io_utils/stft.py): what
librosa.stft / librosa.istft compute with the arguments MelVocoder gives them (cube/io_utils/vocoder.py:69-75: window='hann', win_length = n_fft,
center=True, reflect padding) and the loop of MelVocoder._griffinlim (vocoder.py:104-124), restated with numpy alone — librosa is not installed.

Spectra are frame-major here, [F, nb] with nb = n_fft/2 + 1 (librosa's are [nb, F]; MelVocoder.fft / ifft / griffinlim transpose at their
borders, so [F, nb] is also what their callers see).

    stft    y [L] -> pad n_fft/2 samples by reflection on both sides, F = 1 + L // hop frames at hop, times the periodic Hann window, rfft
    istft   irfft of every frame, times the window, overlap-add at hop; divided by the overlap-added SQUARED window (librosa's window_sumsquare)
            where that exceeds tiny(float32), left undivided elsewhere; n_fft/2 samples trimmed from both ends -> hop (F - 1) samples
    griffinlim   n_iter x [ inverse = istft(|mag| angles); angles = exp(1j angle(stft(inverse))) ], then istft(|mag| angles)

`dtype=np.float32` runs every step in single precision (window, frames, numpy's float32 transform, the sums): the twin that says what float32
arithmetic itself costs on a given case."""
import numpy as np

SIZES = (256, 512, 1024, 2048)

# n_fft, hop, F, seed, amplitude
CASES = (
    (256, 64, 6, 100, 1.0),         # 0 smallest size, hop = n/4
    (256, 256, 4, 101, 1.0),        # 1 hop = n_fft: the envelope is exactly 0 at the frame joins, those samples stay undivided
    (256, 128, 5, 102, 1.0),        # 2 hop = n/2
    (512, 120, 9, 103, 1.0),        # 3 odd power of two, hop does not divide n_fft
    (1024, 256, 4, 104, 1.0),       # 4 the shortest row reflect padding admits
    (1024, 256, 10, 105, 1.0),      # 5 the reference's parameters
    (1024, 240, 7, 106, 1.0),       # 6 this project's hop
    (2048, 512, 5, 107, 1.0),       # 7 largest size
    (256, 64, 12, 108, 1e-20),      # 8 squared magnitudes underflow in float32
)


def _ctype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def hann(n_fft, dtype=np.float64):
    """scipy.signal.get_window('hann', n_fft, fftbins=True): periodic"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)).astype(dtype)


def check_args(n_fft, hop, L):
    if n_fft not in SIZES:
        raise ValueError('n_fft=%r is not one of %r' % (n_fft, SIZES))
    if not 1 <= hop <= n_fft:
        raise ValueError('hop=%r outside [1, n_fft=%d]' % (hop, n_fft))
    if hop * (L // hop) < n_fft // 2 + 1:
        raise ValueError('%d samples: reflect padding of %d needs at least %d in whole hops' % (L, n_fft // 2, n_fft // 2 + 1))


def stft(y, n_fft, hop, dtype=np.float64):
    """y [L] -> [F, nb] complex, F = 1 + L // hop"""
    y = np.asarray(y, dtype=dtype)
    check_args(n_fft, hop, y.shape[0])
    w = hann(n_fft, dtype)
    yp = np.pad(y, n_fft // 2, mode='reflect')
    F = 1 + y.shape[0] // hop
    frames = np.stack([yp[f * hop:f * hop + n_fft] * w for f in range(F)]).astype(dtype)
    return np.fft.rfft(frames, axis=1).astype(_ctype(dtype))


def envelope(n_fft, hop, F, dtype=np.float64):
    """librosa.filters.window_sumsquare over the untrimmed length n_fft + hop (F - 1)"""
    w2 = (hann(n_fft, dtype) ** 2).astype(dtype)
    env = np.zeros(n_fft + hop * (F - 1), dtype=dtype)
    for f in range(F):
        env[f * hop:f * hop + n_fft] += w2
    return env


def istft(S, hop, dtype=np.float64):
    """S [F, nb] -> [hop (F - 1)]"""
    S = np.asarray(S).astype(_ctype(dtype))
    F, nb = S.shape
    n_fft = 2 * (nb - 1)
    check_args(n_fft, hop, hop * (F - 1))
    w = hann(n_fft, dtype)
    fr = (np.fft.irfft(S, n=n_fft, axis=1).astype(dtype) * w).astype(dtype)
    y = np.zeros(n_fft + hop * (F - 1), dtype=dtype)
    for f in range(F):
        y[f * hop:f * hop + n_fft] += fr[f]
    env = envelope(n_fft, hop, F, dtype)
    nz = env > np.finfo(np.float32).tiny
    y[nz] /= env[nz]
    return y[n_fft // 2:n_fft // 2 + hop * (F - 1)]


def unit_phase(z):
    """np.exp(1j * np.angle(z)) in z's own precision; angle(0) = 0, so a bin that is exactly zero gets phase 1"""
    return np.exp(1j * np.angle(z)).astype(z.dtype)


def griffinlim(mag, angles, n_iter, hop, dtype=np.float64, trace=None):
    """mag [F, nb] (its absolute value is taken, as the reference does), angles [F, nb] complex of modulus 1 -> [hop (F - 1)].
    trace (a list): receives the audio before every projection and the final one, n_iter + 1 signals"""
    mag = np.abs(np.asarray(mag, dtype=np.float64)).astype(dtype)
    angles = np.asarray(angles).astype(_ctype(dtype))
    n_fft = 2 * (mag.shape[1] - 1)
    for _ in range(n_iter):
        inverse = istft(mag * angles, hop, dtype)
        if trace is not None:
            trace.append(inverse)
        angles = unit_phase(stft(inverse, n_fft, hop, dtype))
    out = istft(mag * angles, hop, dtype)
    if trace is not None:
        trace.append(out)
    return out


def inconsistency(mag, y, n_fft, hop, dtype=np.float64):
    """|| |mag| - |STFT(y)| ||_F : what Griffin-Lim's alternating projections do not increase"""
    return float(np.linalg.norm(np.abs(np.asarray(mag, dtype=np.float64)) - np.abs(stft(y, n_fft, hop, dtype)).astype(np.float64)))


def preemphasis(x, coef=0.97):
    """scipy.signal.lfilter([1, -coef], [1], x) as the explicit recurrence"""
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    for t in range(x.shape[0]):
        y[t] = x[t] - (coef * x[t - 1] if t > 0 else 0.0)
    return y


_case_cache = {}


def case(i):
    """-> dict(n_fft, hop, F, L, y, angles [F, nb], mag [F, nb] = |STFT64(y)|, S = STFT64(y)); built once, never modified"""
    if i not in _case_cache:
        n_fft, hop, F, seed, amp = CASES[i]
        nb = n_fft // 2 + 1
        L = hop * (F - 1)
        t = np.arange(L)
        rng = np.random.RandomState(seed)
        y = amp * (0.5 * np.sin(2 * np.pi * 0.031 * t) + 0.3 * np.sin(2 * np.pi * 0.11 * t + 1) + 0.05 * rng.randn(L))
        u = rng.rand(nb, F)
        angles = np.exp(2j * np.pi * u).T
        S = stft(y, n_fft, hop)
        assert S.shape == (F, nb)
        c = dict(n_fft=n_fft, hop=hop, F=F, L=L, nb=nb, y=y, angles=np.ascontiguousarray(angles), S=S, mag=np.abs(S))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _case_cache[i] = c
    return _case_cache[i]


_gl_cache = {}


def griffinlim_case(i, n_iter, dtype=np.float64):
    """the restatement's output for case i (cached: the GPU tests share it)"""
    key = (i, n_iter, np.dtype(dtype).name)
    if key not in _gl_cache:
        c = case(i)
        out = griffinlim(c['mag'], c['angles'], n_iter, c['hop'], dtype)
        out.setflags(write=False)
        _gl_cache[key] = out
    return _gl_cache[key]
