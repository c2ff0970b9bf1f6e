"""float64 statement of the loudness meter (csrc/loudness.hip, io_utils/loudness.py): ITU-R BS.1770-4 integrated loudness of a mono row at any
rate, the 4x true peak and the static gain, written out literally with numpy and a plain recursion.

    K-weighting      two biquads re-designed at sr from the analogue prototypes (k_weighting), transposed direct form II, float64
    sub-block k      sum of y^2 over samples [k S, (k+1) S), S = sr / 10
    block j          z_j = (sub-blocks j .. j+3) / (4 S);  a row of 0 < L < 4 S samples: ONE block, mean(y^2) over the row;  L = 0: none
    gates (strict)   z_j > 10^((-70 + 0.691)/10), then also z_j > 0.1 mean(z over the first gate)
    L                -0.691 + 10 log10(mean z over both gates);  -inf and `silent` when no block passes
    true peak        max |y| of y[n] = sum_i x[i] h[n - 4 i + 40], n < 4 L, h = fl32(design_filter(4, 1)) of tests/resample_reference.py
    gain             min(sqrt(10^((target + 0.691)/10) / zbar), 10^(peak_db/20) / max(sample peak, true peak)[, 10^(max_gain_db/20)]) as float32

`chunked_sub_energies` is a numpy emulation of how the kernels split the recursion (CHUNK samples per thread from a zero state, states joined
with powers of the 4x4 step matrix by a Hillis-Steele scan over a TILE, tiles joined one after the other, sums in thread then tile order): the
distance between it and the sequential recursion is what float64 rounding alone does to the scheme."""
import math

import numpy as np

from tests import resample_reference

ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
TABLE_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])     # the Recommendation's printed coefficients


def k_weighting(sr):
    """-> [2, 6] float64 (b0 b1 b2 1 a1 a2) of the shelf and the high-pass"""
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], dtype=np.float64)


def kfilter(x, sr, sos=None):
    """the plain recursion, one sample after the other -> y float64"""
    (b0, b1, b2, _, a1, a2), (c0, c1, c2, _, d1, d2) = (k_weighting(sr) if sos is None else sos).tolist()
    s0 = s1 = s2 = s3 = 0.0
    xs = np.asarray(x, dtype=np.float64).tolist()
    y = [0.0] * len(xs)
    for n, v in enumerate(xs):
        u = b0 * v + s0
        s0 = (b1 * v - a1 * u) + s1
        s1 = b2 * v - a2 * u
        w = c0 * u + s2
        s2 = (c1 * u - d1 * w) + s3
        s3 = c2 * u - d2 * w
        y[n] = w
    return np.array(y, dtype=np.float64)


def kfilter_fast(x, sr):
    """the same filter by scipy.signal.sosfilt (CPU tests of long sequences; test_loudness_cpu.py holds the two together)"""
    from scipy.signal import sosfilt
    return sosfilt(k_weighting(sr), np.asarray(x, dtype=np.float64))


def sub_energies(y, sr):
    S = sr // 10
    L = len(y)
    q = np.asarray(y, dtype=np.float64) ** 2
    return np.array([q[k * S:min((k + 1) * S, L)].sum() for k in range(-(-L // S))], dtype=np.float64)


def blocks(sub, L, sr):
    """-> z float64 [number of blocks]"""
    S = sr // 10
    if L == 0:
        return np.zeros(0)
    if L < 4 * S:
        return np.array([sub.sum() / L])
    return np.array([(((sub[j] + sub[j + 1]) + sub[j + 2]) + sub[j + 3]) / (4.0 * S) for j in range(L // S - 3)])


def gate(z):
    """-> dict(zbar, lufs, blocks, gated, silent, abs_mask, rel_thresh)"""
    a = z > ABS_GATE
    out = {'blocks': int(z.size), 'gated': 0, 'silent': True, 'zbar': 0.0, 'lufs': -np.inf, 'abs_mask': a, 'rel_thresh': None}
    if not a.any():
        return out
    rel = 0.1 * z[a].mean()
    m = a & (z > rel)
    out['rel_thresh'] = rel
    if not m.any():
        return out
    zbar = z[m].mean()
    out.update(gated=int(m.sum()), silent=False, zbar=float(zbar), lufs=-0.691 + 10.0 * math.log10(zbar))
    return out


def gate_margin(z):
    """smallest relative distance of a block from either threshold (inf without blocks)"""
    if z.size == 0:
        return np.inf
    g = gate(z)
    d = np.abs(z / ABS_GATE - 1.0).min()
    if g['rel_thresh'] is not None:
        d = min(d, np.abs(z[g['abs_mask']] / g['rel_thresh'] - 1.0).min())
    return d


def measure(x, sr, fast=False):
    """x: 1-D -> dict(sub, z, zbar, lufs, blocks, gated, silent, sample_peak, true_peak)"""
    x = np.asarray(x, dtype=np.float64)
    y = kfilter_fast(x, sr) if fast and x.size else kfilter(x, sr)
    sub = sub_energies(y, sr)
    z = blocks(sub, x.size, sr)
    out = gate(z)
    out.update(sub=sub, z=z, sample_peak=float(np.abs(x).max()) if x.size else 0.0, true_peak=true_peak(x)[0])
    return out


TP_TAPS = 21            # taps per phase of the 81-tap 4x filter


def tp_filter():
    return resample_reference.design_filter(4, 1).astype(np.float32).astype(np.float64)


def true_peak(x):
    """-> (max |y| in float64, bound of a float32 evaluation: (taps per phase + 2) 2^-24 max over phases of sum |h| times max |x|)"""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0, 0.0
    h = tp_filter()
    up = np.zeros(4 * x.size)
    up[::4] = x
    y = np.convolve(up, h)[40:40 + 4 * x.size]
    hsum = max(np.abs(h[p::4]).sum() for p in range(4))
    return float(np.abs(y).max()), (TP_TAPS + 2) * 2.0 ** -24 * hsum * float(np.abs(x).max())


def gain(zbar, peak, silent, target, peak_db=-1.0, max_gain_db=None):
    """-> (float32 gain, peak_limited)"""
    if silent:
        return np.float32(1.0), False
    g = math.sqrt(10.0 ** ((target + 0.691) / 10.0) / zbar)
    limited = False
    if peak > 0.0 and 10.0 ** (peak_db / 20.0) / peak < g:
        g, limited = 10.0 ** (peak_db / 20.0) / peak, True
    if max_gain_db is not None:
        g = min(g, 10.0 ** (max_gain_db / 20.0))
    return np.float32(g), limited


def apply_gain(x, g):
    return np.float32(g) * np.asarray(x, dtype=np.float32)


# ---- numpy emulation of the chunked scheme ---------------------------------------------------------------------------------------------------
def _step(sos, s, v):
    (b0, b1, b2, _, a1, a2), (c0, c1, c2, _, d1, d2) = sos
    u = b0 * v + s[0]
    n0 = (b1 * v - a1 * u) + s[1]
    n1 = b2 * v - a2 * u
    w = c0 * u + s[2]
    n2 = (c1 * u - d1 * w) + s[3]
    n3 = c2 * u - d2 * w
    return w, [n0, n1, n2, n3]


def _affine(M, v, w):
    return [(((M[i][0] * v[0] + M[i][1] * v[1]) + M[i][2] * v[2]) + M[i][3] * v[3]) + w[i] for i in range(4)]


def _powers(sos, chunk, levels):
    A = np.zeros((4, 4))
    for i in range(4):
        e = [0.0] * 4
        e[i] = 1.0
        A[:, i] = _step(sos, e, 0.0)[1]
    M = np.linalg.matrix_power(A, 1)
    for _ in range(int(math.log2(chunk))):
        M = M @ M
    out = [M]
    for _ in range(levels):
        out.append(out[-1] @ out[-1])
    return out


def chunked_sub_energies(x, sr, chunk, tile):
    """sub-block energies of x the way the kernels compute them, in numpy float64 -> (sub, y)"""
    x = np.asarray(x, dtype=np.float64)
    L, S, T = x.size, sr // 10, tile // chunk
    if L == 0:
        return np.zeros(0), np.zeros(0)
    levels = int(math.log2(T))
    assert 1 << levels == T and chunk <= S
    sos = k_weighting(sr).tolist()
    P = _powers(sos, chunk, levels)
    nt = -(-L // tile)
    xp = np.zeros(nt * tile)
    xp[:L] = x
    xp = xp.reshape(nt, T, chunk)

    def run(s_in, want_y=False):
        s = [a.copy() for a in s_in]
        ys = []
        for j in range(chunk):
            w, s = _step(sos, s, xp[:, :, j])
            if want_y:
                ys.append(w)
        return s, ys

    def scan(f):
        for k in range(levels):
            off = 1 << k
            g = _affine(P[k], [a[:, :-off] for a in f], [a[:, off:] for a in f])
            f = [np.concatenate([a[:, :off], b], axis=1) for a, b in zip(f, g)]
        return f

    zero = [np.zeros((nt, T)) for _ in range(4)]
    F = scan(run(zero)[0])
    Sin = np.zeros((nt, 4))
    for t in range(nt - 1):
        Sin[t + 1] = _affine(P[levels], list(Sin[t]), [F[i][t, T - 1] for i in range(4)])
    first = [a.copy() for a in zero]
    for i in range(4):
        first[i][:, 0] = Sin[:, i]
    F = scan(run(first)[0])
    s_in = [np.concatenate([first[i][:, :1], F[i][:, :-1]], axis=1) for i in range(4)]
    _, ys = run(s_in, want_y=True)
    y = np.stack(ys, axis=2).reshape(-1)[:L]

    q = (y * y).tolist()
    nchunks = -(-L // chunk)
    lo, hi = [0.0] * nchunks, [0.0] * nchunks
    for c in range(nchunks):
        c0 = c * chunk
        nb = (c0 // S + 1) * S - c0
        a = b = 0.0
        for j in range(min(chunk, L - c0)):
            if j < nb:
                a = a + q[c0 + j]
            else:
                b = b + q[c0 + j]
        lo[c], hi[c] = a, b
    nsub = -(-L // S)
    sub = np.zeros(nsub)
    for k in range(nsub):
        a0, a1 = k * S, min((k + 1) * S, L)
        acc = 0.0
        for t in range(a0 // tile, (a1 - 1) // tile + 1):
            t0, tend = t * tile, min((t + 1) * tile, L)
            p0, p1 = max(a0, t0), min(a1, tend)
            part = 0.0
            for c in range(p0 // chunk, (p1 - 1) // chunk + 1):
                part = part + (lo[c] if (c * chunk) // S == k else hi[c])
            acc = acc + part
        sub[k] = acc
    return sub, y


# ---- signals -------------------------------------------------------------------------------------------------------------------------------
def response_at(f, sr):
    """|H(e^jw)| of the K-weighting at f Hz"""
    z = np.exp(-2j * np.pi * f / sr)
    h = 1.0
    for b0, b1, b2, _, a1, a2 in k_weighting(sr):
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return abs(h)


def tone_sequence(levels_and_seconds, sr, f=1000.0):
    """1 kHz tone whose segments read the stated LUFS each: amplitude from the filter's own response, a^2 / 2 |H|^2 = 10^((L + 0.691) / 10)"""
    H = response_at(f, sr)
    out, n0 = [], 0
    for level, sec in levels_and_seconds:
        n = int(round(sec * sr))
        a = math.sqrt(2.0 * 10.0 ** ((level + 0.691) / 10.0)) / H
        out.append(a * np.sin(2.0 * np.pi * f * (n0 + np.arange(n)) / sr))
        n0 += n
    return np.concatenate(out)


TECH3341 = {3: [(-36, 10), (-23, 60), (-36, 10)],
            4: [(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)],
            5: [(-26, 20), (-20, 20.1), (-26, 20)]}
