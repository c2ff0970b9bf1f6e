"""numpy statements of the forced aligner (ttscube_amd/io_utils/forced_align.py, csrc/forced_align.hip) for its CPU and GPU tests; no import from
ttscube_amd.

logmel10()        this project's log10-mel (centred frames, reflect padding, periodic Hann, Slaney mel basis) in float64
features()        cepstra 0 .. 12 of ln(10) * log-mel and their centred deltas, the index clamped to 0 .. nframes - 1
build_lattice()   positions, skips, start / final flags of one utterance
viterbi()         the search of ttsc_fa_viterbi in float64, or in float32 with every operation rounded on its own and the squared distances summed
                  in ascending d — what the kernel computes.  Predecessors j, j - 1, skip[j], taken in that order with strict >; the end is the
                  final position with the largest score, ties to the lowest index.
path_score64()    the float64 score of any path
brute_force()     the optimum over all paths by enumeration (tiny sizes)
accumulate()      the statistics of ttsc_fa_accumulate in the stated grouping: per (utterance, position) over ascending t, per model state over
                  ascending (b, position), the batch total added once to the running tables
global_stats(), reestimate(), kernel_model(), flat_alignment(), fit()    Viterbi re-estimation from the flat start
intervals()       word and phone intervals of an alignment"""
import math

import numpy as np

SAMPLE_RATE, HOP, N_FFT, N_MELS, N_CEP = 24000, 240, 1024, 80, 13
VAR_FLOOR, VAR_TINY = 0.01, 1e-8


# ---- features ----------------------------------------------------------------------------------------------------------------------------------------

def mel_filterbank(sr=SAMPLE_RATE, n_fft=N_FFT, n_mels=N_MELS):
    """the Slaney-scale, slaney-normalised triangular basis over [0, sr / 2]: float64 [n_mels, n_fft / 2 + 1]"""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    to_mel = lambda f: np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)
    to_hz = lambda m: np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    freqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = to_hz(np.linspace(to_mel(np.float64(0.0)), to_mel(np.float64(sr / 2.0)), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - freqs[None, :]
    w = np.maximum(0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def logmel10(x, hop=HOP, n_fft=N_FFT):
    """x [L] -> [L // hop, 80] float64: log10(max(1e-5, mel basis . |STFT|)) of centred, reflect-padded frames"""
    x = np.asarray(x, np.float64)
    F = len(x) // hop
    xp = np.pad(x, n_fft // 2, mode='reflect')
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    frames = np.stack([xp[t * hop:t * hop + n_fft] for t in range(F)]) * win if F else np.zeros((0, n_fft))
    mag = np.abs(np.fft.rfft(frames, axis=1))
    return np.log10(np.maximum(1e-5, mag @ mel_filterbank(n_fft=n_fft).T))


def dct_table(n_coef=N_CEP, n_bins=N_MELS):
    """rows 0 .. n_coef - 1 of the orthonormal DCT-II over n_bins points, float64"""
    c = np.arange(n_coef, dtype=np.float64)[:, None]
    m = np.arange(n_bins, dtype=np.float64)[None, :]
    t = math.sqrt(2.0 / n_bins) * np.cos(math.pi * c * (m + 0.5) / n_bins)
    t[0] = math.sqrt(1.0 / n_bins)
    return t


def deltas(c):
    """[T, K] -> (c[t+1] - c[t-1]) / 2 with the index clamped to 0 .. T - 1, in c's own precision"""
    T = c.shape[0]
    t = np.arange(T)
    return ((c[np.minimum(t + 1, T - 1)] - c[np.maximum(t - 1, 0)]) * c.dtype.type(0.5)).astype(c.dtype)


def features(mel10):
    """[T, 80] log10-mel -> [T, 26] float64"""
    c = np.asarray(mel10, np.float64) @ (math.log(10.0) * dct_table(N_CEP, mel10.shape[1])).T
    return np.concatenate([c, deltas(c)], axis=1)


# ---- lattice -----------------------------------------------------------------------------------------------------------------------------------------

def build_lattice(prons, n_sub):
    """prons: phone ids (>= 1, 0 = silence) per word; -> dict(state, skip, start, final, word, unit, phone) over the positions.  Units: the
    sequence sil, phones of word 0, sil, phones of word 1, ..., sil (words without phones left out); each unit is n_sub positions."""
    units = []                                                    # (phone id, word index)
    for w, ph in enumerate(prons):
        if len(ph):
            units.append((0, -1))
            units += [(int(p), w) for p in ph]
    if not units:
        return {k: np.zeros((0,), np.uint8 if k in ('start', 'final') else np.int32) for k in ('state', 'skip', 'start', 'final', 'word', 'unit', 'phone')}
    units.append((0, -1))
    S = len(units) * n_sub
    lat = {'state': np.zeros(S, np.int32), 'skip': np.full(S, -1, np.int32), 'start': np.zeros(S, np.uint8), 'final': np.zeros(S, np.uint8),
           'word': np.zeros(S, np.int32), 'unit': np.zeros(S, np.int32), 'phone': np.zeros(S, np.int32)}
    for u, (ph, w) in enumerate(units):
        for s in range(n_sub):
            j = u * n_sub + s
            lat['state'][j], lat['word'][j], lat['unit'][j], lat['phone'][j] = ph * n_sub + s, w, u, ph
        if ph == 0 and 0 < u < len(units) - 1:
            lat['skip'][(u + 1) * n_sub] = u * n_sub - 1        # over an inner silence
    lat['start'][0] = lat['start'][n_sub] = 1
    lat['final'][S - 1] = lat['final'][S - n_sub - 1] = 1
    return lat


# ---- search ------------------------------------------------------------------------------------------------------------------------------------------

def emissions(x, state, mean, ivar, cst, dt):
    """e [T, S] in dt: cst[m] - 0.5 sum_d (x[d] - mean[m][d])^2 ivar[m][d], the sum in ascending d, every operation rounded on its own"""
    x, mean, ivar, cst = (np.asarray(a).astype(dt) for a in (x, mean, ivar, cst))
    acc = np.zeros((x.shape[0], len(state)), dt)
    for d in range(x.shape[1]):
        df = (x[:, d][:, None] - mean[state, d][None, :]).astype(dt)
        acc = (acc + ((df * df).astype(dt) * ivar[state, d][None, :]).astype(dt)).astype(dt)
    return (cst[state][None, :] - (dt(0.5) * acc).astype(dt)).astype(dt)


def viterbi(x, lat, mean, ivar, cst, dt=np.float64):
    """x [T, D], lat: state / skip / start / final over S positions -> (align int32 [T] or None, score as dt, ok)"""
    state, skip = np.asarray(lat['state'], np.int64), np.asarray(lat['skip'], np.int64)
    T, S = x.shape[0], len(state)
    if T == 0 or S == 0:
        return None, dt(0), 0
    with np.errstate(invalid='ignore', over='ignore'):
        e = emissions(x, state, mean, ivar, cst, dt)
        ninf = dt(-np.inf)
        v = np.where(np.asarray(lat['start']) != 0, e[0], ninf).astype(dt)
        bp = np.zeros((T, S), np.int8)
        for t in range(1, T):
            best, code = v.copy(), np.zeros(S, np.int8)
            left = np.concatenate([[ninf], v[:-1]]).astype(dt)
            jump = np.where(skip >= 0, v[np.maximum(skip, 0)], ninf).astype(dt)
            m = left > best
            best, code = np.where(m, left, best), np.where(m, 1, code)
            m = jump > best
            best, code = np.where(m, jump, best), np.where(m, 2, code)
            v = (e[t] + best).astype(dt)
            bp[t] = code
    best, bi = ninf, -1
    for j in np.nonzero(np.asarray(lat['final']) != 0)[0]:
        if v[j] > best:
            best, bi = v[j], int(j)
    if bi < 0 or not best < np.inf:
        return None, dt(0), 0
    align = np.zeros(T, np.int32)
    j = bi
    for t in range(T - 1, -1, -1):
        align[t] = j
        if t > 0:
            j = j if bp[t, j] == 0 else (j - 1 if bp[t, j] == 1 else int(skip[j]))
    return align, dt(best), 1


def path_ok(align, lat):
    """the path starts on a start position, ends on a final one and every step is a stay, an advance by one or the skip"""
    if not (lat['start'][align[0]] and lat['final'][align[-1]]):
        return False
    return all(b == a or b == a + 1 or (lat['skip'][b] >= 0 and lat['skip'][b] == a) for a, b in zip(align[:-1], align[1:]))


def path_score64(x, align, lat, mean, ivar, cst):
    e = emissions(x, np.asarray(lat['state'], np.int64), mean, ivar, cst, np.float64)
    return float(e[np.arange(len(align)), align].sum())


def brute_force(x, lat, mean, ivar, cst):
    """the largest float64 score over every path by enumeration, or None"""
    e = emissions(x, np.asarray(lat['state'], np.int64), mean, ivar, cst, np.float64)
    T, S = e.shape
    succ = [[j] + ([j + 1] if j + 1 < S else []) + [k for k in range(S) if lat['skip'][k] == j] for j in range(S)]

    def go(t, j):
        if t == T - 1:
            return e[t, j] if lat['final'][j] else None
        rest = [r for r in (go(t + 1, k) for k in succ[j]) if r is not None]
        return e[t, j] + max(rest) if rest else None

    tops = [r for r in (go(0, j) for j in range(S) if lat['start'][j]) if r is not None]
    return float(max(tops)) if tops else None


# ---- statistics and the model ------------------------------------------------------------------------------------------------------------------------

def accumulate(feats, aligns, oks, lattices, count, total, sumsq):
    """feats: [T_b, D] float32 per utterance, aligns: positions per frame (or None), oks, lattices; adds into the float64 tables count [M],
    total [M, D], sumsq [M, D] (in place) in the order ttsc_fa_accumulate states"""
    M, D = total.shape
    bs, bq, bc = np.zeros((M, D)), np.zeros((M, D)), np.zeros(M)
    for b, (x, al, ok, lat) in enumerate(zip(feats, aligns, oks, lattices)):
        if not ok:
            continue
        x = np.asarray(x).astype(np.float64)
        for p in range(len(lat['state'])):
            frames = np.nonzero(np.asarray(al) == p)[0]
            if len(frames) == 0:
                continue
            s, q = np.zeros(D), np.zeros(D)
            for t in frames:
                s = s + x[t]
                q = q + x[t] * x[t]
            m = int(lat['state'][p])
            bs[m], bq[m], bc[m] = bs[m] + s, bq[m] + q, bc[m] + float(len(frames))
    count += bc
    total += bs
    sumsq += bq


def global_stats(count, total, sumsq):
    n = count.sum()
    mean = total.sum(axis=0) / n
    return mean, sumsq.sum(axis=0) / n - mean * mean


def reestimate(count, total, sumsq, prev_mean, prev_var, floor):
    mean, var = prev_mean.copy(), prev_var.copy()
    for m in np.nonzero(count > 0)[0]:
        mu = total[m] / count[m]
        mean[m] = mu
        var[m] = np.maximum(sumsq[m] / count[m] - mu * mu, floor)
    return mean, var


def kernel_model(mean, var, dt=np.float32):
    D = mean.shape[1]
    cst = -0.5 * (D * math.log(2.0 * math.pi) + np.log(var).sum(axis=1))
    return mean.astype(dt), (1.0 / var).astype(dt), cst.astype(dt)


def flat_alignment(T, S):
    """frame t on position t * S // T, or None where T < S or S == 0"""
    if S == 0 or T < S:
        return None
    return ((np.arange(T, dtype=np.int64) * S) // T).astype(np.int32)


def fit(feats, lattices, M, iterations, dt=np.float32, batch=None):
    """Viterbi re-estimation from the flat start; batch: utterances per accumulate call (the running tables take one batch total at a time).
    -> list, one entry for the flat start and one per iteration: dict(mean, var [M, D] float64 after that step, aligns, oks, score, frames)"""
    D = feats[0].shape[1]
    B = len(feats)
    batch = batch or B

    def stats(aligns, oks):
        count, total, sumsq = np.zeros(M), np.zeros((M, D)), np.zeros((M, D))
        for s in range(0, B, batch):
            accumulate(feats[s:s + batch], aligns[s:s + batch], oks[s:s + batch], lattices[s:s + batch], count, total, sumsq)
        return count, total, sumsq

    aligns = [flat_alignment(x.shape[0], len(l['state'])) for x, l in zip(feats, lattices)]
    oks = [int(a is not None) for a in aligns]
    c, s, q = stats(aligns, oks)
    gmean, gvar = global_stats(c, s, q)
    floor = np.maximum(VAR_FLOOR * gvar, VAR_TINY)
    mean, var = reestimate(c, s, q, np.tile(gmean, (M, 1)), np.tile(np.maximum(gvar, floor), (M, 1)), floor)
    steps = [dict(mean=mean, var=var, aligns=aligns, oks=oks, score=None, frames=int(sum(x.shape[0] for x, k in zip(feats, oks) if k)))]
    for _ in range(iterations):
        km = kernel_model(mean, var, dt)
        res = [viterbi(np.asarray(x).astype(dt), l, *km, dt=dt) for x, l in zip(feats, lattices)]
        aligns, oks = [r[0] for r in res], [r[2] for r in res]
        mean, var = reestimate(*stats(aligns, oks), mean, var, floor)
        steps.append(dict(mean=mean, var=var, aligns=aligns, oks=oks, score=float(sum(float(r[1]) for r in res if r[2])),
                          frames=int(sum(x.shape[0] for x, k in zip(feats, oks) if k))))
    return steps


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------------------

def intervals(align, lat, words, phones, hop, sample_rate, duration):
    """-> (word intervals, phone intervals): lists of (mark, start s, end s); a boundary between frames t - 1 and t is at (t - 0.5) hop /
    sample_rate, the first at 0, the last at duration; silence has the empty mark; a unit without a frame writes nothing"""
    unit = lat['unit'][align]
    cuts = [0] + [t for t in range(1, len(align)) if unit[t] != unit[t - 1]]
    edge = [0.0] + [(t - 0.5) * hop / sample_rate for t in cuts[1:]] + [float(duration)]
    ph = [('' if lat['phone'][align[t]] == 0 else phones[lat['phone'][align[t]]], edge[i], edge[i + 1]) for i, t in enumerate(cuts)]
    wd = []
    for i, t in enumerate(cuts):
        w = int(lat['word'][align[t]])
        if wd and w >= 0 and wd[-1][3] == w:
            wd[-1][2] = edge[i + 1]
        else:
            wd.append(['' if w < 0 else words[w], edge[i], edge[i + 1], w])
    return [tuple(r[:3]) for r in wd], ph
