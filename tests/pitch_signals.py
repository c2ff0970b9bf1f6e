"""Signals with a known F0 and seeded candidate tables for the pitch tracker's tests (CPU and GPU); plain numpy, no import from ttscube_amd."""
import functools

import numpy as np

from tests import pitch_reference as R

SR, HOP, FMIN, FMAX = 24000, 240, 60, 400
EDGE_S, GAP_S, VOICED_S = 0.080, 0.100, 1.4


def _harmonics(f_per_sample, sr):
    phase = 2.0 * np.pi * np.cumsum(f_per_sample) / sr
    return sum(np.sin(h * phase) / h for h in range(1, 9))


def utterance(f_start, f_end, sr=SR):
    """80 ms of digital silence, 0.7 s voiced, a 100 ms silent gap, 0.7 s voiced, 80 ms of silence; F0 runs linearly from f_start to f_end over the
    voiced samples.  -> x float32, truth [L] (F0 per sample, 0 in silence)"""
    nv = int(VOICED_S * sr)
    f = f_start + (f_end - f_start) * np.arange(nv) / nv
    v = _harmonics(f, sr)
    v = 0.3 * v / np.abs(v).max()
    edge, gap, half = np.zeros(int(EDGE_S * sr)), np.zeros(int(GAP_S * sr)), nv // 2
    x = np.concatenate([edge, v[:half], gap, v[half:], edge])
    truth = np.concatenate([edge, f[:half], gap, f[half:], edge])
    return x.astype(np.float32), truth


@functools.lru_cache(maxsize=None)
def known_answer_batch():
    """the glide 90 -> 250 Hz and the steady 120 Hz: x [2, L], lengths, truth [2, L]"""
    a, ta = utterance(90.0, 250.0)
    b, tb = utterance(120.0, 120.0)
    return np.stack([a, b]), [a.shape[0], b.shape[0]], np.stack([ta, tb])


def frame_classes(truth, sr=SR, hop=HOP, fmin=FMIN, fmax=FMAX):
    """per frame: kind (1 = the analysis span [m, m + n + kmax) lies wholly inside one voiced stretch, 0 = wholly inside silence, -1 = it straddles a
    boundary) and the true F0 at the middle of the two windows that are correlated at the true lag"""
    n, _, kmax, _ = R.params(sr, fmin, fmax)
    F = truth.shape[0] // hop
    kind, f_true = np.full((F,), -1), np.zeros((F,))
    voiced = truth > 0
    for t in range(F):
        m = t * hop
        span = np.zeros((n + kmax,), bool)
        got = voiced[m:m + n + kmax]
        span[:got.shape[0]] = got
        if span.all():
            kind[t] = 1
            f_mid = truth[m + n // 2]
            f_true[t] = truth[m + n // 2 + int(round(sr / (2.0 * f_mid)))]
        elif not span.any():
            kind[t] = 0
    return kind, f_true


def check_known_answer(f0, truth):
    """the assertions of the end-to-end check on one utterance's track; -> (kind, number of scored frames)"""
    kind, f_true = frame_classes(truth)
    assert f0.shape[0] == kind.shape[0]
    assert np.mean(kind < 0) <= 0.15, 'too many frames straddle a boundary: %.3f' % np.mean(kind < 0)
    v = kind == 1
    assert v.sum() > 0 and (kind == 0).sum() > 0
    assert np.all(f0[v] > 0), 'unvoiced inside a voiced stretch at frames %s' % np.nonzero(v & (f0 <= 0))[0][:10]
    rel = np.abs(f0[v] - f_true[v]) / f_true[v]
    assert rel.max() <= 0.02, 'F0 off by %.4f at frame %d' % (rel.max(), np.nonzero(v)[0][np.argmax(rel)])
    assert np.all(f0[kind == 0] == 0), 'voiced inside silence'
    return kind, int((kind >= 0).sum())


def disagreement(f_a, f_b, kind):
    """share of the scored frames on which two tracks differ in voicing or by more than 1 Hz"""
    s = kind >= 0
    bad = ((f_a > 0) != (f_b > 0)) | (np.abs(f_a - f_b) > 1.0)
    return float(np.mean(bad[s]))


# ---- injected candidate tables (check b) -------------------------------------------------------------------------------------------------------------

TABLE_FRAMES = (1, 2, 37) * 4 + (37,)     # the last utterance has 20 candidates in every frame
TABLE_KMIN, TABLE_KMAX = 60, 400


@functools.lru_cache(maxsize=None)
def candidate_tables(seed=20240):
    """-> dict of float32 / int32 arrays padded to Fmax = 37 (rows past an utterance's frames are zero) and nframes.  Lags are distinct within a frame, so
    a state can be read back from f0 = sr / lag."""
    rng = np.random.default_rng(seed)
    B, Fm = len(TABLE_FRAMES), max(TABLE_FRAMES)
    lag = np.zeros((B, Fm, R.N_CANDS), np.float32)
    val = np.zeros((B, Fm, R.N_CANDS), np.float32)
    ncand = np.zeros((B, Fm), np.int32)
    maxphi = np.zeros((B, Fm), np.float32)
    rms = np.zeros((B, Fm), np.float32)
    for b, F in enumerate(TABLE_FRAMES):
        for t in range(F):
            nc = R.N_CANDS if b == B - 1 else int(rng.integers(0, R.N_CANDS + 1))
            if b != B - 1 and t == 0 and b % 3 == 0:
                nc = (0, R.N_CANDS, 1, 7)[b // 3]              # the one-frame utterances cover both ends of the range
            ncand[b, t] = nc
            lag[b, t, :nc] = rng.uniform(TABLE_KMIN + 1, TABLE_KMAX - 1, nc)
            val[b, t, :nc] = np.sort(rng.uniform(0.3, 1.0, nc))[::-1]
            maxphi[b, t] = val[b, t, 0] if nc else rng.uniform(0.0, 0.3)
            rms[b, t] = 0.05 * 4.0 ** rng.uniform(0.0, 1.0)
    return dict(lag=lag, val=val, ncand=ncand, maxphi=maxphi, rms=rms, nframes=np.array(TABLE_FRAMES, np.int32))


@functools.lru_cache(maxsize=None)
def table_solutions():
    """per utterance of candidate_tables(): float64 optimum D_opt, its path, the margin of the best final state over the next, and whether the float32
    restatement walks the same path"""
    tb = candidate_tables()
    out = []
    for b, F in enumerate(TABLE_FRAMES):
        a = [tb[k][b, :F] for k in ('lag', 'val', 'ncand', 'maxphi', 'rms')]
        _, p64, final = R.track(*a, TABLE_KMAX, SR, np.float64)
        _, p32, _ = R.track(*a, TABLE_KMAX, SR, np.float32)
        fs = np.sort(final[np.isfinite(final)])
        margin = float(fs[1] - fs[0]) if fs.shape[0] > 1 else np.inf
        out.append(dict(D_opt=float(fs[0]), path=p64, margin=margin, same32=bool(np.array_equal(p64, p32)), args=a))
    return out


def states_from_f0(f0, lag_rows, ncand_row, sr=SR):
    """the state per frame behind a float32 f0 row: the candidate whose float32 sr / lag equals it, 20 where f0 == 0"""
    path = np.full((f0.shape[0],), R.UNVOICED, np.int64)
    for t, v in enumerate(f0):
        if v != 0:
            hit = np.nonzero(np.float32(sr) / lag_rows[t, :int(ncand_row[t])].astype(np.float32) == np.float32(v))[0]
            assert hit.shape[0] == 1, 'frame %d: f0 %r matches %d candidates' % (t, v, hit.shape[0])
            path[t] = hit[0]
    return path
