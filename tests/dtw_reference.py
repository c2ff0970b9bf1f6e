"""numpy statements of the dev-set evaluation (ttscube_amd/io_utils/evaluate.py, csrc/dtw.hip) for its CPU and GPU tests; no import from ttscube_amd.

dtw()            the dynamic program of ttsc_dtw_align in float64, or in float32 with every operation rounded on its own and the sum of squares taken
                 in ascending k — what the kernel computes.  Steps (1,1), (1,0), (0,1), unweighted; ties go to the diagonal, then to (i-1, j), then
                 to (i, j-1): strict <, taken in that order.
path_cost64()    the float64 cost of any path
brute_force()    the optimum over all monotone paths by enumeration (tiny sizes)
path_metrics()   the scores of evaluate.path_metrics from one pair's path
mel_cepstra()    the DCT-II of evaluate.mel_cepstra in float64 or float32"""
import math

import numpy as np

MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)


def local_cost(a, b, dt=np.float64):
    """d [Na, Nb] = sqrt(sum_k (a[i,k] - b[j,k])^2) in dt, the sum in ascending k"""
    a, b = np.asarray(a).astype(dt), np.asarray(b).astype(dt)
    s = np.zeros((a.shape[0], b.shape[0]), dt)
    for k in range(a.shape[1]):
        df = (a[:, k][:, None] - b[:, k][None, :]).astype(dt)
        s = (s + (df * df).astype(dt)).astype(dt)
    return np.sqrt(s).astype(dt)


def dtw(a, b, dt=np.float64):
    """-> (D at the end cell as dt, path int64 [n, 2] from (0, 0) to (Na - 1, Nb - 1))"""
    d = local_cost(a, b, dt)
    Na, Nb = d.shape
    D = np.zeros((Na, Nb), dt)
    bp = np.zeros((Na, Nb), np.int8)
    inf = dt(np.inf)
    for i in range(Na):
        for j in range(Nb):
            if i == 0 and j == 0:
                D[0, 0] = d[0, 0]
                continue
            best, w = (D[i - 1, j - 1] if i > 0 and j > 0 else inf), 0
            up = D[i - 1, j] if i > 0 else inf
            left = D[i, j - 1] if j > 0 else inf
            if up < best:
                best, w = up, 1
            if left < best:
                best, w = left, 2
            D[i, j] = dt(d[i, j] + best)
            bp[i, j] = w
    i, j = Na - 1, Nb - 1
    path = [(i, j)]
    while i or j:
        w = bp[i, j] if i and j else (2 if i == 0 else 1)
        if w != 2:
            i -= 1
        if w != 1:
            j -= 1
        path.append((i, j))
    return D[-1, -1], np.array(path[::-1], dtype=np.int64)


def path_cost64(a, b, path):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    path = np.asarray(path)
    return float(np.sqrt(((a[path[:, 0]] - b[path[:, 1]]) ** 2).sum(axis=1)).sum())


def brute_force(a, b):
    """the smallest float64 cost over every monotone path, by enumeration"""
    d = local_cost(a, b, np.float64)
    Na, Nb = d.shape

    def go(i, j):
        if i == Na - 1 and j == Nb - 1:
            return d[i, j]
        nxt = []
        if i + 1 < Na and j + 1 < Nb:
            nxt.append(go(i + 1, j + 1))
        if i + 1 < Na:
            nxt.append(go(i + 1, j))
        if j + 1 < Nb:
            nxt.append(go(i, j + 1))
        return d[i, j] + min(nxt)

    return float(go(0, 0))


def warp_pair(rng, Na, Nb, K, noise=0.3):
    """a ~ N(0, 1) [Na, K]; b [Nb, K] = a linearly warped copy of a plus noise * N(0, 1); float32"""
    a = rng.standard_normal((Na, K)).astype(np.float32)
    idx = np.clip(np.round(np.linspace(0, Na - 1, Nb)).astype(int), 0, Na - 1)
    b = (a[idx] + noise * rng.standard_normal((Nb, K))).astype(np.float32)
    return a, b


def exact_warp(rng, Na=40, extra=25, K=24):
    """a [Na, K], a non-decreasing surjective w [Na + extra] onto range(Na), b = a[w]: the optimal path is (w[j], j) at cost exactly 0"""
    a = rng.standard_normal((Na, K)).astype(np.float32)
    w = np.sort(np.concatenate([np.arange(Na), rng.integers(0, Na, extra)]))
    return a, a[w].copy(), w


def path_metrics(path, cost, f0_ref, f0_syn, len_ref, len_syn):
    """one pair: path [n, 2] over (reference frame, synthesized frame), cost = D at the end cell, F0 tracks in Hz (0 = unvoiced).
    -> (scores, sums): the scores of evaluate.path_metrics, and the sums a corpus pools"""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    n = int(path.shape[0])
    fr = np.asarray(f0_ref, np.float64)[path[:, 0]]
    fs = np.asarray(f0_syn, np.float64)[path[:, 1]]
    vr, vs = fr > 0, fs > 0
    both = vr & vs
    nb = int(both.sum())
    dhz = fs[both] - fr[both]
    dct = 1200.0 * np.log2(fs[both] / fr[both])
    gross = int((np.abs(fs[both] / fr[both] - 1.0) > 0.2).sum())
    sums = dict(cost=float(cost), n_path=n, n_both_voiced=nb, sq_hz=float((dhz ** 2).sum()), sq_cents=float((dct ** 2).sum()), gross=gross,
                vdiff=int((vr != vs).sum()), len_ref=int(len_ref), len_syn=int(len_syn))
    return scores_from_sums(sums), sums


def scores_from_sums(s):
    nan = float('nan')
    n, nb = s['n_path'], s['n_both_voiced']
    return dict(mcd_db=MCD_SCALE * s['cost'] / n if n else nan,
                f0_rmse_hz=math.sqrt(s['sq_hz'] / nb) if nb else nan,
                f0_rmse_cents=math.sqrt(s['sq_cents'] / nb) if nb else nan,
                gpe=s['gross'] / nb if nb else nan,
                vde=s['vdiff'] / n if n else nan,
                dur_ratio=s['len_syn'] / s['len_ref'] if s['len_ref'] else nan,
                n_path=n, n_both_voiced=nb)


def pool(sums_list):
    """the corpus scores of a list of per-pair sums"""
    keys = ('cost', 'n_path', 'n_both_voiced', 'sq_hz', 'sq_cents', 'gross', 'vdiff', 'len_ref', 'len_syn')
    return scores_from_sums({k: sum(s[k] for s in sums_list) for k in keys})


def dct_table(n_coef=24, n_bins=80):
    """rows 1 .. n_coef of the orthonormal DCT-II over n_bins points, float64 [n_coef, n_bins]"""
    c = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_bins, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_bins) * np.cos(math.pi * c * (m + 0.5) / n_bins)


def mel_cepstra(logmel10, n_coef=24, dt=np.float64):
    """[..., 80] log10-mel -> [..., n_coef]: the DCT-II of ln(10) * logmel10 without c0.  float32: the table (ln(10) folded in) rounded once, the
    products and the sum over the bins rounded one by one in ascending order"""
    x = np.asarray(logmel10).astype(dt)
    w = (math.log(10.0) * dct_table(n_coef, x.shape[-1])).astype(dt)
    if dt == np.float64:
        return x @ w.T
    out = np.zeros(x.shape[:-1] + (n_coef,), dt)
    for m in range(x.shape[-1]):
        out = (out + (x[..., m][..., None] * w[:, m]).astype(dt)).astype(dt)
    return out
