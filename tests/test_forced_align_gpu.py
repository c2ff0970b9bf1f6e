"""GPU: the forced aligner — ttsc_fa_viterbi and ttsc_fa_accumulate (csrc/forced_align.hip) against the float32 / float64 statements of
tests/forced_align_reference.py, the refused arguments of the C ABI, ForcedAligner.fit / align on the generated corpus and scripts/align_corpus.py
followed by scripts/import_textgrid.py.

Bound of the float64 check (derived, not measured), u = 2^-24.  fl(e + x) is monotone in x, so the float32 recurrence returns the maximum over
all paths of each path's own float32 sum, taken frame by frame, of the float32 emissions.  An emission is cst - 0.5 acc with acc a sum of D
non-negative terms, each from a rounded difference, two rounded products (relative error <= 4 u to first order) and up to D - 1 rounded additions:
|acc~ - acc| <= (D + 3) u acc, the halving is exact and the subtraction adds u |e|; with a = |cst| + 0.5 acc >= |e| an emission is off by at most
(D + 4) u a.  The T - 1 rounded additions along a path add at most (T - 1) u sum_t |e~_t|.  So a path P's float32 score lies within
(T + D + 4) u A_P of its float64 score, A_P = sum_t a_t, to first order in u; 1.02 covers the higher orders while (T + D + 4) u < 0.01.  The
kernel's path K is the float32 optimum and the float64 optimum O is one of the paths it beat, hence
    0 <= s64(O) - s64(K) <= 1.02 (T + D + 4) u (A_K + A_O)     and     |score - s64(K)| <= 1.02 (T + D + 4) u A_K.
Beyond that bound the kernel states its arithmetic, so its path and score must equal the float32 restatement's bit for bit."""
import ctypes as C
import functools
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from tests import forced_align_reference as R
from tests import forced_align_signals as S
from tests.conftest import ROOT
from tests.test_forced_align_cpu import N_SUB, PHONES, REF_MAX_BOUNDARY_ERROR_S, boundary_report, lattice_of

pytestmark = pytest.mark.gpu

FRAME_S = 0.010
TOLERANCE_S = REF_MAX_BOUNDARY_ERROR_S + FRAME_S              # the float64 restatement's own largest error plus one frame
M_INJ = 7
# the kernel's edges: 256 threads (S = 260 puts a second position on four of them), emission tiles of 8 frames (T = 297 = 37 tiles + 1)
BIG_T, BIG_S = 297, 260


def lattice(S_, state, skips=(), starts=(0,), finals=None):
    lat = {'state': np.asarray(state, np.int32), 'skip': np.full(S_, -1, np.int32), 'start': np.zeros(S_, np.uint8), 'final': np.zeros(S_, np.uint8)}
    for j, k in skips:
        lat['skip'][j] = k
    lat['start'][list(starts)] = 1
    lat['final'][list(finals if finals is not None else (S_ - 1,))] = 1
    return lat


@functools.lru_cache(maxsize=None)
def injected(D):
    """seed 1234: a model of 7 states and the ragged batch of the issue; each case with its float32 and float64 solutions (computed once, shared,
    never modified)"""
    rng = np.random.default_rng(1234 + D)
    mean = rng.standard_normal((M_INJ, D)).astype(np.float32)
    ivar = (1.0 / rng.uniform(0.5, 2.0, (M_INJ, D))).astype(np.float32)
    cst = rng.uniform(-3.0, 0.0, M_INJ).astype(np.float32)
    st = lambda n: rng.integers(0, M_INJ, n)
    big_skips = [(j, j - int(rng.integers(2, 6))) for j in range(10, BIG_S, 9)]
    shapes = [
        (0, lattice(3, st(3))),
        (1, lattice(1, st(1))),
        (7, lattice(7, st(7))),                                  # only the all-advance path fits
        (6, lattice(7, st(7))),                                  # infeasible
        (6, lattice(7, st(7), skips=[(3, 1)])),                  # the skip over position 2 makes it feasible
        (12, lattice(5, st(5), skips=[(3, 0)], starts=(0, 1), finals=(2, 3, 4))),
        (BIG_T, lattice(BIG_S, st(BIG_S), skips=big_skips, starts=(0, 3, 7), finals=(BIG_S - 1, BIG_S - 4, BIG_S - 30))),
    ]
    cases = []
    for T, lat in shapes:
        x = rng.standard_normal((T, D)).astype(np.float32)
        a32, s32, ok32 = R.viterbi(x, lat, mean, ivar, cst, np.float32)
        a64, s64, ok64 = R.viterbi(x, lat, mean, ivar, cst, np.float64)
        cases.append(dict(x=x, lat=lat, a32=a32, s32=np.float32(s32), ok32=ok32, a64=a64, s64=float(s64), ok64=ok64))
    assert [c['ok32'] for c in cases] == [0, 1, 1, 0, 1, 1, 1] and [c['ok64'] for c in cases] == [0, 1, 1, 0, 1, 1, 1]
    assert list(cases[2]['a32']) == list(range(7)) and 2 not in cases[4]['a32']
    return (mean, ivar, cst), cases


def pack(cases, D, Tmax=None, Smax=None, poison=False):
    """-> (feat [B, Tmax, D], nframes, host lattice arrays).  poison: NaN behind every utterance's own frames, out-of-range ids and set flags behind
    its own positions"""
    B = len(cases)
    Tmax = Tmax or max([c['x'].shape[0] for c in cases] + [1])
    Smax = Smax or max(len(c['lat']['state']) for c in cases)
    feat = np.full((B, Tmax, D), np.nan if poison else 0.0, np.float32)
    lat = {'state': np.full((B, Smax), 10 ** 6 if poison else -1, np.int32), 'skip': np.full((B, Smax), 10 ** 6 if poison else -1, np.int32),
           'start': np.full((B, Smax), 1 if poison else 0, np.uint8), 'final': np.full((B, Smax), 1 if poison else 0, np.uint8),
           'npos': np.asarray([len(c['lat']['state']) for c in cases], np.int32)}
    for b, c in enumerate(cases):
        feat[b, :c['x'].shape[0]] = c['x']
        for k in ('state', 'skip', 'start', 'final'):
            lat[k][b, :len(c['lat'][k])] = c['lat'][k]
    return feat, np.asarray([c['x'].shape[0] for c in cases], np.int32), lat


def run_viterbi(cases, model, **kw):
    from ttscube_amd.io_utils import forced_align as FA
    D = model[0].shape[1]
    feat, nf, lat = pack(cases, D, **kw)
    dev = 'cuda:0'
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dlat = FA.upload_lattice(lat, model[0].shape[0], dev)
    out = FA.viterbi(t(feat), t(nf), dlat, *[t(m) for m in model])
    return {k: v.cpu().numpy() for k, v in out.items()}, (t(feat), t(nf), dlat)


@functools.lru_cache(maxsize=None)
def injected_results(D):
    model, cases = injected(D)
    return run_viterbi(cases, model)


# ---- the search --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [1, 26])
def test_viterbi_equals_the_float32_restatement_bit_for_bit(D):
    model, cases = injected(D)
    out, _ = injected_results(D)
    for b, c in enumerate(cases):
        T = c['x'].shape[0]
        assert int(out['ok'][b]) == c['ok32'], b
        assert np.all(out['align'][b, T:] == -1), b
        if c['ok32']:
            assert np.array_equal(out['align'][b, :T], c['a32']), b
            assert out['score'][b].tobytes() == c['s32'].tobytes(), (b, out['score'][b], c['s32'])
            assert R.path_ok(out['align'][b, :T], c['lat'])
        else:
            assert np.all(out['align'][b] == -1) and out['score'][b] == 0, b


def test_ties_follow_the_stated_order():
    """small integer features, repeated model states at neighbouring positions, variances that are powers of two: every emission is an exact small
    dyadic number, exact ties occur, and the path is the one the stated order gives — in float32 and in float64 alike"""
    rng = np.random.default_rng(1234)
    D, M = 2, 4
    mean = rng.integers(-1, 2, (M, D)).astype(np.float32)
    ivar = np.asarray([[2.0, 0.5], [1.0, 1.0], [0.5, 2.0], [1.0, 0.5]], np.float32)
    cst = np.asarray([0.0, -1.0, 0.0, -0.5], np.float32)
    same = lattice(3, [2, 2, 2])
    cases = [dict(x=np.ones((5, D), np.float32), lat=same)]
    for T, S_ in ((9, 4), (14, 6), (40, 12)):
        state = np.repeat(rng.integers(0, M, (S_ + 1) // 2), 2)[:S_]
        lat = lattice(S_, state, skips=[(j, j - 2) for j in range(3, S_, 3)], starts=(0, 1), finals=(S_ - 1, S_ - 2))
        cases.append(dict(x=rng.integers(-2, 3, (T, D)).astype(np.float32), lat=lat))
    out, _ = run_viterbi(cases, (mean, ivar, cst))
    # one state everywhere: every reachable score ties, staying wins, so the walk back leaves the end position as late as it can
    assert out['align'][0, :5].tolist() == [0, 1, 2, 2, 2]
    ties = 0
    for b, c in enumerate(cases):
        T = c['x'].shape[0]
        a32, s32, ok = R.viterbi(c['x'], c['lat'], mean, ivar, cst, np.float32)
        a64, s64, _ = R.viterbi(c['x'], c['lat'], mean, ivar, cst, np.float64)
        assert ok and np.array_equal(a32, a64) and float(s32) == float(s64)          # exact arithmetic: both precisions agree
        assert np.array_equal(out['align'][b, :T], a32) and out['score'][b].tobytes() == np.float32(s32).tobytes(), b
        e = R.emissions(c['x'], c['lat']['state'].astype(np.int64), mean, ivar, cst, np.float64)
        ties += int(e.size - np.unique(e).size)
    assert ties > 0


def test_paths_are_optimal_within_the_derived_bound():
    D = 26
    model, cases = injected(D)
    out, _ = injected_results(D)
    u = 2.0 ** -24
    for b, c in enumerate(cases):
        if not c['ok64']:
            continue
        T = c['x'].shape[0]
        path = out['align'][b, :T]

        def magnitude(al):
            e = R.emissions(c['x'], c['lat']['state'].astype(np.int64), *model, np.float64)[np.arange(T), al]
            k = np.abs(model[2].astype(np.float64))[c['lat']['state'][al]]
            return float((k + (model[2].astype(np.float64)[c['lat']['state'][al]] - e)).sum())

        own = R.path_score64(c['x'], path, c['lat'], *model)
        rel = 1.02 * (T + D + 4) * u
        assert rel < 0.0102
        tol = rel * (magnitude(path) + magnitude(c['a64']))
        print('T %d S %d: optimum %.6f, kernel path %.3e below it (bound %.3e), score off its own path by %.3e (bound %.3e)'
              % (T, len(c['lat']['state']), c['s64'], c['s64'] - own, tol, float(out['score'][b]) - own, rel * magnitude(path)))
        assert own <= c['s64'] + 1e-12 * abs(c['s64']) and c['s64'] - own <= tol, (b, own, c['s64'], tol)
        assert abs(float(out['score'][b]) - own) <= rel * magnitude(path), (b, float(out['score'][b]), own)


def test_an_utterance_has_the_same_bits_alone_and_in_a_poisoned_batch():
    D = 26
    model, cases = injected(D)
    out, _ = injected_results(D)
    for b in (4, 5, 6):
        T = cases[b]['x'].shape[0]
        alone, _ = run_viterbi([cases[b]], model)
        assert np.array_equal(alone['align'][0, :T], out['align'][b, :T]) and alone['score'][0].tobytes() == out['score'][b].tobytes()
        assert alone['ok'][0] == out['ok'][b]
    padded, _ = run_viterbi(cases, model, Tmax=BIG_T + 13, Smax=BIG_S + 5, poison=True)
    assert np.array_equal(padded['ok'], out['ok']) and padded['score'].tobytes() == out['score'].tobytes()
    assert np.array_equal(padded['align'][:, :BIG_T], out['align']) and np.all(padded['align'][:, BIG_T:] == -1)


# ---- the statistics ----------------------------------------------------------------------------------------------------------------------------------

def _tables(M, D):
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda:0')
    return z(M), z(M, D), z(M, D)


def test_accumulate_equals_the_restatement_bit_for_bit():
    from ttscube_amd.io_utils import forced_align as FA
    D = 26
    model, cases = injected(D)
    out, (feat, nf, dlat) = injected_results(D)
    ok = out['ok'].copy()
    ok[5] = 0                                                     # a row with a valid alignment that is switched off contributes nothing
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    feats = [c['x'] for c in cases]
    aligns = [out['align'][b, :c['x'].shape[0]] for b, c in enumerate(cases)]
    lats = [c['lat'] for c in cases]

    def device(rows_ok, tables):
        FA.accumulate(feat, nf, t(out['align']), t(np.asarray(rows_ok, np.int32)), dlat, *tables)
        return [v.cpu().numpy() for v in tables]

    def host(rows_ok, tables):
        R.accumulate(feats, aligns, list(rows_ok), lats, *tables)
        return tables

    want = host(ok, [np.zeros(M_INJ), np.zeros((M_INJ, D)), np.zeros((M_INJ, D))])
    got = device(ok, _tables(M_INJ, D))
    again = device(ok, _tables(M_INJ, D))
    assert want[0].sum() == sum(c['x'].shape[0] for b, c in enumerate(cases) if ok[b])
    for g, a, w in zip(got, again, want):
        assert g.tobytes() == w.tobytes() and a.tobytes() == g.tobytes()
    # two batches into one running table: the batch totals are added one after the other
    first = np.asarray([1, 1, 1, 1, 1, 1, 0], np.int32) * out['ok']
    second = np.asarray([0, 0, 0, 0, 0, 0, 1], np.int32) * out['ok']
    tables = _tables(M_INJ, D)
    device(first, tables)
    got2 = device(second, tables)
    want2 = host(second, host(first, [np.zeros(M_INJ), np.zeros((M_INJ, D)), np.zeros((M_INJ, D))]))
    for g, w in zip(got2, want2):
        assert g.tobytes() == w.tobytes()
    none = device(np.zeros(len(cases), np.int32), _tables(M_INJ, D))
    assert all(not v.any() for v in none)


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------------------------------------

def test_every_refused_argument_through_the_c_abi():
    from ttscube_amd import _lib
    L = _lib.lib()
    B, T, S_, D, M = 2, 5, 4, 3, 6
    dev = 'cuda:0'
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    feat, nf = z((B, T, D), torch.float32), z((B,), torch.int32)
    state, skip, start, fin, npos = z((B, S_), torch.int32), z((B, S_), torch.int32) - 1, z((B, S_), torch.uint8), z((B, S_), torch.uint8), \
        z((B,), torch.int32)
    mean, ivar, cst = z((M, D), torch.float32), z((M, D), torch.float32) + 1, z((M,), torch.float32)
    align, score, ok = z((B, T), torch.int32), z((B,), torch.float32), z((B,), torch.int32)
    need = int(L.ttsc_fa_workspace_bytes(B, T, S_))
    assert need >= B * T * S_ and need % 16 == 0 and L.ttsc_fa_workspace_bytes(-1, T, S_) == 0
    ws = z((need + 16,), torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(feat=p(feat), nf=p(nf), state=p(state), skip=p(skip), start=p(start), fin=p(fin), npos=p(npos), mean=p(mean), ivar=p(ivar), cst=p(cst),
                B=B, T=T, S=S_, D=D, M=M, ws=p(ws), wsb=need, align=p(align), score=p(score), ok=p(ok))
    order = ('feat', 'nf', 'state', 'skip', 'start', 'fin', 'npos', 'mean', 'ivar', 'cst', 'B', 'T', 'S', 'D', 'M', 'ws', 'wsb', 'align', 'score', 'ok')

    def call(**change):
        a = dict(good, **change)
        return L.ttsc_fa_viterbi(*[a[k] for k in order], _lib.current_stream())

    def refused(rc, what):
        assert rc != 0, what
        assert L.ttsc_last_error(), what

    assert call() == 0
    null = C.c_void_p(0)
    for change in (dict(B=-1), dict(T=-1), dict(S=-1), dict(S=1025), dict(D=0), dict(D=-3), dict(D=64), dict(M=-1), dict(T=1 << 30),
                   dict(feat=null), dict(align=null), dict(nf=null), dict(npos=null), dict(score=null), dict(ok=null), dict(state=null),
                   dict(skip=null), dict(start=null), dict(fin=null), dict(mean=null), dict(ivar=null), dict(cst=null), dict(ws=null),
                   dict(wsb=need - 1), dict(ws=C.c_void_p(ws.data_ptr() + 4))):
        refused(call(**change), change)
    assert call(B=0, feat=null, nf=null) == 0                     # nothing to do is not an error
    # the lattice tables are checked over their host copies
    h = dict(state=np.zeros((B, S_), np.int32), skip=np.full((B, S_), -1, np.int32), start=np.zeros((B, S_), np.uint8), fin=np.zeros((B, S_), np.uint8),
             npos=np.full((B,), S_, np.int32))

    def check(M_=M, S2=S_, B_=B, **change):
        a = {k: v.copy() for k, v in h.items()}
        for k, (idx, val) in change.items():
            a[k][idx] = val
        return L.ttsc_fa_check_lattice(*[C.c_void_p(a[k].ctypes.data) for k in ('state', 'skip', 'start', 'fin', 'npos')], B_, S2, M_)

    assert check() == 0
    for kw in (dict(state=((1, 2), M)), dict(state=((0, 0), -1)), dict(skip=((1, 2), 2)), dict(skip=((1, 3), 7)), dict(skip=((0, 1), -2)),
               dict(start=((1, 1), 2)), dict(fin=((0, 3), 255)), dict(npos=((1,), S_ + 1)), dict(npos=((0,), -1)), dict(B_=-1), dict(M_=-1)):
        refused(check(**kw), kw)
    refused(L.ttsc_fa_check_lattice(null, null, null, null, null, B, S_, M), 'null tables')
    assert check(state=((1, 2), M), npos=((1,), 2)) == 0           # behind an utterance's own positions nothing is looked at
    # accumulate
    count, total, sumsq = _tables(M, D)
    need2 = int(L.ttsc_fa_accumulate_workspace_bytes(B, S_, D))
    ws2 = z((need2 + 16,), torch.uint8)
    good2 = dict(feat=p(feat), nf=p(nf), align=p(align), ok=p(ok), state=p(state), npos=p(npos), B=B, T=T, S=S_, D=D, M=M, ws=p(ws2), wsb=need2,
                 count=p(count), total=p(total), sumsq=p(sumsq))
    order2 = ('feat', 'nf', 'align', 'ok', 'state', 'npos', 'B', 'T', 'S', 'D', 'M', 'ws', 'wsb', 'count', 'total', 'sumsq')

    def call2(**change):
        a = dict(good2, **change)
        return L.ttsc_fa_accumulate(*[a[k] for k in order2], _lib.current_stream())

    assert call2() == 0
    for change in (dict(B=-1), dict(T=-1), dict(S=-1), dict(S=1025), dict(D=0), dict(D=64), dict(M=-1), dict(feat=null), dict(nf=null),
                   dict(align=null), dict(ok=null), dict(state=null), dict(npos=null), dict(count=null), dict(total=null), dict(sumsq=null),
                   dict(ws=null), dict(wsb=need2 - 1), dict(ws=C.c_void_p(ws2.data_ptr() + 8))):
        refused(call2(**change), change)
    torch.cuda.synchronize()
    assert not count.any().item()
    # and the Python wrapper refuses a bad skip before anything is uploaded
    from ttscube_amd.io_utils import forced_align as FA
    bad = FA.pack_lattices([FA.build_lattice([[1], [2]], 2)])
    bad['skip'][0, 6] = 6
    with pytest.raises(_lib.TTSCError):
        FA.upload_lattice(bad, 6, dev)


# ---- features ----------------------------------------------------------------------------------------------------------------------------------------

def test_feature_rows_do_not_depend_on_the_batch_and_match_float64():
    from ttscube_amd.io_utils import forced_align as FA
    rng = np.random.default_rng(1234)
    lens = [37, 1, 64, 0, 20]
    mel = rng.uniform(-5.0, 1.0, (len(lens), 64, 80)).astype(np.float32)
    dmel = torch.from_numpy(mel).cuda()
    full = FA.align_features(dmel, torch.tensor(lens, dtype=torch.int32).cuda()).cpu().numpy()
    assert full.shape == (len(lens), 64, 26)
    w = np.log(10.0) * R.dct_table(13, 80)
    for b, n in enumerate(lens):
        assert not full[b, n:].any()
        alone = FA.align_features(dmel[b:b + 1, :max(n, 1)].contiguous(), torch.tensor([n], dtype=torch.int32).cuda()).cpu().numpy()
        assert alone[0, :n].tobytes() == full[b, :n].tobytes(), b
        if n:
            want = R.features(mel[b, :n])
            tol = 1.02 * 81 * 2.0 ** -24 * (np.abs(mel[b, :n].astype(np.float64)) @ np.abs(w).T)      # 80 products and 79 additions, the table rounded once
            assert np.all(np.abs(full[b, :n, :13] - want[:, :13]) <= tol)
            assert np.all(np.abs(full[b, :n, 13:] - want[:, 13:]) <= tol.max(axis=0) + 1e-6 * np.abs(want[:, 13:]))
            assert np.array_equal(full[b, :n, 13:], R.deltas(np.ascontiguousarray(full[b, :n, :13])))   # the deltas of its own cepstra, exactly


# ---- fit and align on the generated corpus -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fitted():
    """the generated corpus through ForcedAligner.fit (three batches) and align, with the trace and the device's own features per utterance"""
    from ttscube_amd.io_utils import forced_align as FA
    items = S.corpus()
    for it in items:
        it['prons'] = [S.LEXICON[w.upper()] for w in it['words']]
    aligner = FA.ForcedAligner(S.PHONES, n_sub=N_SUB, device='cuda:0')
    assert aligner.phones == PHONES
    trace = []
    history = aligner.fit(items, iterations=4, batch=3, trace=trace)
    feats = []
    for bt in aligner._batches(items, 3):
        f, n = bt['feat'].cpu().numpy(), bt['nframes'].cpu().numpy()
        feats += [f[b, :n[b]].copy() for b in range(len(n))]
    return items, aligner, history, trace, feats, aligner.align(items, batch=3)


def test_fit_equals_the_restatement_after_every_iteration():
    items, aligner, history, trace, feats, _ = fitted()
    lats = [lattice_of(it) for it in items]
    assert [f.shape[0] for f in feats] == [len(it['audio']) // S.HOP for it in items]
    steps = R.fit(feats, lats, len(PHONES) * N_SUB, 4, np.float32, batch=3)
    assert len(trace) == len(steps) == 5 and len(history) == 4
    for k, (got, want) in enumerate(zip(trace, steps)):
        assert got['ok'] == want['oks'] and all(got['ok']), k
        for a, b in zip(got['align'], want['aligns']):
            assert np.array_equal(a, b), k
        assert got['mean'].tobytes() == want['mean'].tobytes() and got['var'].tobytes() == want['var'].tobytes(), k
    for h, want in zip(history, steps[1:]):
        assert h['infeasible'] == [] and h['frames'] == want['frames'] and h['score'] == pytest.approx(want['score'], rel=1e-12)
    scores = [h['score'] for h in history]
    assert all(b > a for a, b in zip(scores, scores[1:])), scores


def test_boundaries_and_silences_on_the_generated_corpus(tmp_path):
    from ttscube_amd.io_utils import forced_align as FA
    items, aligner, _, _, _, results = fitted()
    assert [r['id'] for r in results] == [it['id'] for it in items]
    infeasible, wrong, errs, total = boundary_report(items, [(r['words'], r['phones']) if r['ok'] else None for r in results])
    assert not infeasible and not wrong, (infeasible, wrong)      # the silences are as generated
    assert len(errs) == total
    worst = float(np.max(np.abs(errs)))
    print('device: %d boundaries, largest error %.4f ms (allowed %.1f ms), mean signed error %.4f ms'
          % (total, 1e3 * worst, 1e3 * TOLERANCE_S, 1e3 * float(np.mean(errs))))
    assert worst <= TOLERANCE_S + 1e-9
    for it, r in zip(items, results):
        assert [w[0] for w in r['words'] if w[0]] == it['words']
        assert r['words'][0][1] == 0.0 and r['words'][-1][2] == r['duration'] == len(it['audio']) / S.SAMPLE_RATE
    path = str(tmp_path / 'aligner.npz')
    aligner.save(path)
    again = FA.ForcedAligner.load(path, device='cuda:0')
    assert again.phones == aligner.phones and again.n_sub == N_SUB
    for a, b in zip(again.align(items, batch=8), results):
        assert a['ok'] == b['ok'] and a['score'] == b['score'] and np.array_equal(a['frames'], b['frames'])
        assert a['words'] == b['words'] and a['phones'] == b['phones']


def _load(name):
    spec = importlib.util.spec_from_file_location(name + '_script', os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_align_corpus_then_import_textgrid(tmp_path):
    """scripts/align_corpus.py on the generated corpus, scripts/import_textgrid.py on its output, CubeganDataset on the result: every phone's run
    of frame2phon starts within the tolerance of the truth plus the importer's own 10 ms grid"""
    from ttscube_amd.io_utils.audio import save_wav
    from ttscube_amd.io_utils.io_cubegan import CubeganDataset
    items = S.corpus()
    src, aligned, processed = tmp_path / 'recordings', tmp_path / 'aligned', tmp_path / 'processed'
    src.mkdir()
    (tmp_path / 'lexicon').write_text(S.lexicon_text())
    for it in items:
        save_wav(str(src / (it['id'] + '.wav')), it['audio'], S.SAMPLE_RATE)
        (src / (it['id'] + '.txt')).write_text(it['text'] + '\n')
    out = io.StringIO()
    assert _load('align_corpus').main(['--input-folder', str(src), '--lexicon', str(tmp_path / 'lexicon'), '--output-folder', str(aligned),
                                       '--model-out', str(tmp_path / 'aligner.npz'), '--batch', '4'], out=out) == 0
    assert 'Wrote %d TextGrid files' % len(items) in out.getvalue() and 'Skipped' not in out.getvalue()
    assert _load('import_textgrid').main(['--input-folder', str(aligned), '--output-folder', str(processed), '--dev-ratio', '2', '--speaker', 'syn',
                                          '--prefix', 'SYN', '--batch', '4']) == 0
    ds = CubeganDataset(str(processed / 'train'))
    assert len(ds) == len(items)
    by_id = {it['id']: it for it in items}
    worst = 0.0
    for i in range(len(ds)):
        meta = ds[i]['meta']
        it = by_id[meta['orig_filename']]
        f2p = np.asarray(meta['frame2phon'])
        spoken = [k for k, p in enumerate(meta['phones']) if p in S.PHONES]
        truth = [u for u in it['units'] if u[0]]
        assert [meta['phones'][k] for k in spoken] == [u[0] for u in truth]
        for k, u in zip(spoken, truth):
            frames = np.nonzero(f2p == k)[0]
            assert frames.size, (meta['orig_filename'], k)
            worst = max(worst, abs(frames[0] / 100.0 - u[2] / S.SAMPLE_RATE))
    print('frame2phon: the largest offset of a phone run from the truth is %.1f ms (allowed %.1f ms)' % (1e3 * worst, 1e3 * (TOLERANCE_S + 0.010)))
    assert worst <= TOLERANCE_S + 0.010 + 1e-9
