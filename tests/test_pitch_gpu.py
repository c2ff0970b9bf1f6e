"""GPU: the two pitch kernels (csrc/pitch.hip) against the float64 restatement tests/pitch_reference.py."""
import functools

import numpy as np
import pytest
import torch

from tests import pitch_reference as R
from tests import pitch_signals as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CONFIGS = {
    # F not a multiple of the frame group with a partial last hop | full length | every frame reads into the zero tail | F = 0
    '24k': dict(sr=24000, hop=240, fmin=60, fmax=400, lengths=(240 * 17 + 13, 240 * 40, 900, 100)),
    # K = 503: more lags than threads in a workgroup
    '16k': dict(sr=16000, hop=256, fmin=30, fmax=500, lengths=(256 * 9 + 1, 256 * 20)),
}
KINDS = ('noise', 'harmonic', 'zero', 'offset')


@functools.lru_cache(maxsize=None)
def _batch(cfg_name, kind):
    cfg = CONFIGS[cfg_name]
    rng = np.random.default_rng(KINDS.index(kind) + 11)
    Lmax = max(cfg['lengths'])
    x = np.zeros((len(cfg['lengths']), Lmax), np.float32)
    for b, L in enumerate(cfg['lengths']):
        t = np.arange(L) / cfg['sr']
        if kind == 'noise':
            x[b, :L] = rng.uniform(-0.5, 0.5, L)
        elif kind == 'harmonic':
            x[b, :L] = 0.2 * sum(np.sin(2 * np.pi * h * (110.0 + 30.0 * b) * t) / h for h in range(1, 6))
        elif kind == 'offset':
            x[b, :L] = 0.5 + 0.05 * rng.uniform(-1.0, 1.0, L) + 0.05 * np.sin(2 * np.pi * 150.0 * t)
        x[b, L:] = 7.0      # whatever lies behind an utterance's end in a padded batch must not be read
    return x


@functools.lru_cache(maxsize=None)
def _reference(cfg_name, kind, dtype):
    cfg = CONFIGS[cfg_name]
    x = _batch(cfg_name, kind)
    return [R.nccf(x[b], L, cfg['sr'], cfg['hop'], cfg['fmin'], cfg['fmax'], dtype) for b, L in enumerate(cfg['lengths'])]


def _gpu_tables(cfg_name, kind, want_phi=True):
    from ttscube_amd.io_utils import pitch
    cfg = CONFIGS[cfg_name]
    x = torch.from_numpy(_batch(cfg_name, kind)).to(DEV)
    lengths = torch.tensor(cfg['lengths'], dtype=torch.int32, device=DEV)
    return pitch.nccf(x, lengths, cfg['sr'], cfg['hop'], cfg['fmin'], cfg['fmax'], want_phi=want_phi)


@pytest.mark.parametrize('cfg_name,kind', [('24k', k) for k in KINDS] + [('16k', 'noise'), ('16k', 'harmonic')])
def test_nccf_against_float64(cfg_name, kind):
    """phi, rms and maxphi of ttsc_pitch_nccf against float64, within 4 x the largest deviation of the restatement run in float32 on the same input
    (the kernel sums the n terms in another order).  All-zero input gives phi exactly 0.  Measured on MI355X, largest |deviation| from float64,
    float32 restatement / kernel — phi: 4.8e-8 / 6.5e-8 (24k noise), 2.2e-7 / 2.1e-7 (24k harmonic), 0 / 0 (zeros), 6.2e-7 / 6.3e-7 (24k offset),
    5.5e-8 / 6.0e-8 (16k noise), 2.1e-7 / 2.1e-7 (16k harmonic); rms: at most 2.8e-8 / 2.8e-8; maxphi: at most 1.7e-7 / 1.4e-7."""
    cfg = CONFIGS[cfg_name]
    tab = _gpu_tables(cfg_name, kind)
    got = {k: tab[k].cpu().numpy() for k in ('phi', 'rms', 'maxphi', 'ncand')}
    r64, r32 = _reference(cfg_name, kind, np.float64), _reference(cfg_name, kind, np.float32)
    Fmax = max(cfg['lengths']) // cfg['hop']
    assert got['phi'].shape == (len(cfg['lengths']), Fmax, R.params(cfg['sr'], cfg['fmin'], cfg['fmax'])[3])
    for i, name in enumerate(('phi', 'rms', 'maxphi')):
        tol = 4.0 * max([float(np.abs(a[i].astype(np.float64) - b[i]).max()) for a, b in zip(r32, r64) if b[i].size] or [0.0])
        dev = 0.0
        for b, L in enumerate(cfg['lengths']):
            F = L // cfg['hop']
            if F:
                dev = max(dev, float(np.abs(got[name][b, :F].astype(np.float64) - r64[b][i]).max()))
            assert not got[name][b, F:].any(), '%s is not zero behind the last frame of utterance %d' % (name, b)
        print('%s/%s %s: float32 restatement deviates by %.3e, kernel by %.3e (bound %.3e)' % (cfg_name, kind, name, tol / 4.0, dev, tol))
        assert dev <= tol, (name, dev, tol)
    if kind == 'zero':
        assert not got['phi'].any() and not got['ncand'].any()


def test_candidates_from_the_kernels_own_phi():
    """peak picking, the top-20 order and the parabola: the kernel's candidate tables against the restatement's `candidates` run in float32 on the
    phi the kernel itself wrote (the same inputs, the same comparisons: equal up to the rounding of the parabola)"""
    for cfg_name in CONFIGS:
        cfg = CONFIGS[cfg_name]
        _, kmin, _, _ = R.params(cfg['sr'], cfg['fmin'], cfg['fmax'])
        for kind in ('noise', 'harmonic'):
            tab = {k: v.cpu().numpy() for k, v in _gpu_tables(cfg_name, kind).items()}
            for b, L in enumerate(cfg['lengths']):
                F = L // cfg['hop']
                lag, val, ncand = R.candidates(tab['phi'][b, :F], kmin, np.float32)
                assert np.array_equal(tab['ncand'][b, :F], ncand)
                assert np.allclose(tab['cand_lag'][b, :F], lag, rtol=0, atol=1e-3) and np.allclose(tab['cand_val'][b, :F], val, rtol=0, atol=1e-5)
                assert not tab['cand_lag'][b, F:].any() and not tab['ncand'][b, F:].any()


def _track_tables():
    from ttscube_amd.io_utils import pitch
    tb = S.candidate_tables()
    d = {k: torch.from_numpy(v).to(DEV) for k, v in tb.items()}
    f0 = pitch.track(d['lag'], d['val'], d['ncand'], d['maxphi'], d['rms'], d['nframes'], S.TABLE_KMAX, S.SR)
    return tb, f0.cpu().numpy()


def test_tracking_with_injected_tables():
    """The cost, in float64, of the path ttsc_pitch_track walks through injected candidate tables is within 16 F 2^-24 max(D_opt, 1) of the float64
    optimum (one rounding per accumulation, a few ulps per cost, on both paths); where that optimum is clear of ties and float32 reproduces it, the
    path itself is the same.  F in {1, 2, 37}, 0 .. 20 candidates per frame, one utterance with 20 in every frame.  Measured on MI355X: D_kernel - D_opt
    = 0 on all 13 utterances (bounds 9.5e-7 at F = 1 to 4.1e-4 at F = 37)."""
    tb, f0 = _track_tables()
    sol = S.table_solutions()
    decided = 0
    for b, F in enumerate(S.TABLE_FRAMES):
        assert not f0[b, F:].any()
        path = S.states_from_f0(f0[b, :F], tb['lag'][b, :F], tb['ncand'][b, :F])
        D_k = R.path_cost(path, *sol[b]['args'], S.TABLE_KMAX)
        D_opt = sol[b]['D_opt']
        bound = 16.0 * F * 2.0 ** -24 * max(D_opt, 1.0)
        print('utterance %d (F = %d): D_kernel - D_opt = %.3e, bound %.3e' % (b, F, D_k - D_opt, bound))
        assert D_k - D_opt <= bound, (b, D_k, D_opt, bound)
        if sol[b]['margin'] > 1e-3 and sol[b]['same32']:
            decided += 1
            assert np.array_equal(path, sol[b]['path']), b
    assert decided * 2 >= len(S.TABLE_FRAMES)


def _tracker_f0(x, lengths):
    from ttscube_amd.io_utils.pitch import PitchTracker
    return PitchTracker(DEV)(x, S.SR, S.HOP, S.FMIN, S.FMAX, lengths=lengths)


def test_known_answers_end_to_end():
    """glide 90 -> 250 Hz and steady 120 Hz, silence at both ends and a silent gap: voiced and within 2 % wherever the analysis span lies inside a
    voiced stretch, 0 wherever it lies inside silence; the GPU track agrees with the float64 track (voicing, and 1 Hz) on all but 2 % of the frames
    (measured on MI355X: it disagrees on none)"""
    x, lengths, truth = S.known_answer_batch()
    f0 = _tracker_f0(x, lengths)
    assert f0.dtype == np.float64 and f0.shape == (2, x.shape[1] // S.HOP)
    f64 = R.rapt_f0(x, lengths, S.SR, S.HOP, S.FMIN, S.FMAX)
    for b in range(2):
        kind, _ = S.check_known_answer(f0[b], truth[b])
        d = S.disagreement(f0[b], f64[b].astype(np.float64), kind)
        print('utterance %d: GPU and float64 tracks disagree on %.4f of the scored frames' % (b, d))
        assert d <= 0.02


def test_determinism_and_ragged_independence():
    """the same batch twice gives the same bits, and so does an utterance tracked alone and inside a padded batch"""
    cfg = CONFIGS['24k']
    x = _batch('24k', 'harmonic') + 0.3 * _batch('24k', 'noise')
    for b, L in enumerate(cfg['lengths']):
        x[b, L:] = 0
    lengths = list(cfg['lengths'])
    a, b2 = _tracker_f0(x, lengths), _tracker_f0(x, lengths)
    assert np.array_equal(a, b2)
    t1, t2 = _gpu_tables('24k', 'noise'), _gpu_tables('24k', 'noise')
    for k in ('phi', 'cand_lag', 'cand_val', 'ncand', 'maxphi', 'rms'):
        assert torch.equal(t1[k], t2[k]), k
    for b, L in enumerate(lengths):
        alone = _tracker_f0(x[b, :L], None)
        assert alone.shape == (L // S.HOP,)
        assert np.array_equal(alone, a[b, :L // S.HOP]), b
        assert not a[b, L // S.HOP:].any()


def test_call_shapes_and_rapt_wrapper():
    from ttscube_amd.io_utils.pitch import PitchTracker, rapt
    x, lengths, _ = S.known_answer_batch()
    one = rapt(x[1] * 32768.0, S.SR, S.HOP, min=S.FMIN, max=S.FMAX)
    assert one.dtype == np.float64 and one.shape == (x.shape[1] // S.HOP,)
    assert np.array_equal(one, PitchTracker(DEV)(x[1], S.SR, S.HOP, S.FMIN, S.FMAX))
    assert PitchTracker(DEV)(np.zeros(100, np.float32), S.SR, S.HOP).shape == (0,)
    with pytest.raises(NotImplementedError):
        rapt(x[1], S.SR, S.HOP, otype='pitch')
    with pytest.raises(ValueError):
        PitchTracker(DEV)(x, S.SR, S.HOP, lengths=[1])
