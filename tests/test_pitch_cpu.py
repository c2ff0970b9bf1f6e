"""CPU: the float64 restatement of the pitch tracker (tests/pitch_reference.py) finds the F0 of signals with a known answer — the thresholds of the
end-to-end check belong to the algorithm, not to the kernel — and the same text in float32 follows it."""
import numpy as np

from tests import pitch_reference as R
from tests import pitch_signals as S


def _tracks(dtype):
    x, lengths, _ = S.known_answer_batch()
    return R.rapt_f0(x, lengths, S.SR, S.HOP, S.FMIN, S.FMAX, dtype=dtype)


def test_lag_range_and_frame_count():
    assert R.params(24000, 60, 400) == (180, 60, 400, 341)
    assert R.params(16000, 30, 500) == (120, 32, 534, 503)
    x = np.zeros((1, 240 * 17 + 13), np.float32)
    assert R.rapt_f0(x, [x.shape[1]], 24000, 240).shape == (1, 17)
    assert R.rapt_f0(np.zeros((1, 100), np.float32), [100], 24000, 240).shape == (1, 0)


def test_digital_silence_is_unvoiced_and_phi_is_zero():
    phi, rms, maxphi = R.nccf(np.zeros(2400, np.float32), 2400, 24000, 240, 60, 400)
    assert phi.shape == (10, 341) and not phi.any() and not rms.any() and not maxphi.any()
    assert not R.rapt_f0(np.zeros((1, 2400), np.float32), [2400], 24000, 240).any()


def test_float64_restatement_on_known_answers():
    x, lengths, truth = S.known_answer_batch()
    f0 = _tracks(np.float64)
    for b in range(x.shape[0]):
        S.check_known_answer(f0[b].astype(np.float64), truth[b])


def test_float32_restatement_follows_float64():
    _, _, truth = S.known_answer_batch()
    f64, f32 = _tracks(np.float64), _tracks(np.float32)
    for b in range(f64.shape[0]):
        kind, _ = S.frame_classes(truth[b])
        assert S.disagreement(f64[b], f32[b], kind) <= 0.01


def test_candidates_order_and_refinement():
    phi = np.zeros((1, 12))
    phi[0, [2, 5, 8]] = [0.5, 0.9, 0.5]          # two equal peaks: the smaller lag comes first among them
    phi[0, 10] = 0.2                             # below 0.3 x 0.9
    lag, val, ncand = R.candidates(phi, 60)
    assert ncand[0] == 3
    assert np.allclose(lag[0, :3], [65, 62, 68]) and np.allclose(val[0, :3], [0.9, 0.5, 0.5])
    phi[0, 6] = 0.6                              # an asymmetric peak moves towards its larger neighbour
    lag, val, _ = R.candidates(phi, 60)
    assert 65 < lag[0, 0] < 65.5 and val[0, 0] > 0.9


def test_injected_tables_have_decided_cases():
    """at least half of the injected-table cases have a float64 optimum that is clear of ties (margin > 1e-3) and that float32 reproduces: on those
    the GPU test demands the identical path"""
    sol = S.table_solutions()
    decided = [s['margin'] > 1e-3 and s['same32'] for s in sol]
    assert sum(decided) * 2 >= len(decided), decided
    for s in sol:                                  # the optimum's own path costs what the tracker says it costs
        assert abs(R.path_cost(s['path'], *s['args'], S.TABLE_KMAX) - s['D_opt']) <= 1e-9 * max(s['D_opt'], 1.0)
