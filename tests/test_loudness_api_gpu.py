"""GPU: loudness targets through the public interface (TTSCube, TTSCubeTwoStage, StoryCube) on the tiny seeded models of test_api_gpu.py and
test_twostage_gpu.py: every result, measured by the float64 statement tests/loudness_reference.py, sits at its target or at the peak ceiling."""
import math

import numpy as np
import pytest
import torch

from tests import loudness_reference as R
from tests import story_reference as SR

pytestmark = pytest.mark.gpu

SR_HZ = 24000
TARGET, PEAK_DB = -23.0, -1.0
CEILING = 10.0 ** (PEAK_DB / 20.0)


def _float(a):
    return a.astype(np.float64) / 32767.0                    # the int16 conversion of the API is trunc(w * 32767)


def _quantisation_lu(m):
    """how far truncation to int16 can move the loudness of a row: every sample moves by less than one step, the K-weighting amplifies by at
    most its shelf (+4 dB) -> 20 log10(1 + 1.585 / (32767 rms))"""
    return 20.0 * math.log10(1.0 + 10.0 ** (4.0 / 20.0) / (32767.0 * math.sqrt(m['zbar'])))


def _check_rows(rows, reports, target=TARGET, tol=0.01):
    """each int16 row reads `target` within tol LU, or is reported peak-limited with its peak at the ceiling"""
    seen = []
    for i, (a, rep) in enumerate(zip(rows, reports)):
        m = R.measure(_float(a), SR_HZ)
        seen.append((len(a), round(m['lufs'], 4), rep['peak_limited']))
        assert not rep['silent'] and not m['silent'], i
        if rep['peak_limited']:
            peak = max(m['sample_peak'], m['true_peak'])
            assert abs(peak / CEILING - 1.0) < 1e-3 and m['lufs'] < target, (i, peak, m['lufs'])
        else:
            assert abs(m['lufs'] - target) <= tol, (i, m['lufs'])
            assert max(m['sample_peak'], m['true_peak']) <= CEILING * (1.0 + 1e-3)
        assert rep['lufs_in'] + rep['gain_db'] == pytest.approx(m['lufs'], abs=tol)
    print('rows (samples, LUFS, peak-limited):', seen)
    return seen


def _texts():
    rng = np.random.RandomState(0)
    syms = 'a b c d e f g h i j k l m n o p'.split()
    return [' '.join(rng.choice(syms, size=n)) for n in (9, 3, 14, 6, 11)]


def test_ttscube_batch_at_a_target(tmp_path):
    from tests.test_api_gpu import _make_model_dir
    from ttscube_amd.api import TTSCube
    base, _, _ = _make_model_dir(tmp_path)
    tts = TTSCube(base, None)
    texts = _texts()
    plain = tts.synthesize_batch(texts, speaker='s0', max_batch=3)
    none = tts.synthesize_batch(texts, speaker='s0', max_batch=3, loudness=None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, none))
    got = tts.synthesize_batch(texts, speaker='s0', max_batch=3, loudness=TARGET, peak_db=PEAK_DB)
    reports = tts.loudness_report()
    assert len(got) == len(reports) == len(texts)
    for a, b in zip(got, plain):
        assert a.dtype == np.int16 and a.shape == b.shape
    _check_rows(got, reports)
    for i, t in enumerate(texts):
        assert np.array_equal(tts(t, speaker='s0', loudness=TARGET, peak_db=PEAK_DB), got[i]), i
    # one target per text; a sentence with a break is measured as the joined unit, its pause included
    targets = [-30.0, -26.0, -23.0, -20.0, -33.0]
    per = tts.synthesize_batch(texts, speaker='s0', max_batch=2, loudness=targets)
    for i, (a, rep) in enumerate(zip(per, tts.loudness_report())):
        _check_rows([a], [rep], target=targets[i])
    marked = 'a b c <break time="300ms"/> d e f g'
    joined = tts.synthesize_batch([marked, texts[0]], speaker='s0', markup=[True, False], loudness=TARGET)
    rep = tts.loudness_report()
    _check_rows(joined, rep)
    assert np.array_equal(joined[1], got[0])
    assert np.array_equal(tts(marked, speaker='s0', markup=True, loudness=TARGET), joined[0])
    # joined units go through padded batches of max_batch texts: one text per batch gives the same bytes and a report for every text
    one = tts.synthesize_batch([marked, texts[0]], speaker='s0', markup=[True, False], loudness=TARGET, max_batch=1)
    assert all(np.array_equal(a, b) for a, b in zip(one, joined))
    assert len(tts._loud_log[1]) == 2 and [r['gain_db'] for r in tts.loudness_report()] == [r['gain_db'] for r in rep]
    assert tts(texts[0], speaker='s0').tobytes() == plain[0].tobytes()


def test_storycube_paragraphs_at_a_target(tmp_path):
    from tests.test_api_gpu import _make_model_dir
    from ttscube_amd.api import TTSCube
    from ttscube_amd.story import StoryCube
    base, _, _ = _make_model_dir(tmp_path)
    tts = TTSCube(base, None)
    text = 'a b c | d e f g | h a\n\nk\n\ne f g h i j | a b | c d'
    parts = text.split('\n\n')
    assert len(parts) == 3 and len(parts[1].split()) == 1
    story = StoryCube(None, cube=tts, music=np.zeros(1000, dtype=np.float32))
    plain = story(text, speaker='s1')
    loud = story(text, speaker='s1', loudness=TARGET, peak_db=PEAK_DB)
    assert loud['meta'] == plain['meta'] and loud['audio'].shape == plain['audio'].shape and loud['audio'].dtype == np.int16
    assert story(text, speaker='s1', loudness=None)['audio'].tobytes() == plain['audio'].tobytes()
    lengths = [len(tts(p, speaker='s1')) for p in parts]
    offsets, total, _ = SR.timeline_literal(lengths, parts)
    assert total == loud['audio'].size
    reports = tts.loudness_report()
    covered = np.zeros(total, dtype=bool)
    for i, (o, n) in enumerate(zip(offsets, lengths)):
        cut = loud['audio'][o:o + n]
        covered[o:o + n] = True
        m = R.measure(_float(cut), SR_HZ)
        print('paragraph %d: %d samples, %.4f LUFS, peak-limited %s, quantisation bound %.4f' % (i, n, m['lufs'], reports[i]['peak_limited'],
                                                                                             _quantisation_lu(m)))
        _check_rows([cut], [reports[i]], tol=_quantisation_lu(m) + 1e-6)
    assert not loud['audio'][~covered].any()                 # a music bed of zeros: nothing but the paragraphs


def test_two_stage_at_a_target(tmp_path):
    from tests import test_twostage_cpu as TS
    from tests.test_twostage_gpu import _model_dir
    from ttscube_amd.api import TTSCubeTwoStage
    base, vck = _model_dir(tmp_path)
    tts = TTSCubeTwoStage(base, vck)
    sents = TS.sentences_five()
    texts = [TS.phone_text(s) for s in sents]
    spk = [str(s[1] - 1) for s in sents]
    s0 = 4242
    plain = tts.synthesize_batch(texts, speaker=spk, seed=s0, max_batch=3)
    none = tts.synthesize_batch(texts, speaker=spk, seed=s0, max_batch=3, loudness=None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, none))
    got = tts.synthesize_batch(texts, speaker=spk, seed=s0, max_batch=3, loudness=TARGET, peak_db=PEAK_DB)
    reports = tts.loudness_report()
    assert [a.shape for a in got] == [a.shape for a in plain]
    _check_rows(got, reports)
    for i in range(len(texts)):
        assert np.array_equal(tts(texts[i], speaker=spk[i], seed=s0 + i, loudness=TARGET, peak_db=PEAK_DB), got[i]), i
    gap = tts.synthesize_batch([texts[0], '', texts[2]], speaker=[spk[0], spk[0], spk[2]], seed=s0, max_batch=3, loudness=TARGET)
    assert len(gap[1]) == 0 and np.array_equal(gap[0], got[0]) and np.array_equal(gap[2], got[2])
    assert tts.loudness_report()[1]['silent']
