"""CPU: the host side of the HIP resampler (io_utils/resample.py) — its filter design and output length against scipy, the float64 statement
(tests/resample_reference.py) against scipy.signal.resample_poly, the unchanged default of load_wav, and the absence of any CPU path."""
import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal

from tests import resample_reference as R
from ttscube_amd import _lib
from ttscube_amd.io_utils import resample as RS

CASES = [(1, 2, 1000), (80, 147, 1500), (8, 147, 3000), (3, 2, 700), (160, 147, 900), (1, 10, 501), (3, 1, 37)]


def _row(L, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=L)


@pytest.mark.parametrize('up,down,L', CASES)
def test_filter_design_is_scipys(up, down, L):
    half = 10 * max(up, down)
    want = scipy.signal.firwin(2 * half + 1, 1.0 / max(up, down), window=('kaiser', 5.0)) * up
    for h in (RS.design_filter(up, down), R.design_filter(up, down)):
        assert h.dtype == np.float64 and h.shape == want.shape
        err = np.abs(h - want).max()
        print('design_filter(%d, %d): max |h - firwin * up| = %.3e' % (up, down, err))
        assert err <= 1e-12
    taps = RS.padded_taps(up, down)
    K = -(-(2 * half + 1) // up)
    assert taps.dtype == np.float32 and taps.size == up * ((K + 3) // 4 * 4)
    assert np.array_equal(taps[:2 * half + 1], RS.design_filter(up, down).astype(np.float32))     # rounded to float32 once
    assert not taps[2 * half + 1:].any()


@pytest.mark.parametrize('up,down,L', CASES)
def test_out_len_is_scipys(up, down, L):
    for n in (L, L + 1, 1):
        want = scipy.signal.resample_poly(np.zeros(n), up, down).shape[0]
        assert RS.out_len(n, up, down) == want and R.out_len(n, up, down) == want


@pytest.mark.parametrize('up,down,L', CASES)
def test_float64_statement_is_scipys_resample_poly(up, down, L):
    x = _row(L, 100 + up + down)
    want = scipy.signal.resample_poly(x, up, down)
    y, A = R.resample(x, up, down)
    assert y.shape == want.shape
    err = np.abs(y - want).max()
    print('resample(%d, %d, L=%d): max |restatement - scipy| = %.3e' % (up, down, L, err))
    assert err <= 1e-12
    assert (A >= np.abs(y) - 1e-12).all()


def test_load_wav_default_is_unchanged(tmp_path):
    from ttscube_amd.io_utils.audio import load_wav, read_wav
    x = np.asarray(np.random.RandomState(7).uniform(-0.9, 0.9, size=6000) * 32767, dtype=np.int16)
    path = str(tmp_path / 'a.wav')
    scipy.io.wavfile.write(path, 44100, x)
    got, sr = load_wav(path, 24000)
    want = scipy.signal.resample_poly(x.astype(np.float32) / 32768.0, 80, 147).astype(np.float32)
    assert sr == 24000 and got.dtype == np.float32 and np.array_equal(got, want)
    raw, rate = read_wav(path)
    assert rate == 44100 and raw.dtype == np.float32 and np.array_equal(raw, x.astype(np.float32) / 32768.0)
    same, sr = load_wav(path, 44100)
    assert sr == 44100 and np.array_equal(same, raw)
    stereo = str(tmp_path / 's.wav')
    scipy.io.wavfile.write(stereo, 44100, np.stack([x, x[::-1]], axis=1))
    raw2, _ = read_wav(stereo)
    assert raw2.shape == raw.shape and np.array_equal(raw2, (np.stack([x, x[::-1]], axis=1).astype(np.float32) / 32768.0).mean(axis=1))


def test_no_cpu_path(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ttscube_amd.io_utils.io_vocoder import VocoderDataset
    with pytest.raises(_lib.TTSCError):
        RS.Resampler()(np.zeros(100, dtype=np.float32), 44100, 24000)
    with pytest.raises(_lib.TTSCError):
        RS.resample_poly(np.zeros(100, dtype=np.float32), 1, 2)
    folder = tmp_path / 'wavs'
    folder.mkdir()
    scipy.io.wavfile.write(str(folder / 'a.wav'), 44100, np.asarray(_row(6000, 1) * 30000, dtype=np.int16))
    ds = VocoderDataset(str(folder), cache_dir=str(tmp_path / 'cache'))
    assert len(ds) == 1
    with pytest.raises(_lib.TTSCError):
        ds.precompute()


def test_a_ratio_beyond_the_limit_is_refused_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'lib', no_library)
    r = RS.Resampler()
    with pytest.raises(ValueError, match='24000.*44101|44101.*24000'):
        r(np.zeros(100, dtype=np.float32), 44101, 24000)
    with pytest.raises(ValueError, match='1025'):
        RS.resample_poly(np.zeros(100, dtype=np.float32), 1025, 1)
    with pytest.raises(ValueError, match='1025'):
        r.resample_poly(np.zeros(100, dtype=np.float32), 3, 1025)
    assert RS.ratio(44100, 24000) == (80, 147) and RS.ratio(44100, 2400) == (8, 147) and RS.ratio(48000, 24000) == (1, 2)
    x = np.arange(5, dtype=np.float32)
    assert r(x, 24000, 24000) is x                            # equal rates: the input itself, nothing launched
