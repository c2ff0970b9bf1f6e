"""GPU: the HIP polyphase resampler (csrc/resample.hip, io_utils/resample.py) against its float64 statement (tests/resample_reference.py) within
the derived rounding bound, bit-identical rows alone and in ragged batches, 64-bit indexing on a long row, and the batched vocoder feature cache
(VocoderDataset.precompute) against the same steps taken file by file."""
import filecmp
import os

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from tests import resample_reference as R
from ttscube_amd.io_utils import resample as RS

pytestmark = pytest.mark.gpu

CASES = [(1, 2, 1000), (80, 147, 1500), (8, 147, 3000), (3, 2, 700), (160, 147, 900), (1, 10, 501), (3, 1, 37)]


@pytest.fixture(scope='module')
def resampler():
    return RS.Resampler()


def _row(L, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=L).astype(np.float32)


def _check_against_reference(y, ref, A, up, down, what):
    err, lim = np.abs(y.astype(np.float64) - ref), R.bound(A, up, down)
    worst = float((err[A > 0] / lim[A > 0]).max()) if (A > 0).any() else 0.0
    print('%s: max |y - ref| = %.3e, worst error / bound = %.3f' % (what, err.max() if err.size else 0.0, worst))
    assert (err <= lim).all()
    assert not y[A == 0].any()                                # nothing but zeros went into these


@pytest.mark.parametrize('up,down,L', CASES)
def test_one_row_within_the_rounding_bound(resampler, up, down, L):
    x = _row(L, 10 * up + down)
    y = resampler.resample_poly(x, up, down)
    assert y.dtype == np.float32 and y.shape == (RS.out_len(L, up, down),)
    ref, A = R.resample(x, up, down)
    _check_against_reference(y, ref, A, up, down, 'up=%d down=%d L=%d' % (up, down, L))
    assert np.array_equal(RS.resample_poly(x, up, down), y)   # scipy's call shape, the same launch


@pytest.mark.parametrize('up,down,L', [(1, 50, 40000), (250, 7, 40), (7, 250, 30000)])
def test_ratios_whose_span_or_filter_does_not_fit_lds(resampler, up, down, L):
    """the same loop reads the input span (1 / 50: 13 754 floats a tile), the filter (250 / 7: 6 000 taps) or both (7 / 250) through L2"""
    x = np.stack([_row(L, 3 * up + down), _row(L, 5 * up + down)])
    lens = [L, L - L // 3]
    y = resampler.resample_poly(x, up, down, lengths=lens)
    for b in range(2):
        n = RS.out_len(lens[b], up, down)
        ref, A = R.resample(x[b, :lens[b]], up, down)
        _check_against_reference(y[b, :n], ref, A, up, down, 'up=%d down=%d L=%d' % (up, down, lens[b]))
        assert not y[b, n:].any() and np.array_equal(resampler.resample_poly(x[b, :lens[b]].copy(), up, down), y[b, :n])


def _length_for(n_out, up, down):
    """a row length whose output length is n_out"""
    L = n_out * down // up
    while RS.out_len(L, up, down) < n_out:
        L += 1
    assert RS.out_len(L, up, down) == n_out, (n_out, up, down)
    return L


@pytest.mark.parametrize('up,down', [(80, 147), (8, 147), (3, 1)])
def test_ragged_batch_rows_are_bit_identical_to_rows_alone(resampler, up, down):
    lens = [1500, 1, 0, _length_for(2 * RS.TILE + 1, up, down), _length_for(RS.TILE - 1, up, down)]
    Lmax = max(lens)
    x = np.stack([_row(Lmax, 50 + b) for b in range(len(lens))])      # what lies behind a row's length is not zero: it must not be read
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    yd, out_lens, peak = resampler.resample_device(xd, ld, down * 300, up * 300)
    y, peak = yd.cpu().numpy(), peak.cpu().numpy()
    assert y.shape == (len(lens), RS.out_len(Lmax, up, down)) and out_lens.tolist() == [RS.out_len(v, up, down) for v in lens]
    assert np.array_equal(resampler(x, down * 300, up * 300, lengths=lens), y)
    for b, L in enumerate(lens):
        n = RS.out_len(L, up, down)
        assert not y[b, n:].any()
        assert peak[b] == (np.abs(y[b]).max() if n else 0.0)
        if L:
            alone = resampler.resample_poly(x[b, :L].copy(), up, down)
            assert alone.shape == (n,) and np.array_equal(alone, y[b, :n])
    assert not y[2].any() and peak[2] == 0.0
    pair = resampler.resample_poly(x[[4, 1], :lens[4]].copy(), up, down, lengths=[lens[4], 1])       # another batch, another row pitch
    n1 = RS.out_len(1, up, down)
    assert np.array_equal(pair[0], y[4, :RS.TILE - 1]) and np.array_equal(pair[1, :n1], y[1, :n1]) and not pair[1, n1:].any()


def test_long_row_indexes_past_2_to_the_31(resampler):
    up, down, L = 160, 147, 13500000
    x = _row(L, 99)
    yd, out_lens, peak = resampler.resample_poly_device(torch.from_numpy(x).cuda().unsqueeze(0), torch.tensor([L], dtype=torch.int32).cuda(), up, down)
    O = RS.out_len(L, up, down)
    assert (O - 1) * down > 2 ** 31 and yd.shape == (1, O) and out_lens.tolist() == [O]
    idx = list(range(256)) + list(range(O - 256, O))
    y = torch.cat([yd[0, :256], yd[0, O - 256:]]).cpu().numpy()
    ref, A = R.resample(x, up, down, outputs=idx)
    _check_against_reference(y, ref, A, up, down, 'up=160 down=147 L=13500000, first and last 256 outputs')
    assert float(peak[0]) == float(yd.abs().max())


# ---- the vocoder feature cache ----------------------------------------------------------------------------------------------------------------------

def _write(path, rate, seconds, seed, channels=1):
    rng = np.random.RandomState(seed)
    t = np.arange(int(rate * seconds)) / rate
    x = 0.5 * np.sin(2 * np.pi * rng.uniform(100, 300) * t) + 0.2 * rng.uniform(-1, 1, size=t.size)
    if channels == 2:
        x = np.stack([x, 0.5 * x[::-1]], axis=1)
    scipy.io.wavfile.write(path, rate, np.asarray(x * 0.8 * 32767, dtype=np.int16))


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp('vocoder_cache')
    wavs = root / 'wavs'
    wavs.mkdir()
    _write(str(wavs / 'a441.wav'), 44100, 0.41, 1)
    _write(str(wavs / 'b441.wav'), 44100, 0.30, 2)
    _write(str(wavs / 'c480.wav'), 48000, 0.37, 3)
    _write(str(wavs / 'd240.wav'), 24000, 0.33, 4)
    _write(str(wavs / 'e441_stereo.wav'), 44100, 0.35, 5, channels=2)
    return root, str(wavs)


def test_precompute_writes_what_the_steps_give_file_by_file(folder, resampler, monkeypatch):
    from ttscube_amd.io_utils import io_vocoder
    from ttscube_amd.io_utils.audio import read_wav
    from ttscube_amd.io_utils.vocoder import MelVocoder
    root, wavs = folder
    caches = {k: str(root / ('cache_' + k)) for k in ('b1', 'b3', 'lazy')}
    ds1 = io_vocoder.VocoderDataset(wavs, cache_dir=caches['b1'])
    ds3 = io_vocoder.VocoderDataset(wavs, cache_dir=caches['b3'])
    assert len(ds1) == 5
    assert ds1.precompute(batch=1) == 5 and ds3.precompute(batch=3, resampler=resampler) == 5
    names = sorted(os.listdir(caches['b1']))
    assert len(names) == 15 and names == sorted(os.listdir(caches['b3']))
    match, mismatch, errors = filecmp.cmpfiles(caches['b1'], caches['b3'], names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)

    lazy = io_vocoder.VocoderDataset(wavs, cache_dir=caches['lazy'])
    vocoder = MelVocoder()
    for i, path in enumerate(ds1._examples):
        samples, rate = read_wav(path)
        base = ds1._cache_base(path)
        got = {k: np.load(base + '.' + k + '.npy') for k in ('audio', 'audio_low', 'mgc')}
        for key, sr in (('audio', 24000), ('audio_low', 2400)):
            y = resampler(samples, rate, sr)
            want = (y / np.float32(np.abs(y).max())) * np.float32(0.98)
            assert want.dtype == np.float32 and got[key].dtype == np.float32 and np.array_equal(got[key], want), (path, key)
        mel = vocoder.melspectrogram(got['audio'], 24000, 80, 240)
        assert got['mgc'].dtype == mel.dtype and got['mgc'].shape == mel.shape and got['mgc'].tobytes() == mel.tobytes(), path
        assert abs(float(np.abs(got['audio']).max()) - 0.98) <= 2.0 ** -23
        for g, w in zip((got['audio'], got['audio_low'], got['mgc']), lazy[i]):                 # the lazy path: scipy + one spectrogram per file
            assert g.shape == w.shape and g.dtype == w.dtype, path
    assert sorted(os.listdir(caches['lazy'])) == names

    def no_load(*a, **k):
        raise AssertionError('load_wav was called')
    monkeypatch.setattr(io_vocoder, 'load_wav', no_load)
    for i in range(len(ds1)):
        wav, wav_low, mel = ds1[i]
        assert wav.ndim == 1 and mel.shape == (1 + len(wav) // 240, 80)
    assert ds1.precompute(batch=2) == 0


def test_load_wav_on_the_resampler(folder, resampler):
    from ttscube_amd.io_utils.audio import load_wav, read_wav
    _, wavs = folder
    for name in ('a441.wav', 'c480.wav', 'e441_stereo.wav'):
        path = os.path.join(wavs, name)
        got, sr = load_wav(path, 24000, resampler=resampler)
        host, _ = load_wav(path, 24000)                       # (the default path, for the shape)
        samples, rate = read_wav(path)
        up, down = RS.ratio(rate, 24000)
        ref, A = R.resample(samples, up, down)
        assert sr == 24000 and got.dtype == np.float32 and got.shape == host.shape == ref.shape
        _check_against_reference(got, ref, A, up, down, name)
