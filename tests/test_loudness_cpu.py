"""CPU: the float64 statement of the loudness meter (tests/loudness_reference.py) and the host code of io_utils/loudness.py — no kernel runs."""
import json
import math
import os

import numpy as np
import pytest

from tests import loudness_reference as R
from tests.conftest import ROOT


def _mod():
    from ttscube_amd.io_utils import loudness
    return loudness


def test_k_weighting_at_48k_is_the_printed_table():
    M = _mod()
    assert np.abs(M.k_weighting(48000) - R.TABLE_48K).max() < 1e-12
    assert np.abs(R.k_weighting(48000) - R.TABLE_48K).max() < 1e-12
    for sr in (16000, 22050, 24000, 44100, 48000):
        assert np.array_equal(M.k_weighting(sr), R.k_weighting(sr))


def test_recursion_equals_sosfilt():
    x = np.random.default_rng(1).standard_normal(5000)
    for sr in (16000, 24000, 48000):
        y, ys = R.kfilter(x, sr), R.kfilter_fast(x, sr)
        assert np.abs(y - ys).max() <= 1e-13 * np.abs(ys).max()


def test_full_scale_997_hz_sine():
    read = {}
    for sr in (48000, 24000, 16000):
        x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * sr) / sr)
        read[sr] = R.measure(x, sr, fast=True)['lufs']
    assert abs(read[48000] - (-3.01)) <= 0.005
    assert abs(read[24000] - (-2.9843)) < 1e-4               # the documented figures of the bilinear re-design
    assert abs(read[16000] - (-2.9700)) < 1e-4
    # the mistake the re-design avoids: the 48 kHz table applied unchanged at 24 kHz
    from scipy.signal import sosfilt
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * 24000) / 24000)
    y = sosfilt(R.TABLE_48K, x)
    wrong = R.gate(R.blocks(R.sub_energies(y, 24000), x.size, 24000))['lufs']
    assert abs(wrong - (-0.64)) < 0.01


@pytest.mark.parametrize('case,reads', [(3, -23.021), (4, -23.021), (5, -22.985)])
def test_tech3341_gating_sequences(case, reads):
    sr = 24000
    m = R.measure(R.tone_sequence(R.TECH3341[case], sr), sr, fast=True)
    assert abs(m['lufs'] - (-23.0)) <= 0.1
    assert abs(m['lufs'] - reads) < 1e-3
    z = m['z'][m['z'] > 0]
    lu = -0.691 + 10.0 * np.log10(z)                          # every block at least 1 LU from either gate
    assert np.abs(lu - (-70.0)).min() >= 1.0
    rel = -0.691 + 10.0 * math.log10(m['z'][m['abs_mask']].mean()) - 10.0
    assert np.abs(lu[lu > -70.0] - rel).min() >= 1.0


def test_short_empty_and_silent_rows():
    sr = 24000
    x = 0.1 * np.random.default_rng(2).standard_normal(9599)
    m = R.measure(x, sr)
    assert m['blocks'] == 1 and m['gated'] == 1 and not m['silent']
    assert m['zbar'] == pytest.approx(np.mean(R.kfilter(x, sr) ** 2), rel=1e-13)       # one block: the mean square of the whole row
    assert R.measure(x[:1], sr)['blocks'] == 1
    full = R.measure(0.1 * np.random.default_rng(3).standard_normal(9600 + 2400 + 5), sr)
    assert full['blocks'] == 2                                # whole sub-blocks only: the 5 trailing samples are in no block
    e = R.measure(np.zeros(0), sr)
    assert (e['blocks'], e['gated'], e['silent'], e['lufs'], e['sample_peak'], e['true_peak']) == (0, 0, True, -np.inf, 0.0, 0.0)
    s = R.measure(np.zeros(24000), sr)
    assert s['blocks'] == 7 and s['gated'] == 0 and s['silent'] and s['lufs'] == -np.inf
    q = R.measure(1e-5 * np.random.default_rng(4).standard_normal(24000), sr)          # -100 dBFS or so: under the absolute gate
    assert q['silent'] and q['blocks'] == 7
    assert R.gain(0.0, 0.0, True, -23.0) == (np.float32(1.0), False)


def test_gain_ceiling_and_max_gain():
    M = _mod()
    zbar = 10.0 ** ((-30.0 + 0.691) / 10.0)                   # a row at -30 LUFS
    g, lim = M.host_gain(zbar, 0.1, False, -23.0)
    assert not lim and 20.0 * math.log10(g) == pytest.approx(7.0, abs=1e-6)
    g, lim = M.host_gain(zbar, 0.5, False, -23.0, peak_db=-1.0)                        # 7 dB on a peak of -6.02 dB would pass -1 dB
    assert lim and float(g) * 0.5 == pytest.approx(10.0 ** (-1.0 / 20.0), rel=1e-6)
    g, lim = M.host_gain(zbar, 0.1, False, -23.0, max_gain_db=3.0)
    assert not lim and 20.0 * math.log10(g) == pytest.approx(3.0, abs=1e-6)
    assert M.host_gain(0.0, 0.0, True, -23.0) == (np.float32(1.0), False)
    for args in ((zbar, 0.1, False, -23.0), (zbar, 0.5, False, -23.0, -1.0), (zbar, 0.1, False, -23.0, -1.0, 3.0)):
        assert M.host_gain(*args) == R.gain(*args)
    x = np.random.default_rng(5).standard_normal(100).astype(np.float32)
    y = R.apply_gain(x, g)
    assert y.dtype == np.float32 and np.array_equal(y, (x.astype(np.float64) * np.float64(g)).astype(np.float32))   # one product, rounded once
    assert float(M.lufs(zbar)) == pytest.approx(-30.0, abs=1e-12) and M.lufs(0.0) == -np.inf


def test_refused_rates():
    M = _mod()
    for sr in (22055, 10 * (M.CHUNK - 1), 0, -24000, 24000.5):
        with pytest.raises(ValueError):
            M.check_rate(sr)
        with pytest.raises(ValueError):
            M.kernel_constants(sr)
    assert M.check_rate(10 * M.CHUNK) == 640 and M.check_rate(22050) == 22050


def test_kernel_constants():
    M = _mod()
    assert M.TILE == 256 * M.CHUNK and 1 << M.LEVELS == M.TILE // M.CHUNK
    k = M.kernel_constants(24000)
    assert k.shape == (10 + 16 * (M.LEVELS + 1),) and k.dtype == np.float64
    sos = M.k_weighting(24000)
    A = M.state_matrix(sos)
    assert max(abs(np.linalg.eigvals(A))) < 1.0
    P = k[10:].reshape(M.LEVELS + 1, 4, 4)
    assert np.abs(P[0] - np.linalg.matrix_power(A, M.CHUNK)).max() < 1e-12
    assert max(abs(np.linalg.eigvals(P[0]))) == pytest.approx(0.53, abs=0.01)          # spectral radius of A^64 at 24 kHz
    s = np.array([0.3, -0.2, 0.1, 0.05])                      # A is the step at zero input
    assert np.allclose(A @ s, M.cascade_step(sos, s, 0.0)[1], rtol=0, atol=1e-15)
    taps = M.true_peak_taps()
    h = R.tp_filter()
    assert taps.shape == (4, 21) and taps.dtype == np.float32
    for p in range(4):
        assert np.array_equal(taps[p][:len(h[p::4])].astype(np.float64), h[p::4]) and not taps[p][len(h[p::4]):].any()


def test_chunked_emulation_is_close_to_the_recursion():
    M = _mod()
    x = np.random.default_rng(6).standard_normal(2 * M.TILE + 333)
    sub, y = R.chunked_sub_energies(x, 24000, M.CHUNK, M.TILE)
    ys = R.kfilter(x, 24000)
    ref = R.sub_energies(ys, 24000)
    assert np.abs(y - ys).max() <= 1e-12 * np.abs(ys).max()
    assert np.abs(sub - ref).max() <= 1e-13 * ref.max()


class _ReferenceMeter:
    """LoudnessMeter.normalize on the restatement"""

    def normalize(self, rows, sr, target=-23.0, peak_db=-1.0):
        out, rep = [], []
        for x in rows:
            m = R.measure(np.asarray(x, dtype=np.float32), sr, fast=True)
            g, lim = R.gain(m['zbar'], max(m['sample_peak'], m['true_peak']), m['silent'], target, peak_db)
            gdb = 20.0 * math.log10(float(g))
            out.append(R.apply_gain(x, g))
            rep.append({'lufs_in': m['lufs'], 'lufs_out': m['lufs'] + gdb, 'gain_db': gdb, 'peak_limited': lim, 'silent': m['silent']})
        return out, rep


def test_normalize_script(tmp_path):
    import importlib.util
    from ttscube_amd.io_utils.audio import read_wav, save_wav
    spec = importlib.util.spec_from_file_location('normalize_loudness', os.path.join(ROOT, 'scripts', 'normalize_loudness.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    rng = np.random.default_rng(7)
    save_wav(str(src / 'a.wav'), 0.05 * rng.standard_normal(24000), 24000)
    save_wav(str(src / 'b.wav'), 0.2 * rng.standard_normal(30000), 24000)
    save_wav(str(src / 'c.wav'), 0.1 * rng.standard_normal(16000), 16000)
    save_wav(str(src / 'quiet.wav'), np.zeros(12000), 24000)
    report = script.main(['--input-folder', str(src), '--output-folder', str(dst), '--target', '-20', '--peak', '-1', '--batch', '2'],
                         meter=_ReferenceMeter())
    on_disk = json.load(open(dst / 'report.json'))
    assert on_disk['silent'] == ['quiet.wav'] == report['silent'] and sorted(on_disk['files']) == ['a.wav', 'b.wav', 'c.wav', 'quiet.wav']
    for name, sr in (('a.wav', 24000), ('b.wav', 24000), ('c.wav', 16000)):
        y, rate = read_wav(str(dst / name))
        assert rate == sr and on_disk['files'][name]['sample_rate'] == sr
        assert not on_disk['files'][name]['peak_limited']
        assert abs(R.measure(y, sr, fast=True)['lufs'] - (-20.0)) < 0.01           # int16 quantisation
        assert abs(on_disk['files'][name]['lufs_out'] - (-20.0)) < 1e-5
    q, _ = read_wav(str(dst / 'quiet.wav'))
    assert not q.any() and on_disk['files']['quiet.wav']['lufs_in'] is None and on_disk['files']['quiet.wav']['gain_db'] == 0.0
    (src / 'odd.wav').write_bytes((src / 'a.wav').read_bytes())
    import scipy.io.wavfile
    scipy.io.wavfile.write(str(src / 'odd.wav'), 22055, np.zeros(100, dtype=np.int16))
    with pytest.raises(ValueError):
        script.main(['--input-folder', str(src), '--output-folder', str(tmp_path / 'out2')], meter=_ReferenceMeter())
    assert not (tmp_path / 'out2').exists()
