"""CPU: the numpy statements of the dev-set evaluation (tests/dtw_reference.py) against first principles, the DCT table and the score arithmetic of
io_utils/evaluate.py, and scripts/evaluate.py's argument surface and JSON layout around an injected host aligner.  No kernel runs here."""
import importlib.util
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import dtw_reference as R
from tests.conftest import ROOT


def _script():
    spec = importlib.util.spec_from_file_location('evaluate_script', os.path.join(ROOT, 'scripts', 'evaluate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_is_optimal_against_brute_force():
    rng = np.random.default_rng(1234)
    for Na in range(1, 6):
        for Nb in range(1, 6):
            a, b = rng.standard_normal((Na, 3)), rng.standard_normal((Nb, 3))
            D, path = R.dtw(a, b, np.float64)
            opt = R.brute_force(a, b)
            assert abs(D - opt) <= 1e-12 * max(opt, 1.0), (Na, Nb, D, opt)
            assert abs(R.path_cost64(a, b, path) - opt) <= 1e-12 * max(opt, 1.0)
            assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (Na - 1, Nb - 1)
            step = np.diff(path, axis=0)
            assert set(map(tuple, step)) <= {(1, 1), (1, 0), (0, 1)}


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_restatement_recovers_an_exact_warp(dt):
    a, b, w = R.exact_warp(np.random.default_rng(1234))
    assert a.shape[0] == 40 and b.shape[0] == 65 and np.all(np.diff(w) >= 0) and set(w) == set(range(40))
    D, path = R.dtw(a, b, dt)
    assert D == 0
    assert np.array_equal(path, np.stack([w, np.arange(65)], axis=1))


def test_tie_order_on_equal_frames():
    """every cost 0: the diagonal is taken while it exists, then (i-1, j) before (i, j-1) — walking back from the end"""
    for Na, Nb in ((5, 8), (8, 5), (6, 6)):
        a, b = np.ones((Na, 4), np.float32), np.ones((Nb, 4), np.float32)
        D, path = R.dtw(a, b, np.float32)
        assert D == 0
        m = min(Na, Nb)
        want = [(0, j) for j in range(Nb - m)] if Nb > Na else [(i, 0) for i in range(Na - m)]
        want += [(Na - m + k, Nb - m + k) for k in range(m)]
        assert [tuple(c) for c in path] == want


def test_dct_table_is_orthonormal_and_matches_the_restatement():
    from ttscube_amd.io_utils import evaluate as E
    T = E.dct_table(24, 80)
    assert T.dtype == np.float64 and T.shape == (24, 80)
    assert np.abs(T @ T.T - np.eye(24)).max() <= 1e-12
    full = E.dct_table(79, 80)
    assert np.abs(full @ full.T - np.eye(79)).max() <= 1e-12
    assert np.abs(T.sum(axis=1)).max() <= 1e-12               # c0 is dropped: every kept row is orthogonal to the constant
    assert np.array_equal(T, R.dct_table(24, 80))


def _metrics(path, cost, f_ref, f_syn, len_ref, len_syn):
    from ttscube_amd.io_utils import evaluate as E
    path = np.asarray(path, np.int32).reshape(-1, 2)
    Lp = len_ref + len_syn - 1
    pa, pb = np.full((1, Lp), -1, np.int32), np.full((1, Lp), -1, np.int32)
    pa[0, :len(path)], pb[0, :len(path)] = path[:, 0], path[:, 1]
    t = torch.from_numpy
    return E.path_metrics(t(pa), t(pb), torch.tensor([len(path)], dtype=torch.int32), torch.tensor([cost], dtype=torch.float32),
                          t(np.asarray(f_ref, np.float32)[None]), t(np.asarray(f_syn, np.float32)[None]),
                          torch.tensor([len_ref], dtype=torch.int32), torch.tensor([len_syn], dtype=torch.int32))


def test_path_metrics_on_hand_made_numbers():
    path = [(0, 0), (1, 1), (2, 1), (3, 2), (3, 3)]
    f_ref, f_syn = [0.0, 100.0, 100.0, 200.0], [0.0, 110.0, 250.0, 0.0]
    out = _metrics(path, 2.5, f_ref, f_syn, 4, 4)
    s = out['pairs'][0]
    # cells: (0,0) u/u; (1,1) 100/110; (2,1) 100/110; (3,2) 200/250 (gross: +25 %); (3,3) v/u
    assert s['n_path'] == 5 and s['n_both_voiced'] == 3
    assert s['mcd_db'] == pytest.approx(10.0 * math.sqrt(2.0) / math.log(10.0) * 2.5 / 5, rel=1e-12)
    assert s['f0_rmse_hz'] == pytest.approx(math.sqrt((100.0 + 100.0 + 2500.0) / 3), rel=1e-12)
    c1, c2 = 1200.0 * math.log2(1.1), 1200.0 * math.log2(1.25)
    assert s['f0_rmse_cents'] == pytest.approx(math.sqrt((2 * c1 * c1 + c2 * c2) / 3), rel=1e-12)
    assert s['gpe'] == pytest.approx(1.0 / 3) and s['vde'] == pytest.approx(1.0 / 5) and s['dur_ratio'] == 1.0
    ref, _ = R.path_metrics(path, 2.5, f_ref, f_syn, 4, 4)
    for k, v in ref.items():
        assert s[k] == pytest.approx(v, rel=1e-12), k
    assert out['corpus'] == s


def test_path_metrics_without_a_both_voiced_cell_gives_nan_not_zero():
    out = _metrics([(0, 0), (1, 1)], 1.0, [0.0, 120.0], [130.0, 0.0], 2, 2)
    s = out['pairs'][0]
    assert s['n_both_voiced'] == 0 and s['vde'] == 1.0
    for k in ('f0_rmse_hz', 'f0_rmse_cents', 'gpe'):
        assert math.isnan(s[k]), k
    assert math.isfinite(s['mcd_db'])
    empty = _metrics(np.zeros((0, 2)), 0.0, [100.0], [100.0], 1, 1)['pairs'][0]
    assert empty['n_path'] == 0 and math.isnan(empty['mcd_db']) and math.isnan(empty['vde'])


def test_corpus_scores_pool_sums_not_means():
    from ttscube_amd.io_utils import evaluate as E
    one = _metrics([(0, 0)], 3.0, [100.0], [110.0], 1, 1)
    two = _metrics([(0, 0), (1, 1), (2, 2)], 1.0, [100.0, 100.0, 0.0], [100.0, 100.0, 0.0], 3, 3)
    c = E.pool(one['sums'] + two['sums'])
    assert c['mcd_db'] == pytest.approx(E.MCD_SCALE * 4.0 / 4) and c['n_path'] == 4 and c['n_both_voiced'] == 3
    assert c['f0_rmse_hz'] == pytest.approx(math.sqrt(100.0 / 3))
    ref = R.pool([R.path_metrics([(0, 0)], 3.0, [100.0], [110.0], 1, 1)[1],
                  R.path_metrics([(0, 0), (1, 1), (2, 2)], 1.0, [100.0, 100.0, 0.0], [100.0, 100.0, 0.0], 3, 3)[1]])
    for k, v in ref.items():
        assert c[k] == pytest.approx(v, rel=1e-12, nan_ok=True), k


# ---- scripts/evaluate.py -----------------------------------------------------------------------------------------------------------------------------

def test_script_argument_surface():
    S = _script()
    a = S.parse_args(['--devset', 'd', '--generated', 'g'])
    assert (a.devset, a.generated, a.model, a.batch, a.limit, a.device, a.output, a.forced) == ('d', 'g', None, 32, -1, 'cuda:0', None, False)
    a = S.parse_args(['--devset', 'd', '--model', 'm', '--conditioning', 'fasttext:en', '--word-vectors', 'v.vec', '--forced', '--batch', '8',
                      '--limit', '5', '--device', 'cuda:1', '--output', 'o.json'])
    assert (a.model, a.conditioning, a.word_vectors, a.forced, a.batch, a.limit, a.device, a.output) == \
        ('m', 'fasttext:en', 'v.vec', True, 8, 5, 'cuda:1', 'o.json')
    for bad in (['--devset', 'd'], ['--generated', 'g'], ['--devset', 'd', '--generated', 'g', '--model', 'm'],
                ['--devset', 'd', '--generated', 'g', '--forced'], ['--devset', 'd', '--generated', 'g', '--batch', '0']):
        with pytest.raises(SystemExit):
            S.parse_args(bad)


def _host_aligner(a, len_a, b, len_b):
    """dtw_align's contract from the float64 restatement"""
    P, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    Lp = max(Na + Nb - 1, 0)
    out = {'cost': torch.zeros(P), 'plen': torch.zeros(P, dtype=torch.int32), 'path_a': torch.full((P, Lp), -1, dtype=torch.int32),
           'path_b': torch.full((P, Lp), -1, dtype=torch.int32)}
    for p in range(P):
        la, lb = int(len_a[p]), int(len_b[p])
        if la == 0 or lb == 0:
            continue
        D, path = R.dtw(a[p, :la].numpy(), b[p, :lb].numpy(), np.float64)
        out['cost'][p], out['plen'][p] = float(D), len(path)
        out['path_a'][p, :len(path)] = torch.from_numpy(path[:, 0].astype(np.int32))
        out['path_b'][p, :len(path)] = torch.from_numpy(path[:, 1].astype(np.int32))
    return out


def test_script_json_layout_with_an_injected_aligner(tmp_path):
    """the dev-set loop, the printed lines and the JSON file, with host stand-ins for the two kernels' callers: three items, the third one's
    synthesized copy is shifted, the second has no voiced frame"""
    from ttscube_amd.io_utils import evaluate as E
    from ttscube_amd.io_utils.audio import save_wav
    rng = np.random.default_rng(7)
    dev, gen = tmp_path / 'dev', tmp_path / 'gen'
    dev.mkdir()
    gen.mkdir()
    ids = ['FILE_%08d' % k for k in range(3)]
    for k, i in enumerate(ids):
        n = 6 + k
        mel = rng.standard_normal((n + 1, 80)).astype(np.float32)
        f0 = np.zeros(n) if k == 1 else np.where(np.arange(n) % 3 == 0, 0.0, 100.0 + 10.0 * k)
        with open(dev / (i + '.mgc'), 'wb') as f:
            np.save(f, mel)
        with open(dev / (i + '.pitch'), 'wb') as f:
            np.save(f, f0)
        json.dump({'id': i}, open(dev / (i + '.json'), 'w'))
        save_wav(str(gen / (i + '.wav')), np.zeros(240 * n, np.int16), 24000)

    class HostEvaluator(E.Evaluator):
        def analyse(self, x, lens):
            """the synthesized side = the stored reference features of the row with that many samples (the third shifted by a frame)"""
            mels, f0s = [], []
            for L in lens:
                k = L // 240 - 6
                mel = np.load(open(dev / (ids[k] + '.mgc'), 'rb'))[:L // 240]
                f0 = np.load(open(dev / (ids[k] + '.pitch'), 'rb')).astype(np.float32)
                if k == 2:
                    mel, f0 = np.roll(mel, 1, axis=0), np.roll(f0, 1)
                mels.append(torch.from_numpy(mel.copy()))
                f0s.append(torch.from_numpy(f0.copy()))
            m, f, n = self._pad_features(mels, f0s)
            return m, f, n

    ev = HostEvaluator('cpu', aligner=_host_aligner, cepstra=lambda m, n: torch.from_numpy(R.mel_cepstra(m.numpy(), n).astype(np.float32)))
    out = io.StringIO()
    path = tmp_path / 'metrics.json'
    assert _script().main(['--devset', str(dev), '--generated', str(gen), '--batch', '2', '--output', str(path)], evaluator=ev, out=out) == 0
    lines = out.getvalue().strip().split('\n')
    assert len(lines) == 4 and [ln.split()[0] for ln in lines[:3]] == ids and lines[3].startswith('corpus (3 items)')
    res = json.load(open(path))
    assert sorted(res) == ['corpus', 'items'] and [it['id'] for it in res['items']] == ids
    for rec in res['items'] + [res['corpus']]:
        assert set(E.SCORES) <= set(rec)
    a, b, c = res['items']
    assert a['mcd_db'] == 0 and a['f0_rmse_hz'] == 0 and a['vde'] == 0 and a['dur_ratio'] == 1 and a['n_path'] == 6
    assert b['n_both_voiced'] == 0 and b['f0_rmse_hz'] is None and b['gpe'] is None and b['mcd_db'] == 0      # nan is written as null
    assert c['mcd_db'] > 0 and c['n_path'] >= 8
    assert res['corpus']['n_path'] == a['n_path'] + b['n_path'] + c['n_path']
    assert res['corpus']['mcd_db'] == pytest.approx(sum(it['mcd_db'] * it['n_path'] for it in res['items']) / res['corpus']['n_path'])
    limited = ev.evaluate_devset(str(dev), str(gen), batch=32, limit=2)
    assert [it['id'] for it in limited['items']] == ids[:2]
