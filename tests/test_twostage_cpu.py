"""CPU: the parts of the two-stage text-to-speech path that need no GPU — the AR launch planner (networks/textcoder_plan.py), the argument
parsing of scripts/synthesize.py, and the INPUT CONDITION of tests/test_twostage_gpu.py: on every sentence those tests use, the float64 oracle's
largest duration logit leads the second-largest by at least 1e-3 at every phone, so an fp32 run cannot pick another duration than float64.

The sentences of the GPU tests are defined here (seeded; `sentences_*`), so that both files speak about the same inputs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from tests.conftest import ROOT

PFRAMES = 3
NET_SEED = 93              # fill_state_dict seed of the small Textcoder (the `_Enc` model of tests/test_meldecoder_gpu.py: 40 phones, max_duration 9)
SEED_FIVE = 0            # RandomState seeds of the sentence sets: chosen so that the input condition below holds (and asserted there)
SEED_FORTY = 1
LENS_FIVE = [13, 6, 9, 1, 11]
OOV_ROW = 2                # the sentence of the five whose LAST phone is out of the vocabulary (id 0, inside its x_len)
DUR_GAP = 1e-3


class Enc:
    """the `_Enc` of tests/test_meldecoder_gpu.py (that module is GPU-marked as a whole; the numbers are restated, and compared in the GPU tests)"""
    phon2int = {str(i): i for i in range(40)}
    speaker2int = {str(i): i for i in range(2)}
    max_pitch = 200
    max_duration = 9


def _sentences(lens, seed, oov_row=None):
    """-> list of (phone ids [n] int64 in 1..40, 0 = out of vocabulary; speaker id 1..2)"""
    rng = np.random.RandomState(seed)
    out = []
    for b, n in enumerate(lens):
        ids = rng.randint(1, 41, size=n).astype(np.int64)
        if b == oov_row:
            ids[-1] = 0
        out.append((ids, int(rng.randint(1, 3))))
    return out


def sentences_five():
    return _sentences(LENS_FIVE, SEED_FIVE, OOV_ROW)


SCRIPT_SPEAKER = '1'       # scripts/synthesize.py takes ONE speaker for the whole file: the five sentences, all spoken by this one (id 2)


def sentences_script():
    return [(ids, Enc.speaker2int[SCRIPT_SPEAKER] + 1) for ids, _ in sentences_five()]


def sentences_forty():
    rng = np.random.RandomState(1000 + SEED_FORTY)
    return _sentences([int(v) for v in rng.randint(3, 9, size=40)], SEED_FORTY)


def padded_batch(sents):
    """the batch dict CubenetTextcoder.inference_batch takes: x_char padded with 0, x_speaker [B, 1], x_len"""
    n = max(len(s[0]) for s in sents)
    x = np.zeros((len(sents), n), dtype=np.int64)
    for b, (ids, _) in enumerate(sents):
        x[b, :len(ids)] = ids
    return {'x_char': torch.from_numpy(x), 'x_speaker': torch.tensor([[s[1]] for s in sents]), 'x_len': torch.tensor([len(s[0]) for s in sents])}


def solo_batch(sent):
    return {'x_char': torch.from_numpy(sent[0])[None, :], 'x_speaker': torch.tensor([[sent[1]]])}


def phone_text(sent):
    """the sentence as a phone string for api.PhoneText2Feat; the out-of-vocabulary phone is spelled 'zz'"""
    return ' '.join('zz' if i == 0 else str(int(i) - 1) for i in sent[0])


_SD = {}


def state_dict():
    """the small Textcoder's fill_state_dict weights (shared, never modified)"""
    if 'sd' not in _SD:
        from ttscube_amd.networks.textcoder import CubenetTextcoder
        _SD['sd'] = M.fill_state_dict(M.named_shapes(CubenetTextcoder(Enc(), pframes=PFRAMES)), NET_SEED)
    return _SD['sd']


def duration_gaps(sd, sent):
    """float64 oracle duration head of one sentence -> (durations [n], gap between the two largest logits of every phone [n], fp32 durations [n])"""
    x, spk = torch.from_numpy(sent[0])[None, :], torch.tensor([[sent[1]]])
    with torch.no_grad():
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        lg = M.textcoder_text_stack(sd64, x, spk)[1][0]
        d32 = torch.argmax(M.textcoder_text_stack(sd, x, spk)[1][0], dim=-1)
    top = torch.topk(lg, 2, dim=-1).values
    return torch.argmax(lg, dim=-1).tolist(), (top[:, 0] - top[:, 1]).tolist(), d32.tolist()


# ---- 10. planner ---------------------------------------------------------------------------------------------------------------------------
def _plan():
    spec = importlib.util.spec_from_file_location('_textcoder_plan_alone', os.path.join(ROOT, 'ttscube_amd', 'networks', 'textcoder_plan.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # (loaded by path: the module must not need the package, let alone the library)
    return mod.plan_ar_launches


@pytest.mark.parametrize('steps,max_rows', [([5, 0, 7, 7, 1], 2), ([3], 1), ([0, 0], 4), ([], 3), ([9, 8, 7, 6, 5, 4, 3, 2, 1], 3), ([4] * 40, 32),
                                            ([2, 9, 0, 9, 1, 9], 1), (list(range(70)), 32)])
def test_planner_covers_every_row_once_longest_first(steps, max_rows):
    plan = _plan()(steps, max_rows)
    flat = [b for rows in plan for b in rows]
    assert sorted(flat) == [b for b, s in enumerate(steps) if s > 0]                 # every row with steps once, zero-step rows in no launch
    assert all(1 <= len(rows) <= max_rows for rows in plan)
    assert [steps[b] for b in flat] == sorted((s for s in steps if s > 0), reverse=True)   # longest first, across the launches too
    assert len(plan) == -(-len(flat) // max_rows)                                     # no launch left half empty before the last
    for rows in plan:
        assert steps[rows[0]] == max(steps[b] for b in rows)                          # a launch's first row sets its horizon


def test_planner_is_stable_and_refuses_bad_arguments():
    plan = _plan()
    assert plan([4, 4, 4], 2) == [[0, 1], [2]]                                        # ties keep the row order
    assert plan([1, 3, 2], 8) == [[1, 2, 0]]
    with pytest.raises(ValueError):
        plan([1, 2], 0)
    with pytest.raises(ValueError):
        plan([1, -2], 2)


# ---- 11. script arguments ------------------------------------------------------------------------------------------------------------------
def _script():
    spec = importlib.util.spec_from_file_location('_synthesize_script', os.path.join(ROOT, 'scripts', 'synthesize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_synthesize_script_arguments(tmp_path):
    S = _script()
    p = S.parser().parse_args(['--textcoder', 'tc', '--vocoder', 'griffinlim', '--input', 'in.txt', '--output-folder', 'out'])
    assert (p.textcoder, p.vocoder, p.input, p.output_folder) == ('tc', 'griffinlim', 'in.txt', 'out')
    assert (p.phonemizer, p.speaker, p.batch, p.seed, p.device) == (None, 'none', 32, 0, 'cuda:0')
    p = S.parser().parse_args(['--textcoder', 'tc', '--vocoder', 'g_1', '--phonemizer', 'ph', '--input', 'i', '--output-folder', 'o', '--speaker', 'anca',
                               '--batch', '4', '--seed', '17', '--device', 'cuda:1'])
    assert (p.vocoder, p.phonemizer, p.speaker, p.batch, p.seed, p.device) == ('g_1', 'ph', 'anca', 4, 17, 'cuda:1')
    for missing in ('--textcoder', '--vocoder', '--input', '--output-folder'):
        argv = ['--textcoder', 'tc', '--vocoder', 'v', '--input', 'i', '--output-folder', 'o']
        k = argv.index(missing)
        with pytest.raises(SystemExit):
            S.parser().parse_args(argv[:k] + argv[k + 2:])
    with pytest.raises(SystemExit):
        S.check(S.parser().parse_args(['--textcoder', 'tc', '--vocoder', 'v', '--input', 'i', '--output-folder', 'o', '--batch', '0']))
    with pytest.raises(SystemExit):
        S.check(S.parser().parse_args(['--textcoder', 'tc', '--vocoder', 'v', '--input', 'i', '--output-folder', 'o', '--seed', '-1']))
    f = tmp_path / 'in.txt'
    f.write_text('1 2 3\n\n  4 5 | 6  \n')
    assert S.read_sentences(str(f)) == ['1 2 3', '4 5 | 6']
    (tmp_path / 'empty.txt').write_text('\n')
    with pytest.raises(SystemExit):                                                   # refused before the package (and a GPU) is needed
        S.main(['--textcoder', 'tc', '--vocoder', 'v', '--input', str(tmp_path / 'empty.txt'), '--output-folder', str(tmp_path / 'o')])


# ---- 12. input condition of the GPU tests --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['five', 'script', 'forty'])
def test_duration_logits_of_the_test_sentences_are_well_separated(which):
    sd = state_dict()
    sents = {'five': sentences_five, 'script': sentences_script, 'forty': sentences_forty}[which]()
    if which != 'forty':
        assert [len(s[0]) for s in sents] == LENS_FIVE and sents[OOV_ROW][0][-1] == 0 and all((s[0][:-1] > 0).all() for s in sents)
    else:
        assert len(sents) == 40 and all(3 <= len(s[0]) <= 8 for s in sents)
    worst = np.inf
    for i, s in enumerate(sents):
        d64, gaps, d32 = duration_gaps(sd, s)
        worst = min(worst, min(gaps))
        assert min(gaps) >= DUR_GAP, '%s sentence %d: duration logit gap %.3g < %g at phone %d' % (which, i, min(gaps), DUR_GAP, int(np.argmin(gaps)))
        assert d32 == d64, '%s sentence %d: the oracle picks other durations in fp32 than in float64' % (which, i)
    print('%s: smallest duration-logit gap %.3g' % (which, worst))


def test_enc_restates_the_small_model_of_the_ar_tests():
    """the numbers this file restates are those of tests/test_meldecoder_gpu.py::_Enc (read from its source: importing it needs nothing, but it is
    the GPU module's; a drift between the two would make the CPU condition speak about another model)"""
    src = open(os.path.join(ROOT, 'tests', 'test_meldecoder_gpu.py')).read()
    body = src[src.index('class _Enc:'):src.index('def _ar_reference')]
    assert 'range(40)' in body and 'range(2)' in body and 'max_pitch = 200' in body and 'max_duration = 9' in body
