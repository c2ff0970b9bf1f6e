"""GPU: training and running Cubegan with word-vector conditioning (`conditioning='fasttext:<lang>'`, vectors from a local table).

  1-2  ttsc_phone_rows_assemble / _bwd (csrc/train_ops.hip) against the cat / repeat / index formulation: the forward bit for bit, the adjoint against
       that formulation differentiated in float64 with a bound made from the float64 side;
  3    Languasito2(cond_type='fasttext').forward in training mode against vectors made by the reference itself
       (tools/gen_golden_cond_training.py -> tests/golden/languasito2_ft_train_a.npz);
  4    two Cubegan training steps with the crop path active: every word-encoder parameter moves, two fresh runs end on the same bits;
  5    scripts/train_cubegan.py --lm fasttext:xx -> scripts/export_model.py -> api.TTSCube."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from oracle.fingerprint import compare
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

B_, N_, NW_ = 2, 5, 3
PATTERNS = {
    'all_to_word_0': [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
    'one_word_skipped': [[0, 0, 2, 2, 2], [2, 2, 0, 0, 2]],                 # nobody points at word 1
    'non_monotone': [[2, 0, 1, 0, 2], [1, 2, 2, 0, 1]],
    'padding_zeros_after_the_true_length': [[0, 1, 1, 2, 2], [0, 1, 2, 0, 0]],   # utterance 1 has 3 phonemes; its padding rows carry 0
}
# the real widths (char BiLSTM 512, speaker embedding 128, word BiLSTM 512); 4 / 4 / 4: every part is ONE 16-byte access; 5 / 3 / 6: no part is a
# multiple of one, the element-wise kernel runs
WIDTHS = [(512, 128, 512), (4, 4, 4), (5, 3, 6)]


def _operands(widths, seed=0):
    Ch, Cs, Cw = widths
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B_, N_, Ch, generator=g), torch.randn(B_, 1, Cs, generator=g), torch.randn(B_, NW_, Cw, generator=g),
            torch.randn(B_, N_, Ch + Cs + Cw, generator=g))


def _formulation(h, spk, cond, p2w):
    """modules.py:930-940 / 1079-1082 as torch writes it"""
    sel = torch.gather(cond, 1, p2w[:, :, None].expand(-1, -1, cond.shape[2]))
    return torch.cat([h, spk.repeat(1, h.shape[1], 1), sel], dim=-1)


@pytest.mark.parametrize('widths', WIDTHS, ids=lambda w: 'x'.join(map(str, w)))
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_phone_rows_assemble_forward_is_bit_equal_to_cat_repeat_index(widths, pattern):
    from ttscube_amd.networks.text_autograd import phone_rows_assemble
    h, spk, cond, _ = _operands(widths)
    p2w = torch.tensor(PATTERNS[pattern])
    out = phone_rows_assemble(h.cuda(), spk.cuda(), cond.cuda(), p2w)
    assert out.shape == (B_, N_, sum(widths))
    assert torch.equal(out.cpu(), _formulation(h, spk, cond, p2w))


@pytest.mark.parametrize('widths', WIDTHS, ids=lambda w: 'x'.join(map(str, w)))
@pytest.mark.parametrize('pattern', sorted(PATTERNS))
def test_phone_rows_assemble_adjoint_matches_float64_within_the_summation_bound(widths, pattern):
    """Every gradient element is a sum of at most N terms of gout, added in fp32 one after the other: its error is at most N * 2^-23 * sum |terms|
    (each of the <= N - 1 additions rounds a partial sum no larger than sum |terms| by at most 2^-24 relative; N * 2^-23 leaves a factor two).  sum |terms|
    comes from the float64 side: the adjoint is linear in gout with coefficients 0 / 1, so differentiating the formulation against |gout| gives it."""
    from ttscube_amd.networks.text_autograd import phone_rows_assemble
    h, spk, cond, gout = _operands(widths)
    p2w = torch.tensor(PATTERNS[pattern])

    def adjoint(g):
        leaves = [t.double().requires_grad_(True) for t in (h, spk, cond)]
        _formulation(*leaves, p2w).backward(g.double())
        return [t.grad for t in leaves]
    want, sums = adjoint(gout), adjoint(gout.abs())

    def native():
        leaves = [t.cuda().requires_grad_(True) for t in (h, spk, cond)]
        phone_rows_assemble(*leaves, p2w).backward(gout.cuda())
        torch.cuda.synchronize()
        return [t.grad.cpu() for t in leaves]
    got, again = native(), native()
    for name, g, w, s in zip(('gh', 'gspk', 'gcond'), got, want, sums):
        assert g.shape == w.shape and g.dtype == torch.float32, name
        err, bound = (g.double() - w).abs(), N_ * 2.0 ** -23 * s
        print('%s %s %s: max error %.3e, bound at that element %.3e' % (pattern, widths, name, float(err.max()), float(bound.flatten()[err.argmax()])))
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
    assert torch.equal(got[0], gout[:, :, :widths[0]])                       # a copy
    for b in range(B_):
        for w in range(NW_):
            if w not in PATTERNS[pattern][b]:
                assert bool((got[2][b, w] == 0).all()), (b, w)               # a word no phoneme points at: exact zeros
    assert all(torch.equal(a, b) for a, b in zip(got, again))                # two launches, the same bits


def test_phone_rows_assemble_rejects_an_index_outside_the_words_before_it_launches(monkeypatch):
    from ttscube_amd import _lib
    from ttscube_amd.networks.text_autograd import phone_rows_assemble
    h, spk, cond, _ = _operands((4, 4, 4))
    launched = []
    real = _lib.lib().ttsc_phone_rows_assemble
    monkeypatch.setattr(_lib.lib(), 'ttsc_phone_rows_assemble', lambda *a: launched.append(a) or real(*a))
    for bad in ([[0, 1, 2, 3, 0], [0, 0, 0, 0, 0]], [[0, 1, 2, -1, 0], [0, 0, 0, 0, 0]]):
        with pytest.raises(_lib.TTSCError):
            phone_rows_assemble(h.cuda(), spk.cuda(), cond.cuda(), torch.tensor(bad))
    assert not launched
    phone_rows_assemble(h.cuda(), spk.cuda(), cond.cuda(), torch.tensor(PATTERNS['non_monotone']))
    assert len(launched) == 1                                                # (the counter does see a launch)


# ---- 3: the reference's own training-mode forward, losses and gradients ---------------------------------------------------------------------------
def test_word_conditioned_training_forward_losses_and_gradients_match_the_reference(golden_dir):
    """Thresholds: those of tests/test_reference_goldens_gpu.py for languasito2_train_* — outputs, losses and every gradient fingerprint within 1e-4.
    The fixture's `replay_check` is the same comparison made by its generator with this project's formulation in float64 on the CPU: 1.2e-6 for the
    `_lm_*` tensors (1.9e-6 over all tensors), far inside 1e-4, so the plain gate holds for the word encoders too and no widened one is used."""
    from ttscube_amd.networks import training as T
    from ttscube_amd.networks.modules import Languasito2
    z = np.load(os.path.join(golden_dir, 'languasito2_ft_train_a.npz'))
    assert float(z['replay_check']) < 1e-4 and float(z['replay_check_all']) < 1e-4
    shapes = [(k, tuple(s)) for k, s in json.loads(str(z['shapes']))]
    cfg = json.loads(str(z['cfg']))
    net = Languasito2(cfg['num_phones'], cfg['num_speakers'], cfg['max_pitch'], cfg['max_duration'], cond_type='fasttext')
    assert M.named_shapes(net) == shapes
    net.load_state_dict(M.fill_state_dict(shapes, int(z['seed'])), strict=True)
    net = net.cuda().train()
    f2ps, o = [], 0
    for n in z['f2p_len']:
        f2ps.append([int(v) for v in z['f2p_flat'][o:o + int(n)]])
        o += int(n)
    X = {'x_char': torch.from_numpy(z['x_char']), 'x_speaker': torch.from_numpy(z['x_speaker']), 'y_frame2phone': f2ps,
         'y_pitch': torch.from_numpy(z['y_pitch']), 'y_dur': torch.from_numpy(z['y_dur']), 'x_words': torch.from_numpy(z['x_words']),
         'x_phon2word': torch.from_numpy(z['x_phon2word']), 'x_tok_ids': None}
    p_dur, p_pitch, p_vuv, cond = net(X)                   # Languasito2.forward -> the differentiable HIP path; NotImplementedError before this feature
    assert p_dur.requires_grad and cond.requires_grad
    for got, key in ((p_dur, 'p_dur'), (p_pitch, 'p_pitch'), (p_vuv, 'p_vuv'), (cond, 'conditioning')):
        assert got.shape == z[key].shape, key
        d = float((got.detach().cpu() - torch.from_numpy(z[key])).abs().max())
        print(key, 'max abs deviation %.3e' % d)
        assert d < 1e-4, key
    l_dur, l_pitch = T.text_losses(p_dur, p_pitch, p_vuv, X['y_dur'].cuda(), X['y_pitch'].cuda(), cfg['max_pitch'],
                                   int(max(cfg['max_pitch'], cfg['max_duration']) + 1))
    print('losses', float(l_dur.detach()) - float(z['loss_duration']), float(l_pitch.detach()) - float(z['loss_pitch']))
    assert abs(float(l_dur.detach()) - float(z['loss_duration'])) < 1e-4 and abs(float(l_pitch.detach()) - float(z['loss_pitch'])) < 1e-4
    l_cond = (cond * torch.from_numpy(z['cond_probe']).cuda()).sum() / cond.numel()
    (l_dur + l_pitch + l_cond).backward()
    torch.cuda.synchronize()
    params = dict(net.named_parameters())
    names = json.loads(str(z['grad_names']))
    assert sum(k.startswith('_lm_t.') for k in names) == 16 and sum(k.startswith('_lm_g.') for k in names) == 16
    bad, worst = {}, (0.0, None)
    for k in names:
        assert params[k].grad is not None, k
        fp = {f: z['grad/%s/%s' % (k, f)] for f in ('norm', 'sum', 'probe', 'idx', 'samples', 'size')}
        dev = compare(params[k].grad.cpu().numpy(), k, fp)
        worst = max(worst, (max(dev.values()), k))
        if max(dev.values()) > 1e-4:
            bad[k] = dev
    print('worst gradient fingerprint deviation %.3e (%s)' % worst)
    assert not bad, bad


# ---- 4: the step --------------------------------------------------------------------------------------------------------------------------------
def _conditioned_run(steps=2):
    from ttscube_amd.io_utils.io_cubegan import CubeganCollate
    from ttscube_amd.io_utils.synthetic import SYNTHETIC_VOCABULARY, synthetic_encodings, synthetic_examples
    from ttscube_amd.io_utils.word_vectors import WordVectors
    from ttscube_amd.networks import training as T
    from ttscube_amd.networks.cubegan import Cubegan
    enc = synthetic_encodings()
    table = WordVectors.synthetic(SYNTHETIC_VOCABULARY, dim=300, seed=5)
    batch = CubeganCollate(enc, conditioning_type='fasttext:xx', word_vectors=table).collate_fn(
        list(synthetic_examples(2, 31, min_ph=12, max_ph=20, words=4)))
    assert batch['y_audio'].shape[1] > 11760 and batch['x_words'].shape[1] > 4      # the crop path; words behind a left context
    torch.manual_seed(0)
    model = Cubegan(enc, conditioning='fasttext:xx', train=True).cuda().train()
    opts = T.cubegan_configure_optimizers(model)
    lm = {k: p.detach().clone() for k, p in model._languasito.named_parameters() if k.startswith('_lm_')}
    rng = random.Random(1)
    outs = [dict(T.cubegan_training_step(model, batch, opts, rng=rng)) for _ in range(steps)]
    torch.cuda.synchronize()
    return model, lm, outs


def test_conditioned_cubegan_steps_move_the_word_encoders_and_are_reproducible():
    model, lm0, outs = _conditioned_run()
    assert len(lm0) == 32
    for out in outs:
        assert all(np.isfinite(v) for v in out.values()), out
    now = dict(model._languasito.named_parameters())
    still = [k for k, p0 in lm0.items() if torch.equal(p0, now[k].detach())]
    assert not still, still
    first = {k: v.detach().clone() for k, v in model.state_dict().items()}
    del model
    again, _, _ = _conditioned_run()
    differ = [k for k, v in again.state_dict().items() if not torch.equal(v, first[k])]
    assert not differ, differ[:8]


# ---- 5: trainer -> export -> TTSCube --------------------------------------------------------------------------------------------------------------
def test_trainer_export_and_api_round_trip_with_word_vectors(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    from ttscube_amd import _lib
    from ttscube_amd.api import TTSCube
    from ttscube_amd.io_utils.word_vectors import WordVectors
    base = str(tmp_path / 'cg')
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_cubegan.py'), '--synthetic', '4', '--lm', 'fasttext:xx', '--epochs', '1',
                          '--batch-size', '2', '--num-workers', '1', '--output-base', base], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    import yaml
    assert yaml.safe_load(open(base + '.yaml'))['conditioning'] == 'fasttext:xx'
    assert os.path.exists(base + '.vectors.npz') and os.path.exists(base + '.last')
    import export_model
    import tarfile
    import io
    nvol = export_model.export_model(base, str(tmp_path / 'pack'))
    blob = b''.join(open('%s-%02d' % (tmp_path / 'pack', i), 'rb').read() for i in range(nvol))
    with tarfile.open(fileobj=io.BytesIO(blob)) as tar:
        assert sorted(tar.getnames()) == ['cubegan.encodings', 'cubegan.model', 'cubegan.vectors.npz', 'cubegan.yaml']
    def text2feat(text):          # two phonemes per word
        words = text.split()
        return {'words': words, 'phones': ['p%d' % (1 + i % 7) for i in range(2 * len(words))], 'phon2word': [i // 2 for i in range(2 * len(words))]}
    sentence = 'w1 w2 w3'
    table = WordVectors(base + '.vectors.npz')
    tts = TTSCube(base, None, text2feat=text2feat, word_vectors=table)
    audio = tts(sentence, speaker='s0')
    assert audio.dtype == np.int16 and audio.size > 0
    assert np.array_equal(audio, TTSCube(base, None, text2feat=text2feat)(sentence, speaker='s0'))       # the table beside the model is the default
    # sentences of different word counts in one padded batch: the word BiLSTMs stop at each sentence's own last word, so every result is the
    # single-sentence call's
    texts = ['w1 w2 w3', 'w9 w4', 'w5 w6 w7 w8 w1 w30', 'w2']
    for t, got in zip(texts, tts.synthesize_batch(texts, speaker='s0', max_batch=4)):
        solo = tts(t, speaker='s0')
        assert got.shape == solo.shape and np.array_equal(got, solo), t
    words = sorted(table._index)
    vecs = np.stack([table.get_word_vector(w) for w in words])
    vecs[words.index('w2')] = -vecs[words.index('w2')] + 0.5
    other = TTSCube(base, None, text2feat=text2feat, word_vectors=WordVectors(words=words, vectors=vecs))(sentence, speaker='s0')
    assert other.shape != audio.shape or not np.array_equal(other, audio)                                # one word's vector changes the audio
    os.rename(base + '.vectors.npz', base + '.moved.npz')
    with pytest.raises(_lib.TTSCError, match='word_vectors'):
        TTSCube(base, None, text2feat=text2feat)                                                         # at construction, not at the first call
