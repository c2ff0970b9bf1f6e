"""GPU: the sentence phonemizer — its three kernels against float64 torch on the host, CubenetPhonemizer / Text2FeatBlizzard against fixtures
made by the reference (tools/gen_golden_phonemizer.py), batched == single bit for bit, training parity and determinism, the plain-text
path of TTSCube, and the trainer script."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import meldecoder_ref as M
from oracle.fingerprint import probe_vector
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LOGIT_TOL = 1e-4        # the project's gate for teacher-forced logits
MARGIN = 2 * LOGIT_TOL  # a tag is compared wherever the reference's top-2 logit margin is at least this
MAX_LEFT_OUT = 0.05     # ... and the positions left out may be at most this share of a text


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def _enc_of(g):
    from ttscube_amd.io_utils.io_phonemizer import PhonemizerEncodings
    enc = PhonemizerEncodings()
    obj = json.loads(str(g['enc']))
    enc._grapheme2int, enc._phon2int = obj['grapheme2int'], obj['phon2int']
    return enc


def _net_of(g, train=False):
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))]
    net = CubenetPhonemizer(_enc_of(g))
    net.load_state_dict(M.fill_state_dict(shapes, int(g['seed'])), strict=True)
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _status():
    from ttscube_amd import _lib
    return int(_lib.lib().ttsc_phonemizer_status())


# ---- kernels alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,lengths', [(1, 37, None), (3, 50, [50, 1, 17]), (5, 129, [129, 128, 0, 64, 3])])
def test_char_features_moves_values_exactly(B, N, lengths):
    from ttscube_amd.networks.phonemizer import char_features
    rng = np.random.RandomState(B)
    G = 60
    ct, st = torch.from_numpy(rng.randn(G, 32).astype(np.float32)), torch.from_numpy(rng.randn(2, 8).astype(np.float32))
    xc, xs = torch.from_numpy(rng.randint(0, G, size=(B, N))), torch.from_numpy(rng.randint(0, 2, size=(B, N)))
    want = torch.cat([ct[xc], st[xs]], dim=-1).permute(0, 2, 1).contiguous()
    ld = None
    if lengths is not None:
        want = want * (torch.arange(N)[None, :] < torch.tensor(lengths)[:, None]).float()[:, None, :]
        ld = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    _status()
    got = char_features(xc.to(DEV), xs.to(DEV), ct.to(DEV), st.to(DEV), ld).cpu()
    assert got.shape == (B, 40, N) and torch.equal(got, want)
    assert _status() == 0


def test_char_features_out_of_range_id_writes_zeros_and_sets_the_status_bit():
    from ttscube_amd._lib import TTSCError
    from ttscube_amd.networks.phonemizer import char_features, check_status
    rng = np.random.RandomState(1)
    ct, st = torch.from_numpy(rng.randn(10, 32).astype(np.float32)), torch.from_numpy(rng.randn(2, 8).astype(np.float32))
    xc, xs = torch.tensor([[1, 10, 3, -1, 2]]), torch.tensor([[0, 1, 2, 0, 1]])
    _status()
    got = char_features(xc.to(DEV), xs.to(DEV), ct.to(DEV), st.to(DEV)).cpu()
    assert torch.equal(got[0, :32, [0, 2, 4]], ct[[1, 3, 2]].t()) and torch.equal(got[0, 32:, [0, 1, 3, 4]], st[[0, 1, 0, 1]].t())
    assert float(got[0, :32, [1, 3]].abs().max()) == 0.0 and float(got[0, 32:, 2].abs().max()) == 0.0
    with pytest.raises(TTSCError, match='outside its embedding table'):
        check_status('test')
    assert _status() == 0        # reading cleared it


@pytest.mark.parametrize('M_,P', [(37, 7), (123, 81), (1, 81), (65, 300), (9, 512)])
def test_tag_argmax_against_float64(M_, P):
    from ttscube_amd.networks.phonemizer import tag_argmax
    rng = np.random.RandomState(M_ + P)
    K = 400
    x = torch.from_numpy(rng.randn(M_, K).astype(np.float32))
    w = torch.from_numpy((rng.randn(P, K) / np.sqrt(K)).astype(np.float32))
    b = torch.from_numpy(rng.uniform(-0.1, 0.1, size=P).astype(np.float32))
    ref = x.double() @ w.double().t() + b.double()
    tags, logits = tag_argmax(x.to(DEV), w.to(DEV), b.to(DEV), want_logits=True)
    err = float((logits.cpu().double() - ref).abs().max())
    print('tag_argmax M=%d P=%d: |logit| rms %.3f, max-abs error %.3e' % (M_, P, float(ref.pow(2).mean().sqrt()), err))
    assert err <= 1e-5
    top = torch.topk(ref, 2, dim=-1).values
    sure = (top[:, 0] - top[:, 1]) > 2e-5
    assert tags.dtype == torch.int32 and torch.equal(tags.cpu().long()[sure], ref.argmax(dim=-1)[sure])
    # the arg-max is the arg-max of the kernel's own logits (first maximum), and the tags do not depend on whether the logits are written
    assert torch.equal(tags.cpu().long(), logits.cpu().argmax(dim=-1))
    tags2, none = tag_argmax(x.to(DEV), w.to(DEV), b.to(DEV))
    assert none is None and torch.equal(tags2, tags)


def test_tag_argmax_ties_ragged_rows_and_row_independence():
    from ttscube_amd.networks.phonemizer import tag_argmax
    rng = np.random.RandomState(5)
    K, P, B, N = 400, 81, 3, 21
    x = torch.from_numpy(np.abs(rng.randn(B, N, K)).astype(np.float32))
    w = torch.from_numpy((rng.randn(P, K) / np.sqrt(K)).astype(np.float32))
    w[5] = 0.05
    w[3] = w[5]                      # two equal rows that win everywhere: the lower index is the answer
    b = torch.zeros(P)
    lens = [21, 0, 10]
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tags, logits = tag_argmax(x.to(DEV), w.to(DEV), b.to(DEV), ld, N, want_logits=True)
    tags, logits = tags.cpu(), logits.cpu()
    assert tags.shape == (B, N)
    for i, n in enumerate(lens):
        assert tags[i, :n].tolist() == [3] * n and tags[i, n:].tolist() == [0] * (N - n)
        assert torch.equal(logits[i, :n, 3], logits[i, :n, 5]) and float(logits[i, n:].abs().max() if n < N else 0.0) == 0.0
    # a row gives the same bits alone, in another batch, and at another place in a tile
    solo_t, solo_l = tag_argmax(x[2:3, 7:8].contiguous().to(DEV), w.to(DEV), b.to(DEV), want_logits=True)
    assert torch.equal(solo_l.cpu()[0, 0], logits[2, 7]) and int(solo_t.cpu()[0, 0]) == int(tags[2, 7])
    shifted_t, shifted_l = tag_argmax(x[:, 1:].contiguous().to(DEV), w.to(DEV), b.to(DEV), want_logits=True)
    assert torch.equal(shifted_l.cpu()[0], logits[0, 1:])


@pytest.mark.parametrize('R,K', [(77, 81), (1, 7), (1031, 300)])
def test_masked_ce_against_float64(R, K):
    from ttscube_amd.networks.phonemizer import masked_ce
    rng = np.random.RandomState(R)
    lg = torch.from_numpy(rng.randn(R, K).astype(np.float32))
    tg = torch.from_numpy(rng.randint(1 if R == 1 else 0, K, size=R))
    if R > 1:
        tg[::3] = 0
    ref_in = lg.double().requires_grad_(True)
    ref = F.cross_entropy(ref_in, tg, ignore_index=0)
    ref.backward()
    x = lg.to(DEV).requires_grad_(True)
    _status()
    loss, status = masked_ce(x, tg.to(DEV), 0)
    loss.backward()
    e_loss, e_grad = abs(float(loss.detach()) - float(ref.detach())), float((x.grad.cpu().double() - ref_in.grad).abs().max())
    print('masked_ce R=%d K=%d: loss %.6f, loss error %.3e, gradient max-abs error %.3e' % (R, K, float(ref), e_loss, e_grad))
    assert e_loss <= 1e-6 and e_grad <= 1e-6
    assert int(status.item()) == 0 and _status() == 0
    loss2, _ = masked_ce(lg.to(DEV), tg.to(DEV), 0)
    assert torch.equal(loss2, loss.detach())          # fixed-order reduction: the same bits again


def test_masked_ce_all_ignored_and_bad_targets():
    from ttscube_amd.networks.phonemizer import masked_ce
    rng = np.random.RandomState(3)
    R, K = 50, 81
    lg = torch.from_numpy(rng.randn(R, K).astype(np.float32))
    x = lg.to(DEV).requires_grad_(True)
    loss, status = masked_ce(x, torch.zeros(R, dtype=torch.long, device=DEV), 0)
    loss.backward()
    assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0 and int(status.item()) == 0      # (torch: NaN)
    tg = torch.from_numpy(rng.randint(1, K, size=R))
    good = tg.clone()
    tg[4], tg[9] = K + 3, -1
    good[4] = good[9] = 0                                 # what is left once the bad rows contribute nothing
    ref_in = lg.double().requires_grad_(True)
    ref = F.cross_entropy(ref_in, good, ignore_index=0)
    ref.backward()
    _status()
    x = lg.to(DEV).requires_grad_(True)
    loss, status = masked_ce(x, tg.to(DEV), 0)
    loss.backward()
    assert abs(float(loss) - float(ref)) <= 1e-6 and float((x.grad.cpu().double() - ref_in.grad).abs().max()) <= 1e-6
    assert int(status.item()) == 2 and _status() == 2 and _status() == 0


# ---- reference parity, inference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b', 'long'])
def test_forward_and_tags_match_the_reference(name):
    g = _golden('phonemizer_' + name)
    net = _net_of(g)
    X = {'x_char': torch.from_numpy(g['x_char']), 'x_case': torch.from_numpy(g['x_case'])}
    ref = torch.from_numpy(g['logits'])
    logits = net(X).cpu()
    err = float((logits - ref).abs().max())
    top = torch.topk(ref, 2, dim=-1).values
    margin = top[..., 0] - top[..., 1]
    sure = margin >= MARGIN
    left_out = 1.0 - float(sure.float().mean())
    tags, tlog = net.tag(X, return_logits=True)
    print('phonemizer_%s: %d characters, logits max-abs error %.3e, min margin %.3e, left out %.2f %%, tags differing %d'
          % (name, ref.shape[1], err, float(margin.min()), 100 * left_out, int((tags.cpu().long() != torch.from_numpy(g['tags'])).sum())))
    assert logits.shape == ref.shape and err <= LOGIT_TOL
    assert left_out <= MAX_LEFT_OUT
    assert torch.equal(tags.cpu().long()[sure], torch.from_numpy(g['tags'])[sure])
    assert float((tlog.cpu() - ref).abs().max()) <= LOGIT_TOL
    assert torch.equal(net.tag(X), tags)


def _write_phonemizer(g, net, base):
    _enc_of(g).save(base + '.encodings')
    net.save(base + '.model')


def test_text2feat_equals_the_reference_dict(tmp_path):
    from ttscube_amd.io_utils.io_text import Text2FeatBlizzard
    g = _golden('phonemizer_a')
    top = torch.topk(torch.from_numpy(g['logits']), 2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) >= MARGIN          # the fixture the whole dict is compared on
    base = str(tmp_path / 'phonemizer')
    _write_phonemizer(g, _net_of(g), base)
    t2f = Text2FeatBlizzard(base, device=DEV)
    assert t2f._phonemizer is not None and not t2f._phonemizer.training
    assert t2f(str(g['text'])) == json.loads(str(g['result']))


def test_batched_equals_single_bit_for_bit(tmp_path):
    from ttscube_amd import _lib
    from ttscube_amd.io_utils.io_phonemizer import encode_text
    from ttscube_amd.io_utils.io_text import Text2FeatBlizzard, normalize_text
    g = _golden('phonemizer_b')
    base = str(tmp_path / 'phonemizer')
    _write_phonemizer(g, _net_of(g), base)
    t2f = Text2FeatBlizzard(base, device=DEV)
    texts = ["Hello.", "Don't stop me now, I'm having such a good time!", "A", "Well,\nwell.\n\nWhat have we here?",
             "The rain in Spain stays mainly in the plain; or so they say.", "Yes", "It's nine o'clock on a Saturday: the regular crowd shuffles in.",
             "Good morning and welcome to the world of speech synthesis, where every sentence gets its tags alone and in company!"]
    together = t2f.batch(texts)
    singles = [t2f(t) for t in texts]
    assert together == singles
    assert len({len(d['orig_text']) for d in singles}) == len(texts)      # ragged
    norm = [normalize_text(t) for t in texts]
    B, N = len(norm), max(len(t) for t in norm)
    xc, xs = np.zeros((B, N), dtype=np.int64), np.zeros((B, N), dtype=np.int64)
    for i, t in enumerate(norm):
        encode_text(t2f._encodings, t, xc[i], xs[i])
    lens = [len(t) for t in norm]
    net = t2f._phonemizer
    tags, logits = net.tag({'x_char': torch.from_numpy(xc), 'x_case': torch.from_numpy(xs)}, lengths=_lib.DevLengths(lens, device=DEV), return_logits=True)
    for i, n in enumerate(lens):
        t1, l1 = net.tag({'x_char': torch.from_numpy(xc[i:i + 1, :n].copy()), 'x_case': torch.from_numpy(xs[i:i + 1, :n].copy())}, return_logits=True)
        assert torch.equal(l1[0], logits[i, :n]), i
        assert torch.equal(t1[0], tags[i, :n]) and int(tags[i, n:].abs().sum()) == 0
    _lib.check_split_status('test_batched_equals_single')


# ---- reference parity, training -----------------------------------------------------------------------------------------------------------
def _batch_of(g):
    return {'x_char': torch.from_numpy(g['x_char']), 'x_case': torch.from_numpy(g['x_case']), 'y_phon': torch.from_numpy(g['y_phon'])}


@pytest.mark.parametrize('name', ['phonemizer_train_a', 'phonemizer_train_b'])
def test_training_step_matches_the_reference(name):
    g = _golden(name)
    net = _net_of(g, train=True)
    batch = _batch_of(g)
    assert int((batch['y_phon'] == 0).sum()) > 0 and len(set(g['lengths'].tolist())) > 1
    logits = net(batch)
    assert logits.requires_grad
    e_logits = float((logits.detach().cpu() - torch.from_numpy(g['logits'])).abs().max())
    loss = net.training_step(batch, 0)
    e_loss = abs(float(loss) - float(g['loss']))
    worst, worst_probe = 0.0, 0.0
    names = json.loads(str(g['grad_names']))
    assert names == [k for k, _ in net.named_parameters()]
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        got = p.grad.detach().cpu().double().numpy().reshape(-1)
        if 'grad/%s/full' % k in g.files:
            worst = max(worst, float(np.abs(got - g['grad/%s/full' % k]).max()))
            continue
        assert got.size == int(g['grad/%s/size' % k])
        worst = max(worst, float(np.abs(got[g['grad/%s/idx' % k]] - g['grad/%s/samples' % k]).max()))
        # every element within LOGIT_TOL bounds the probe (a dot product with a fixed N(0,1) vector z) by LOGIT_TOL * sum |z|
        z = probe_vector(k, got.size)
        e_probe = abs(float(got @ z) - float(g['grad/%s/probe' % k]))
        worst_probe = max(worst_probe, e_probe / float(np.abs(z).sum()))
        assert e_probe <= LOGIT_TOL * float(np.abs(z).sum()), k
        assert abs(float(np.sqrt((got * got).sum())) - float(g['grad/%s/norm' % k])) <= LOGIT_TOL * np.sqrt(got.size), k
    print('%s: loss %.6f (error %.3e), logits max-abs error %.3e, gradients max-abs error %.3e (probe / sum|z| %.3e)'
          % (name, float(loss), e_loss, e_logits, worst, worst_probe))
    assert e_logits <= LOGIT_TOL and e_loss <= LOGIT_TOL and worst <= LOGIT_TOL


def _run_steps(g, n):
    torch.manual_seed(0)
    net = _net_of(g, train=True)
    batch = _batch_of(g)
    losses = [net.training_step(batch, i) for i in range(n)]
    torch.cuda.synchronize()
    return net, [float(v) for v in losses]


def test_three_step_runs_are_bit_identical():
    g = _golden('phonemizer_train_a')
    n1, l1 = _run_steps(g, 3)
    n2, l2 = _run_steps(g, 3)
    assert l1 == l2
    for (k, a), (_, b) in zip(n1.state_dict().items(), n2.state_dict().items()):
        assert torch.equal(a, b), k
    assert not torch.equal(n1.state_dict()['_output_softmax.weight'].cpu(), M.fill_state_dict(
        [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))], int(g['seed']))['_output_softmax.weight'])      # it did move


def test_thirty_steps_lower_the_loss_and_eval_still_works():
    from ttscube_amd import _lib
    from ttscube_amd.networks.phonemizer import check_status
    g = _golden('phonemizer_train_a')
    net, losses = _run_steps(g, 31)
    print('loss at step 0 %.4f, at step 30 %.4f' % (losses[0], losses[30]))
    assert losses[30] < losses[0]
    check_status('test')
    _lib.check_split_status('test')
    net.eval()
    batch = _batch_of(g)
    out = net.validation_step(dict(batch), 0)
    assert out['pred'].shape == out['target'].shape == tuple(batch['y_phon'].shape) and np.isfinite(out['loss'])
    net.validation_epoch_end([out])
    assert 0.0 <= net._val_pacc <= 1.0 and 0.0 <= net._val_sacc <= 1.0
    with torch.no_grad():
        ref = F.cross_entropy(net(batch).cpu().double().reshape(-1, len(net._encodings.phonemes)),
                              batch['y_phon'].reshape(-1), ignore_index=0)
    assert abs(out['loss'] - float(ref)) <= 1e-4


# ---- public interface -----------------------------------------------------------------------------------------------------------------------
def test_ttscube_takes_plain_text(tmp_path):
    from tests.test_api_gpu import _Enc, _make_model_dir
    from ttscube_amd.api import PhoneText2Feat, TTSCube
    from ttscube_amd.io_utils.io_phonemizer import PhonemizerEncodings
    from ttscube_amd.io_utils.io_text import Text2FeatBlizzard
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    base, _, _ = _make_model_dir(tmp_path)
    enc = PhonemizerEncodings()
    enc._grapheme2int = {g: i for i, g in enumerate(['PAD', '§', ' '] + list("abcdefghijklmnopqrstuvwxyz',.!?"))}
    enc._phon2int = {p: i for i, p in enumerate(['PAD', '_'] + sorted(_Enc().phon2int))}
    pbase = os.path.join(str(tmp_path), 'phonemizer')
    enc.save(pbase + '.encodings')
    net = CubenetPhonemizer(enc)
    net.load_state_dict(M.fill_state_dict(M.named_shapes(net), 31), strict=True)
    net.save(pbase + '.model')
    tts = TTSCube(base, pbase)
    plain = TTSCube(base, None)
    assert isinstance(tts._text2feat, Text2FeatBlizzard) and isinstance(plain._text2feat, PhoneText2Feat)
    assert tts._text2feat._phonemizer is not None

    def phoneme_string(text):
        rez = tts._text2feat(text)
        per_word = [[] for _ in rez['words']]
        for p, w in zip(rez['phones'], rez['phon2word']):
            per_word[w].append(p)
        again = plain._text2feat('|'.join(' '.join(ps) for ps in per_word))
        assert again['phones'] == rez['phones'] and again['phon2word'] == rez['phon2word']
        return '|'.join(' '.join(ps) for ps in per_word), rez

    texts = ["Good morning, Bob!", "It's a fine day.\nIsn't it?", "Yes.", "Well, well: what have we here?\n\nA second paragraph."]
    singles = []
    for t in texts:
        s, rez = phoneme_string(t)
        assert len(rez['phones']) > 0
        a, b = tts(t, speaker='s1'), plain(s, speaker='s1')
        assert a.dtype == np.int16 and a.shape == b.shape and np.array_equal(a, b), t
        singles.append(a)
    for got, want in zip(tts.synthesize_batch(texts, speaker='s1'), singles):
        assert got.shape == want.shape and np.array_equal(got, want)


def test_trainer_script_writes_files_the_front_end_loads(tmp_path):
    from ttscube_amd.io_utils.io_text import Text2FeatBlizzard
    base = str(tmp_path / 'phonemizer')
    data = os.path.join(GOLDEN, 'phonemizer_dev.json')
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'train_phonemizer.py'), '--output-base', base, '--train-file', data, '--dev-file', data,
           '--batch-size', '4', '--num-workers', '0', '--max-steps', '5']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)      # a fresh child process under its own time limit
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'steps 5' in r.stdout and 'Val PACC' in r.stdout
    for ext in ('.encodings', '.last'):
        assert os.path.exists(base + ext), ext
    shutil.copy(base + '.last', base + '.model')
    t2f = Text2FeatBlizzard(base, device=DEV)
    rez = t2f('Enfin, la soirée finit.')
    assert rez['orig_text'] == '§Enfin, la soirée finit.§' and ''.join(rez['words']) == rez['orig_text']
    assert len(rez['phones']) == len(rez['phon2word']) <= len(rez['orig_text']) and '_' not in rez['phones']
