"""GPU: the word-level G2P — ttsc_g2p_decode against a float64 restatement of the loop on the host, Seq2Seq / G2P / Text2Feat against fixtures
made by the reference (tools/gen_golden_g2p.py), launch independence (free running == arg-max of the fixed-steps logits, a word alone == inside
a launch, batched sentences == single calls, padding enters only through N), the plain-text path of TTSCube, bad ids, the 10 N + 1 give-up,
and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LOGIT_TOL = 1e-4        # the project's gate for teacher-forced logits
MARGIN = 2 * LOGIT_TOL  # a transcription is compared when the reference's top-2 margin is at least this at every step the word uses
MAX_LEFT_OUT = 0.05     # ... and the words left out may be at most this share of a fixture
EOS = 2


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def _state_of(g):
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))]
    sd = M.fill_state_dict(shapes, int(g['seed']))
    sd['output.bias'][EOS] += float(g['eos_offset'])
    return sd


def _g2p_of(g, lexicon=False):
    from ttscube_amd.networks.g2p import G2P
    obj = json.loads(str(g['enc']))
    g2p = G2P()
    g2p.token2int, g2p.label2int, g2p.label_list = obj['token2int'], obj['label2int'], obj['label_list']
    g2p.initialize_network()
    g2p.seq2seq.load_state_dict(_state_of(g), strict=True)
    g2p.eval()
    g2p.to(DEV)
    if lexicon:
        g2p.load_lexicon(os.path.join(GOLDEN, 'g2p.lexicon'))
    return g2p


def _write_g2p_dir(g, base):
    """<base>.{encodings,best,lexicon}: the reference's en-* layout with the fixture's seeded weights"""
    with open(base + '.encodings', 'w') as f:
        f.write(str(g['enc']))
    torch.save(_state_of(g), base + '.best')
    with open(os.path.join(GOLDEN, 'g2p.lexicon')) as src, open(base + '.lexicon', 'w') as dst:
        dst.write(src.read())


def _status():
    from ttscube_amd import _lib
    return int(_lib.lib().ttsc_g2p_status())


# ---- the kernel against float64 -------------------------------------------------------------------------------------------------------------
def _ref_decode(net, enc, ns, feed):
    """float64 host restatement of modules.py:266-297 + 71-88 on given encoder states: feed [B, T] = the label fed back after each step (a label
    outside the table feeds back zeros: the kernel's convention for a bad teacher label)"""
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    D = net.decoder.hidden_size
    W = sd['attention.attn.conv.weight'][:, :, 0]
    b_att, v = sd['attention.attn.conv.bias'], sd['attention.v']
    emb = sd['output_emb.weight']
    B, T = feed.shape
    out = torch.zeros((B, T, sd['output.weight'].shape[0]), dtype=torch.float64)

    def cell(x, h, c, l):
        gates = sd['decoder.weight_ih_l%d' % l] @ x + sd['decoder.bias_ih_l%d' % l] + sd['decoder.weight_hh_l%d' % l] @ h + sd['decoder.bias_hh_l%d' % l]
        i, f, g, o = gates[:D], gates[D:2 * D], gates[2 * D:3 * D], gates[3 * D:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c

    for b in range(B):
        e = enc[b, :ns[b]].double()
        z = torch.zeros(D, dtype=torch.float64)
        h1, c1 = cell(torch.zeros(e.shape[1] + emb.shape[1], dtype=torch.float64), z, z, 0)
        h2, c2 = cell(h1, z, z, 1)
        last = torch.zeros(emb.shape[1], dtype=torch.float64)
        for t in range(T):
            q = c2                                                                   # decoder_hidden[-1][-1]: the CELL state of the last layer
            energy = torch.tanh(torch.cat([q[None, :].expand(e.shape[0], -1), e], dim=1) @ W.t() + b_att)
            att = torch.softmax(energy @ v, dim=0)                                    # over all positions, padding included
            ctx = att @ e
            h1, c1 = cell(torch.cat([ctx, last]), h1, c1, 0)
            h2, c2 = cell(h1, h2, c2, 1)
            out[b, t] = sd['output.weight'] @ h2 + sd['output.bias']
            f = int(feed[b, t])
            last = emb[f] if 0 <= f < emb.shape[0] else torch.zeros(emb.shape[1], dtype=torch.float64)
    return out


def _net(L, sizes=None, seed=0):
    from ttscube_amd.networks.modules import Seq2Seq
    torch.manual_seed(seed)
    net = Seq2Seq(30, L, **(sizes or {}))
    with torch.no_grad():          # livelier recurrences than the default init
        for n, p in net.named_parameters():
            if 'weight_hh' in n or 'weight_ih' in n:
                p.mul_(2.0)
    return net.eval().to(DEV)


@pytest.mark.parametrize('B,N,T,L,sizes', [
    (1, 1, 5, 42, None), (37, 11, 9, 42, None), (3, 100, 6, 42, None), (1, 11, 23, 42, None), (37, 1, 4, 42, None),
    (5, 30, 7, 7, dict(embedding_size=20, encoder_size=24, decoder_size=32)),
])
def test_decode_kernel_against_float64(B, N, T, L, sizes):
    """teacher-forced mode and fixed-steps mode; N = 100 is past the LDS-resident case; ragged n in the B = 37 cases"""
    net = _net(L, sizes)
    rng = np.random.RandomState(B * 1000 + N)
    E = net.encoder.hidden_size * 2
    enc = torch.from_numpy(rng.uniform(-1, 1, size=(B, N, E)).astype(np.float32))
    ns = [N] * B if B < 37 else [int(v) for v in rng.randint(1, N + 1, size=B)]
    n_arg = None if B < 37 else ns
    _status()
    # teacher forced
    gs = torch.from_numpy(rng.randint(0, L, size=(B, T)))
    idx, count, logits = net.decode(enc.to(DEV), n=n_arg, gs=gs)
    ref = _ref_decode(net, enc, ns, gs)
    err = float((logits.cpu().double() - ref).abs().max())
    print('g2p_decode teacher-forced B=%d N=%d T=%d L=%d: |logit| rms %.3f, max-abs error %.3e' % (B, N, T, L, float(ref.pow(2).mean().sqrt()), err))
    assert logits.shape == (B, T, L) and count.cpu().tolist() == [T] * B
    assert err <= LOGIT_TOL
    assert torch.equal(idx.cpu().long(), logits.cpu().argmax(dim=-1))
    # fixed steps, free running: the float64 loop is fed the labels the kernel chose, which must be the arg-max of the kernel's own logits and
    # the float64 arg-max wherever that one is clear
    idx, count, logits = net.decode(enc.to(DEV), n=n_arg, steps=T)
    assert torch.equal(idx.cpu().long(), logits.cpu().argmax(dim=-1)) and count.cpu().tolist() == [T] * B
    ref = _ref_decode(net, enc, ns, idx.cpu().long())
    err = float((logits.cpu().double() - ref).abs().max())
    print('g2p_decode fixed steps   B=%d N=%d T=%d L=%d: max-abs error %.3e' % (B, N, T, L, err))
    assert err <= LOGIT_TOL
    top = torch.topk(ref, 2, dim=-1).values
    sure = (top[..., 0] - top[..., 1]) > MARGIN
    assert torch.equal(idx.cpu().long()[sure], ref.argmax(dim=-1)[sure])
    assert _status() == 0


# ---- the decoder against the reference's fixtures -------------------------------------------------------------------------------------------
def test_teacher_forced_logits_match_the_reference():
    g = _golden('g2p_a')
    g2p = _g2p_of(g)
    x, y = torch.from_numpy(g['x']).to(DEV), torch.from_numpy(g['y']).to(DEV)
    got = g2p.seq2seq(x, gs_output=y).cpu()
    err = float((got - torch.from_numpy(g['logits'])).abs().max())
    print('g2p_a teacher-forced logits %s: max-abs error %.3e' % (tuple(got.shape), err))
    assert got.shape == g['logits'].shape and err <= LOGIT_TOL
    words, want = json.loads(str(g['words'])), json.loads(str(g['transcriptions']))
    sure = g['free_margins'] >= MARGIN
    assert (~sure).mean() <= MAX_LEFT_OUT
    got_tr = g2p.transcribe(words)
    assert [t for t, s in zip(got_tr, sure) if s] == [t for t, s in zip(want, sure) if s]


@pytest.mark.parametrize('name', ['s1', 's2', 'long'])
def test_free_running_matches_the_reference(name):
    g = _golden('g2p_b')
    g2p = _g2p_of(g)
    x = torch.from_numpy(g[name + '/x']).to(DEV)
    ref, counts, margins = torch.from_numpy(g[name + '/logits']), g[name + '/counts'], g[name + '/margins']
    got = g2p.seq2seq(x).cpu()
    assert got.shape == ref.shape                       # the reference's batch-wide loop length
    err = max(float((got[i, :c] - ref[i, :c]).abs().max()) for i, c in enumerate(counts))
    print('g2p_b/%s free-running logits %s, steps used %s: max-abs error %.3e' % (name, tuple(got.shape), sorted(set(counts.tolist())), err))
    assert err <= LOGIT_TOL
    words, want = json.loads(str(g[name + '/words'])), json.loads(str(g[name + '/transcriptions']))
    sure = margins >= MARGIN
    assert (~sure).mean() <= MAX_LEFT_OUT
    got_tr = g2p.transcribe(words)
    assert [t for t, s in zip(got_tr, sure) if s] == [t for t, s in zip(want, sure) if s]
    # the per-word stop ends a word where the reference's transcribe stops reading it
    idx, count = g2p.seq2seq.transcribe_ids(x)
    assert [int(c) for c, s in zip(count.cpu(), sure) if s] == [int(c) for c, s in zip(counts, sure) if s]


# ---- launch independence ----------------------------------------------------------------------------------------------------------------------
def test_free_running_is_the_argmax_of_the_fixed_steps_logits_and_words_do_not_see_each_other():
    g = _golden('g2p_b')
    g2p = _g2p_of(g)
    net = g2p.seq2seq
    x = torch.from_numpy(g['s1/x']).to(DEV)
    idx, count = net.transcribe_ids(x)
    logits = net(x)
    idx, count, am = idx.cpu().long(), count.cpu().tolist(), logits.cpu().argmax(dim=-1)
    assert idx.shape == (x.shape[0], 10 * x.shape[1] + 1) and logits.shape[1] == max(count)
    for i, c in enumerate(count):
        assert torch.equal(idx[i, :c], am[i, :c]) and not idx[i, c:].any()
        assert (c == 10 * x.shape[1] + 1 and EOS not in idx[i].tolist()) or (idx[i, c - 1] == EOS and EOS not in idx[i, :c - 1].tolist())
    # one word alone (same N): the same labels, the same logit bits on the steps both launches computed
    for i in (0, 3, x.shape[0] - 1):
        idx1, count1 = net.transcribe_ids(x[i:i + 1])
        assert int(count1[0]) == count[i] and torch.equal(idx1.cpu().long()[0], idx[i])
        solo = net(x[i:i + 1])
        T = min(solo.shape[1], logits.shape[1])
        assert torch.equal(solo[0, :T], logits[i, :T])
    # ... and in another order, next to other words
    perm = torch.arange(x.shape[0] - 1, -1, -1, device=DEV)
    idx2, count2 = net.transcribe_ids(x[perm])
    assert torch.equal(idx2.cpu().long(), idx[perm.cpu()]) and count2.cpu().tolist() == [count[i] for i in perm.cpu().tolist()]


def test_padding_enters_only_through_n():
    """a word decoded with the N of a longer sentence differs from the same word alone only through N: inside a wide launch with n = its own
    N it gives the bits of the narrow launch; with the wide N it gives the bits of the wide batch — and those two differ (the reference attends
    over the padding)"""
    g = _golden('g2p_b')
    g2p = _g2p_of(g)
    net = g2p.seq2seq
    word, N_wide = 'zorblax', 15
    N_own = len(word) + 1
    narrow = torch.from_numpy(g2p.encode_words([word])).to(DEV)
    wide = torch.from_numpy(g2p.encode_words([word, 'uncharacteristic'[:N_wide - 1]], N_wide)).to(DEV)
    T = 6
    y = torch.zeros((1, T), dtype=torch.long, device=DEV) + 5
    alone = net(narrow, gs_output=y)
    in_wide_own_n = net(wide, gs_output=y.expand(2, T).contiguous(), n=[N_own, N_wide])
    in_wide = net(wide, gs_output=y.expand(2, T).contiguous())
    alone_wide = net(wide[:1], gs_output=y)
    assert torch.equal(in_wide_own_n[0], alone[0])
    assert torch.equal(in_wide[0], alone_wide[0])
    diff = float((in_wide[0] - alone[0]).abs().max())
    print('the same word with N = %d and N = %d: logits differ by up to %.3e' % (N_own, N_wide, diff))
    assert diff > 1e-6
    # the runtime path: words of two sentences in one launch, each with its own sentence's N
    tr = g2p._decode_words([word, word], [N_own, N_wide])
    assert tr[0] == g2p._decode_words([word], [N_own])[0] and tr[1] == g2p._decode_words([word], [N_wide])[0]


def test_text2feat_batch_equals_the_single_calls():
    from ttscube_amd.io_utils.io_text import Text2Feat
    from ttscube_amd.networks import seq2seq
    t2f = Text2Feat.from_g2p(_g2p_of(_golden('g2p_c'), lexicon=True))
    texts = ['Zorblax panics - quietly.', 'Good morning!', "Don't blorf the extraordinarily uncharacteristic quux, said Bob.\nNo?", 'Qi']
    singles = [t2f(t) for t in texts]
    before = seq2seq.LAUNCHES[0]
    assert t2f.batch(texts) == singles
    assert seq2seq.LAUNCHES[0] == before + 1              # one decoder launch for all sentences
    assert t2f.batch([]) == []


# ---- front-end and API ------------------------------------------------------------------------------------------------------------------------
def test_text2feat_returns_the_reference_dict(tmp_path):
    from ttscube_amd.io_utils.io_text import Text2Feat
    from ttscube_amd.networks import seq2seq
    g = _golden('g2p_c')
    assert float(g['margins'].min()) >= MARGIN
    base = str(tmp_path / 'en-g2p')
    _write_g2p_dir(g, base)
    t2f = Text2Feat(base, device=DEV)
    assert t2f(str(g['text'])) == json.loads(str(g['result']))
    # every word a lexicon hit: no decode launch
    before = seq2seq.LAUNCHES[0]
    rez = t2f('Good morning, world - welcome!')
    assert seq2seq.LAUNCHES[0] == before and rez['phones'][:4] == [' ', 'G', 'UH', 'D']
    t2f('Good zorblax')
    assert seq2seq.LAUNCHES[0] == before + 1


def test_ttscube_takes_plain_text_through_the_g2p(tmp_path):
    from tests.test_api_gpu import _make_model_dir
    from ttscube_amd.api import TTSCube
    from ttscube_amd.io_utils.io_text import Text2Feat
    base, _, _ = _make_model_dir(tmp_path)
    pbase = os.path.join(str(tmp_path), 'phonemizer')
    _write_g2p_dir(_golden('g2p_c'), pbase)
    tts = TTSCube(base, pbase)
    assert isinstance(tts._text2feat, Text2Feat)
    other = TTSCube(base, None, text2feat=tts._text2feat)
    a, b = tts('Good morning.', speaker='s1'), other('Good morning.', speaker='s1')
    assert a.dtype == np.int16 and a.size > 0 and a.shape == b.shape and np.array_equal(a, b)
    texts = ['Good morning.', 'Zorblax panics, and the world is welcome.']
    for got, t in zip(tts.synthesize_batch(texts, speaker='s1'), texts):
        assert np.array_equal(got, tts(t, speaker='s1'))


# ---- bad inputs and limits --------------------------------------------------------------------------------------------------------------------
def test_ids_outside_their_tables_set_the_status_bit_and_raise():
    from ttscube_amd._lib import TTSCError
    from ttscube_amd.networks.seq2seq import check_status, g2p_embed
    g = _golden('g2p_a')
    net = _g2p_of(g).seq2seq
    _status()
    G = net.input_emb.weight.shape[0]
    ids = torch.tensor([[3, G, 4, -1]], device=DEV)
    out = g2p_embed(ids, net.input_emb.weight).cpu()
    tab = net.input_emb.weight.detach().cpu()
    assert torch.equal(out[0, 0], tab[3]) and torch.equal(out[0, 2], tab[4]) and float(out[0, [1, 3]].abs().max()) == 0.0
    with pytest.raises(TTSCError, match='outside the input embedding table'):
        check_status('test')
    assert _status() == 0                                   # reading cleared it
    # a teacher label outside the table feeds back zeros: every step, the one after the bad label included, equals the float64 loop with a zero
    # embedding fed back there — and that loop tells zeros from row 0 or any other row of the table by far more than the tolerance
    x = torch.from_numpy(g['x'][:2]).to(DEV)
    L, N = net.output.weight.shape[0], x.shape[1]
    gs = torch.tensor([[L, 3, 3], [4, -1, 3]], device=DEV)
    with torch.no_grad():
        enc = net.encode(x)
    bad = net.decode(enc, gs=gs, want_idx=False)[2].cpu().double()
    with pytest.raises(TTSCError, match='outside the output embedding table'):
        check_status('test')
    ref = _ref_decode(net, enc.cpu(), [N, N], gs.cpu())
    err = float((bad - ref).abs().max())
    others = min(float((_ref_decode(net, enc.cpu()[:1], [N], torch.tensor([[r, 3, 3]]))[0, 1] - ref[0, 1]).abs().max()) for r in (0, 1, L - 1))
    print('bad teacher label: max-abs error against float64 with zeros fed back %.3e; feeding back a table row instead moves step 2 by >= %.3e'
          % (err, others))
    assert others > 10 * LOGIT_TOL
    assert err <= LOGIT_TOL
    assert bool(torch.isfinite(net(x, gs_output=gs)).all())
    with pytest.raises(TTSCError, match='outside the output embedding table'):
        check_status('test')
    # one padded length per word, each inside [1, N]: refused before any launch, whatever carries them
    from ttscube_amd import _lib
    from ttscube_amd.networks import seq2seq
    before = seq2seq.LAUNCHES[0]
    for short in ([N], torch.tensor([N], dtype=torch.int32, device=DEV), _lib.DevLengths([N], device=DEV)):
        with pytest.raises(TTSCError, match='one padded length per word'):
            net.decode(enc, n=short, steps=2)
    with pytest.raises(TTSCError, match='one padded length per word'):
        net.transcribe_ids(x, n=[N])
    assert seq2seq.LAUNCHES[0] == before
    with pytest.raises(TTSCError, match='padded length'):
        net.transcribe_ids(x, n=[1, x.shape[1] + 1])
    assert _status() == 0


def test_a_run_without_eos_gives_up_after_10n_plus_1_steps():
    g = _golden('g2p_a')
    g2p = _g2p_of(g)
    with torch.no_grad():
        g2p.seq2seq.output.bias[EOS] -= 100.0              # <EOS> can never win
    words = ['ab', 'abcdef']
    x = torch.from_numpy(g2p.encode_words(words)).to(DEV)
    idx, count = g2p.seq2seq.transcribe_ids(x)
    N = x.shape[1]
    assert count.cpu().tolist() == [10 * N + 1] * 2 and EOS not in idx.cpu().tolist()[0]
    assert g2p.seq2seq(x).shape[1] == 10 * N + 1
    # each word gives up by its own N inside a mixed launch
    idx, count = g2p.seq2seq.transcribe_ids(x, n=[3, N])
    assert count.cpu().tolist() == [31, 10 * N + 1] and not idx.cpu()[0, 31:].any()
    assert all(len(t) <= 10 * N + 1 for t in g2p.transcribe(words))


# ---- command line -----------------------------------------------------------------------------------------------------------------------------
def _cli(args, timeout):
    return subprocess.run([sys.executable, '-m', 'ttscube_amd.networks.g2p'] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_command_line_modes(tmp_path):
    g = _golden('g2p_a')
    base = str(tmp_path / 'en-g2p')
    _write_g2p_dir(g, base)
    with open(os.path.join(GOLDEN, 'g2p.lexicon')) as f:
        lines = f.readlines()[:150]
    data = str(tmp_path / 'words.lexicon')
    with open(data, 'w') as f:
        f.writelines(lines)
    out = str(tmp_path / 'out.txt')
    r = _cli(['--transcribe-file', data, '--model', base, '--output-file', out, '--device', DEV], 600)      # a fresh child under its own time limit
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out) as f:
        got = [l.rstrip('\n').split('\t') for l in f]
    assert [w for w, _ in got] == [l.split('\t')[0] for l in lines]
    g2p = _g2p_of(g)
    want = g2p.transcribe([l.split('\t')[0] for l in lines[:128]]) + g2p.transcribe([l.split('\t')[0] for l in lines[128:]])
    assert [t for _, t in got] == [' '.join(t) for t in want]
    r = _cli(['--test-file', data, '--load', base, '--device', DEV], 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    acc = g2p.evaluate(type('DS', (), {'examples': [(l.split('\t')[0], l.strip().split('\t')[1].split(' ')) for l in lines]}))
    assert 'Word accuracy rate is {0:.2f}%'.format(acc * 100) in r.stdout
    r = _cli(['--train-file', data, '--dev-file', data, '--store', str(tmp_path / 'new')], 120)
    assert r.returncode != 0 and 'training is not built' in r.stderr
