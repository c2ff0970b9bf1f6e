"""CPU: the word-level G2P front-end without its decoder — the id matrix of `transcribe`, the lexicon, the assembly of G2P.__call__ / Text2Feat
around a stubbed decoder (against the dict the reference's Text2Feat returned, tools/gen_golden_g2p.py), front-end selection, the C-ABI table,
the batches of `evaluate`, and the errors of the paths that are not built (host tensors, training)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from tests.conftest import GOLDEN


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def _g2p_of(g, lexicon=False):
    from ttscube_amd.networks.g2p import G2P
    obj = json.loads(str(g['enc']))
    g2p = G2P()
    g2p.token2int, g2p.label2int, g2p.label_list = obj['token2int'], obj['label2int'], obj['label_list']
    if lexicon:
        g2p.load_lexicon(os.path.join(GOLDEN, 'g2p.lexicon'))
    return g2p


def test_transcribe_builds_the_reference_id_matrix():
    g = _golden('g2p_a')
    g2p = _g2p_of(g)
    words = json.loads(str(g['words']))
    x = g2p.encode_words(words)
    assert x.dtype == np.int64 and np.array_equal(x, g['x'])
    assert x.shape[1] == max(len(w) for w in words) + 1
    for i, w in enumerate(words):
        assert x[i, len(w)] == 2 and not x[i, len(w) + 1:].any()
    # an unknown character is <UNK>; a wider N only adds <PAD>
    y = g2p.encode_words(['a#b'], N=6)
    assert y[0, 1] == 1 and y[0, 3] == 2 and y[0, 4:].tolist() == [0, 0]


def test_seq2seq_has_the_reference_state_dict():
    from ttscube_amd.networks.modules import Seq2Seq
    g = _golden('g2p_a')
    g2p = _g2p_of(g)
    g2p.initialize_network()
    assert isinstance(g2p.seq2seq, Seq2Seq)
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))]
    assert M.named_shapes(g2p.seq2seq) == shapes
    g2p.seq2seq.load_state_dict(M.fill_state_dict(shapes, int(g['seed'])), strict=True)
    for k in ('input_emb.weight', 'output_emb.weight', 'encoder.weight_ih_l1_reverse', 'decoder.weight_ih_l0', 'attention.attn.conv.weight',
              'attention.v', 'output.bias'):
        assert k in dict(shapes)


def test_lexicon_fixture_loads_and_malformed_lines_are_skipped(tmp_path):
    from ttscube_amd.networks.g2p import G2P, G2PDataset
    path = os.path.join(GOLDEN, 'g2p.lexicon')
    with open(path) as f:
        lines = f.readlines()
    assert 1000 < len(lines) <= 2000 and os.path.getsize(path) <= 1 << 20
    g2p = G2P()
    g2p.load_lexicon(path)
    assert g2p.lookup['good'] == ['G', 'UH', 'D'] and all(k == k.lower() for k in g2p.lookup)
    assert len(g2p.lookup) == len({l.split('\t')[0].lower() for l in lines})
    ds = G2PDataset(path)
    assert len(ds.examples) == len(lines) and ds.examples[0] == (lines[0].split('\t')[0], lines[0].strip().split('\t')[1].split(' '))
    bad = tmp_path / 'bad.lexicon'
    bad.write_text('ONE\tW AH N\nno tab here\nTWO\tT UW\textra\n\nThree\tTH R IY\n')
    g2 = G2P()
    g2.load_lexicon(str(bad))
    assert g2.lookup == {'one': ['W', 'AH', 'N'], 'three': ['TH', 'R', 'IY']}
    assert G2PDataset(str(bad)).examples == [('ONE', ['W', 'AH', 'N']), ('Three', ['TH', 'R', 'IY'])]


def test_encodings_follow_the_reference_rules(tmp_path):
    """update_encodings + save on the lexicon fixture give the committed encodings (made by the reference), and load reads them back"""
    from ttscube_amd.networks.g2p import G2P, G2PDataset
    g2p = G2P()
    g2p.update_encodings(G2PDataset(os.path.join(GOLDEN, 'g2p.lexicon')))
    g2p.save(str(tmp_path / 'g2p'))
    with open(os.path.join(GOLDEN, 'g2p.encodings')) as f:
        want = f.read()
    assert (tmp_path / 'g2p.encodings').read_text() == want
    assert json.loads(want) == json.loads(str(_golden('g2p_a')['enc']))


def _stubbed(g, calls):
    g2p = _g2p_of(g, lexicon=True)
    ref = dict(zip(json.loads(str(g['words'])), json.loads(str(g['transcriptions']))))

    def decode(words, ns):
        calls.append((list(words), list(ns)))
        return [ref[w] for w in words]

    g2p._decode_words = decode
    return g2p


def test_front_end_assembly_matches_the_reference_dict():
    from ttscube_amd.io_utils.io_text import Text2Feat
    g = _golden('g2p_c')
    calls = []
    g2p = _stubbed(g, calls)
    t2f = Text2Feat.from_g2p(g2p)
    want = json.loads(str(g['result']))
    got = t2f(str(g['text']))
    assert got == want
    assert '' in got['phones'] and '_' not in got['phones'] and got['orig_text'].startswith(' ') and '\n' not in got['orig_text']
    # the decoder saw only the words the lexicon does not hold, each with the N of the whole sentence (lexicon hits count towards it)
    words = json.loads(str(g['words']))
    N = max(len(w) for w in words) + 1
    assert len(calls) == 1
    assert calls[0][0] == [w for w in words if w not in g2p.lookup] and 0 < len(calls[0][0]) < len(words)
    assert calls[0][1] == [N] * len(calls[0][0])
    # the token objects carry the transcriptions: ' ' -> [' '], '-' and '"' -> ['_'], other punctuation -> ['']
    tokens = g2p(want['orig_text'])
    by_word = {t.word: t.transcription for t in tokens}
    assert by_word[' '] == [' '] and by_word['-'] == ['_'] and by_word['"'] == ['_'] and by_word[','] == [''] and by_word['!'] == ['']
    assert by_word['Good'] == g2p.lookup['good']
    # batch: one decoder call for all sentences, every word with its own sentence's N; results equal the single calls
    calls.clear()
    short = 'Zorblax panic'
    both = t2f.batch([str(g['text']), short])
    assert len(calls) == 1 and both[0] == want and both[1] == t2f(short)
    assert ('zorblax', N) in zip(*calls[0]) and ('zorblax', len('zorblax') + 1) in zip(*calls[0])


def test_a_text_of_lexicon_hits_never_reaches_the_decoder():
    from ttscube_amd.io_utils.io_text import Text2Feat
    calls = []
    t2f = Text2Feat.from_g2p(_stubbed(_golden('g2p_c'), calls))
    rez = t2f('Good morning, world - welcome!')
    assert calls == [] and rez['phones'][:4] == [' ', 'G', 'UH', 'D'] and rez['words'][1] == 'Good'
    assert t2f('... !')['phones'] == [' ', '', '', '', ' ', '', ' '] and calls == []


def test_front_end_selection(tmp_path):
    from ttscube_amd import api
    from ttscube_amd.api import PhoneText2Feat, TTSCube
    from ttscube_amd.io_utils import io_text
    base = str(tmp_path / 'phonemizer')
    made = []

    class Fake:
        def __init__(self, path, device='cuda:0'):
            made.append((path, device))

    real = io_text.Text2Feat
    io_text.Text2Feat = Fake
    try:
        with open(os.path.join(GOLDEN, 'g2p.encodings')) as f:
            (tmp_path / 'phonemizer.encodings').write_text(f.read())
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), PhoneText2Feat)      # no model, no lexicon
        (tmp_path / 'phonemizer.best').write_bytes(b'')
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), PhoneText2Feat)      # a missing .lexicon
        (tmp_path / 'phonemizer.lexicon').write_text('A\tAH\n')
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), Fake) and made == [(base, 'cuda:0')]
        os.remove(base + '.best')
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), PhoneText2Feat)      # a missing model
        (tmp_path / 'phonemizer.model').write_bytes(b'')
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:1'), Fake) and made[-1] == (base, 'cuda:1')
        mine = lambda text: {'phones': [], 'words': [], 'phon2word': []}
        assert TTSCube._make_text2feat(base, mine, 'cuda:0') is mine and len(made) == 2       # a caller's text2feat wins
        (tmp_path / 'phonemizer.encodings').write_text('{}')                                    # not a G2P's encodings
        os.remove(base + '.model')
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), PhoneText2Feat) and len(made) == 2
    finally:
        io_text.Text2Feat = real
    assert api.TTSCube._is_g2p(str(tmp_path / 'nothing')) is False


def test_g2p_encodings_never_reach_the_sentence_tagger(tmp_path):
    """a G2P's .encodings next to a .model but no .lexicon: the files pass the tagger's existence check, yet they are not the tagger's"""
    from ttscube_amd.api import PhoneText2Feat, TTSCube
    from ttscube_amd.io_utils import io_text
    base = str(tmp_path / 'phonemizer')
    with open(os.path.join(GOLDEN, 'g2p.encodings')) as f:
        (tmp_path / 'phonemizer.encodings').write_text(f.read())
    (tmp_path / 'phonemizer.model').write_bytes(b'')
    made = []

    class Fake:
        def __init__(self, path, device='cuda:0'):
            made.append(path)

    real = io_text.Text2FeatBlizzard, io_text.Text2Feat
    io_text.Text2FeatBlizzard = io_text.Text2Feat = Fake
    try:
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), PhoneText2Feat) and made == []
        assert TTSCube._g2p_files(base) == 'incomplete' and TTSCube._is_g2p(base) is False
        (tmp_path / 'phonemizer.encodings').write_text('{"grapheme2int": {}}')               # the tagger's own files still reach it
        assert isinstance(TTSCube._make_text2feat(base, None, 'cuda:0'), Fake) and made == [base]
        assert TTSCube._g2p_files(base) is None
    finally:
        io_text.Text2FeatBlizzard, io_text.Text2Feat = real


def test_new_symbols_are_bound():
    from ttscube_amd import _lib
    for s in ('ttsc_g2p_decode', 'ttsc_g2p_embed', 'ttsc_g2p_status'):
        assert s in _lib.SIGNATURES
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'ttscube_hip.h')) as f:
        header = f.read()
    fields = header.split('typedef struct ttsc_g2p_args {')[1].split('}')[0]
    names = re.findall(r'(\w+)\s*[;,]', re.sub(r'/\*.*?\*/', '', fields, flags=re.S))
    assert names == [n for n, _ in _lib.G2pArgs._fields_]


def test_host_tensors_and_training_raise():
    from ttscube_amd._lib import TTSCError
    from ttscube_amd.networks.g2p import main
    from ttscube_amd.networks.seq2seq import Seq2Seq, g2p_embed
    net = Seq2Seq(30, 42)
    x = torch.zeros((2, 5), dtype=torch.long)
    net.eval()
    with pytest.raises(TTSCError, match='CPU'):
        net(x)
    with pytest.raises(TTSCError, match='CPU'):
        net.transcribe_ids(x)
    with pytest.raises(TTSCError, match='no CPU path'):
        g2p_embed(x, net.input_emb.weight)
    with pytest.raises(TTSCError, match='no CPU path'):
        net.decode(torch.zeros((2, 5, 400)))
    net.train()
    with pytest.raises(TTSCError, match='training is not built'):
        net(x, gs_output=x)
    assert main(['g2p', '--train-file', 'a', '--dev-file', 'b', '--store', 'c']) != 0      # the reference's third mode


def test_evaluate_walks_every_example_in_batches_of_64():
    g2p = _g2p_of(_golden('g2p_a'))
    sizes = []

    class DS:
        examples = []

    def transcribe(words):
        sizes.append(len(words))
        return [['AH'] if w.startswith('x') else ['B'] for w in words]

    g2p.transcribe = transcribe
    for n, want in ((130, [64, 64, 2]), (64, [64]), (5, [5]), (128, [64, 64])):
        sizes.clear()
        DS.examples = [('x%d' % i if i % 2 else 'y%d' % i, ['AH']) for i in range(n)]
        acc = g2p.evaluate(DS)
        assert sizes == want and acc == 1.0 - ((n + 1) // 2) / n
