"""CPU: the phonemizer's host side — collate, encodings, tokenizer + curation, state_dict layout, front-end selection of TTSCube — against
fixtures made by the reference (tools/gen_golden_phonemizer.py).  No kernel runs here."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from ttscube_amd.io_utils.io_phonemizer import PhonemizerCollate, PhonemizerDataset, PhonemizerEncodings
from ttscube_amd.io_utils.io_text import SimpleTokenizer, curate, normalize_text


def _enc():
    return PhonemizerEncodings(os.path.join(GOLDEN, 'phonemizer.encodings'))


def _dev():
    return PhonemizerDataset(os.path.join(GOLDEN, 'phonemizer_dev.json'))


def test_collate_auto_equals_the_reference():
    ds = _dev()
    g = np.load(os.path.join(GOLDEN, 'phonemizer_collate.npz'))
    b = PhonemizerCollate(_enc()).collate_fn([ds[i] for i in range(len(ds))])
    for k in ('x_char', 'x_case', 'y_phon', 'y_new_word'):
        assert b[k].dtype == torch.long and tuple(b[k].shape) == g[k].shape, k
        assert np.array_equal(b[k].numpy(), g[k]), k
    assert b['x_words'] == json.loads(str(g['x_words']))
    assert any('hybrid' in ds[i] for i in range(len(ds)))


def test_collate_aligned_has_one_target_per_character():
    ds = _dev()
    exs = [ds[i] for i in range(len(ds))]
    enc = _enc()
    b = PhonemizerCollate(enc, targets='aligned').collate_fn(exs)
    assert b['y_phon'].shape == b['x_char'].shape == b['y_new_word'].shape
    for i, e in enumerate(exs):
        want = [enc.phonemes.get(p, 0) for p in e['phones']]
        assert b['y_phon'][i, :len(want)].tolist() == want and int(b['y_phon'][i, len(want):].abs().sum()) == 0
    bad = copy.deepcopy(exs[:2])
    bad[1]['phones'] = bad[1]['phones'][:-1]
    with pytest.raises(ValueError, match='one tag per'):
        PhonemizerCollate(enc, targets='aligned').collate_fn(bad)
    with pytest.raises(ValueError):
        PhonemizerCollate(enc, targets='hybrid')


def test_encodings_compute_save_load(tmp_path):
    ds = _dev()
    e = PhonemizerEncodings()
    e.compute(ds)
    assert e.graphemes['PAD'] == 0 and e.phonemes['PAD'] == 0
    assert sorted(e.graphemes.values()) == list(range(len(e.graphemes))) and sorted(e.phonemes.values()) == list(range(len(e.phonemes)))
    assert all(g == g.lower() for g in e.graphemes if g != 'PAD')
    e.save(str(tmp_path / 'x.encodings'))
    e2 = PhonemizerEncodings(str(tmp_path / 'x.encodings'))
    assert e2.graphemes == e.graphemes and e2.phonemes == e.phonemes
    assert set(json.load(open(tmp_path / 'x.encodings'))) == {'grapheme2int', 'phon2int'}


@pytest.mark.parametrize('name', ['a', 'b', 'long'])
def test_tokenizer_and_curation_reproduce_the_reference_result(name):
    g = np.load(os.path.join(GOLDEN, 'phonemizer_%s.npz' % name))
    want = json.loads(str(g['result']))
    enc = PhonemizerEncodings()
    obj = json.loads(str(g['enc']))
    enc._grapheme2int, enc._phon2int = obj['grapheme2int'], obj['phon2int']
    names = [' '] * len(enc.phonemes)
    for p, i in enc.phonemes.items():
        names[i] = p
    text = normalize_text(str(g['text']))
    assert text == want['orig_text'] and text.startswith('§') and text.endswith('§') and '\n' not in text
    words = [w.word for w in SimpleTokenizer()(text)]
    assert ''.join(words) == text
    got = curate(text, words, [names[i] for i in g['tags'].reshape(-1).tolist()])
    assert got == want
    # the collate encodes the text as the reference did
    b = PhonemizerCollate(enc).collate_fn([{'orig_text': text, 'phones': ['1'], 'phon2word': [1], 'words': ['1']}])
    assert np.array_equal(b['x_char'].numpy(), g['x_char']) and np.array_equal(b['x_case'].numpy(), g['x_case'])


def test_state_dict_layout_and_save_load(tmp_path):
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    g = np.load(os.path.join(GOLDEN, 'phonemizer_a.npz'))
    shapes = [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))]
    net = CubenetPhonemizer(_enc())
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == shapes
    assert sum(p.numel() for p in net.parameters()) == 2155121
    net.save(str(tmp_path / 'p.model'))
    other = CubenetPhonemizer(_enc())
    other.load(str(tmp_path / 'p.model'))
    for (k, a), (_, b) in zip(net.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k


def test_no_cpu_path():
    from ttscube_amd import _lib
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    net = CubenetPhonemizer(_enc()).eval()
    X = {'x_char': torch.zeros(1, 4, dtype=torch.long), 'x_case': torch.zeros(1, 4, dtype=torch.long)}
    with pytest.raises(_lib.TTSCError):
        net(X)
    with pytest.raises(_lib.TTSCError):
        net.tag(X)


def test_ttscube_front_end_selection(tmp_path):
    """constructor logic only: no phonemizer files (or phonemizer_path=None) -> the phoneme-string reader, exactly as before"""
    from ttscube_amd.api import PhoneText2Feat, TTSCube
    assert isinstance(TTSCube._make_text2feat(None, None, 'cuda:0'), PhoneText2Feat)
    assert isinstance(TTSCube._make_text2feat(str(tmp_path / 'phonemizer'), None, 'cuda:0'), PhoneText2Feat)
    (tmp_path / 'phonemizer.encodings').write_text('{}')        # one of the two files is not enough
    assert isinstance(TTSCube._make_text2feat(str(tmp_path / 'phonemizer'), None, 'cuda:0'), PhoneText2Feat)
    mine = lambda text: {'phones': [], 'words': [], 'phon2word': []}
    assert TTSCube._make_text2feat(str(tmp_path / 'phonemizer'), mine, 'cuda:0') is mine
    rez = PhoneText2Feat()('a b | c')
    assert rez['phones'] == ['a', 'b', 'c'] and rez['phon2word'] == [0, 0, 1]


def test_validation_metrics_follow_the_reference_definitions():
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    net = CubenetPhonemizer(_enc())
    t = np.array([[1, 2, 3, 0], [4, 5, 0, 0]])
    p = np.array([[1, 9, 0, 7], [4, 5, 6, 6]])     # one real error in sentence 0; a 0 on either side never counts
    net.validation_epoch_end([{'loss': 1.0, 'target': t, 'pred': p}, {'loss': 3.0, 'target': t[1:], 'pred': t[1:]}])
    assert net._val_loss == 2.0 and net._val_pacc == 1.0 - 1 / 7 and net._val_sacc == 1.0 - 1 / 3


def test_new_symbols_are_bound():
    from ttscube_amd import _lib
    for s in ('ttsc_char_features', 'ttsc_tag_argmax', 'ttsc_masked_ce', 'ttsc_masked_ce_workspace_bytes', 'ttsc_phonemizer_status'):
        assert s in _lib.SIGNATURES
