"""CPU: the text side of the corpus importer — the TextGrid reader, `merge` against what the reference's `_merge` returned for the recorded
alignments (tools/gen_golden_import.py), the train/dev split, `fix_item` and the context lookup."""
import json
import os

import pytest

from tests.conftest import GOLDEN
from ttscube_amd.io_utils import corpus_import as CI
from ttscube_amd.io_utils.io_text import SimpleTokenizer
from ttscube_amd.io_utils.textgrid import TextGrid


def _g(name):
    return os.path.join(GOLDEN, name)


def test_long_format():
    tg = TextGrid.fromFile(_g('textgrid_long.TextGrid'))
    assert len(tg) == 3 and [t.name for t in tg] == ['words', 'phones', 'text [1]']
    assert (tg.minTime, tg.maxTime) == (0.0, 1.25)
    assert len(tg[0]) == 4 and len(tg[1]) == 7 and len(tg[2]) == 1
    assert [iv.mark for iv in tg[0]] == ['', 'she', 'said', '']                       # empty marks are intervals like any other
    assert (tg[0][2].minTime, tg[0][2].maxTime, tg[0][2].mark) == (0.55, 1.05, 'said')
    assert tg[1][2].mark == 'IY1' and tg['phones'][5].maxTime == 1.05
    assert tg[2][0].mark == 'She said "x = 3".'                                       # doubled quotes, and '= 3' inside a string is no value
    with pytest.raises(KeyError):
        tg['nothing']


def test_short_format_and_utf16():
    a = TextGrid.fromFile(_g('textgrid_short.TextGrid'))
    b = TextGrid.fromFile(_g('textgrid_short_utf16.TextGrid'))
    assert open(_g('textgrid_short_utf16.TextGrid'), 'rb').read(2) in (b'\xff\xfe', b'\xfe\xff')
    for tg in (a, b):
        assert [len(t) for t in tg] == [2, 4, 1]
        assert [iv.mark for iv in tg[0]] == ['naïve', 'café']
        assert (tg[1][3].minTime, tg[1][3].maxTime, tg[1][3].mark) == (0.65, 0.9, 'EY1')
        assert tg[2][0].mark == 'Naïve café'


def test_utf8_bom_and_comment_lines(tmp_path):
    text = open(_g('textgrid_short.TextGrid'), encoding='utf-8').read().replace('<exists>', '! a comment with "quotes" and 12\n<exists>')
    p = tmp_path / 'bom.TextGrid'
    p.write_bytes(b'\xef\xbb\xbf' + text.encode('utf-8'))
    assert [iv.mark for iv in TextGrid.fromFile(str(p))[1]] == ['N', 'IY1', 'K', 'EY1']


def test_point_tier_is_refused():
    with pytest.raises(ValueError, match='only interval tiers'):
        TextGrid.fromFile(_g('textgrid_point_tier.TextGrid'))
    with pytest.raises(ValueError, match='not a Praat TextGrid'):
        TextGrid.fromString('"ooTextFile"\n"Sound"\n0\n1\n')
    with pytest.raises(ValueError, match='the file ends'):
        TextGrid.fromString('File type = "ooTextFile"\nObject class = "TextGrid"\n0\n1\n<exists>\n1\n"IntervalTier"\n"w"\n0\n1\n1\n0\n1\n')


def test_merge_equals_every_recorded_case():
    cases = json.load(open(_g('import_textgrid_merge.json')))
    assert 6 <= len(cases) <= 10
    tok = SimpleTokenizer()
    for c in cases:
        tokens = tok(c['orig_text'])
        assert [t.word for t in tokens] == c['tokens'], c['name']
        phones, phon2word, frame2phon = CI.merge(c['words'], c['phones'], tokens)
        assert phones == c['merged_phones'], c['name']
        assert phon2word == c['phon2word'], c['name']
        assert frame2phon == c['frame2phon'], c['name']


def test_read_item_from_a_textgrid():
    item = CI.read_item(_g('textgrid_short'), 'anna')
    assert item['orig_text'] == ' Naïve café' and item['words'] == [' ', 'Naïve', ' ', 'café']
    assert item['phones'] == [' ', 'N', 'IY1', ' ', 'K', 'EY1'] and item['phon2word'] == [0, 1, 1, 2, 3, 3]
    assert len(item['frame2phon']) == 90 and item['orig_end'] == 900 and item['orig_start'] == 0
    assert item['speaker'] == 'anna' and item['orig_filename'] == 'textgrid_short'
    assert max(item['frame2phon']) < len(item['phones'])


def test_split_train_dev():
    data = list(range(10))
    train, dev = CI.split_train_dev(data, 0.5)
    assert dev == [1, 3, 5, 7, 9] and train == [0, 2, 4, 6, 8]
    train, dev = CI.split_train_dev(list(range(2500)), 0.001)
    assert dev == [999, 1999] and len(train) == 2498
    train, dev = CI.split_train_dev(data, 2)          # int(1 / 2) == 0: everything trains
    assert train == data and dev == []
    train, dev = CI.split_train_dev(data, 1.0)
    assert train == [] and dev == data
    train, dev = CI.split_train_dev([0, 1, 2], 0.34)
    assert train == [0, 2] and dev == [1]


def test_fix_item_and_context():
    errors = {}
    item = CI.fix_item({'phones': ['HH', 'AH0', 'hello', ',', ' ', 'spn', 'OW1', 'hello']}, errors)
    assert item['phones'] == ['HH', 'AH0', ' ', ',', ' ', ' ', 'OW1', ' '] and errors == {'hello': 0, 'spn': 1}
    text = 'It was   late.\nThe  rain had stopped. Nobody spoke.\n\n\n\nMorning came.\n\nShe left at noon; the others\nstayed behind.'
    items = [{'orig_text': ' the rain had stopped.', 'left_context': '', 'right_context': ''},
             {'orig_text': ' Morning came.', 'left_context': '', 'right_context': ''},
             {'orig_text': ' the others stayed', 'left_context': '', 'right_context': ''},
             {'orig_text': ' not in the book', 'left_context': '', 'right_context': ''}]
    assert CI.fetch_context(items, text) == 3
    assert (items[0]['left_context'], items[0]['right_context']) == ('It was late.', 'Nobody spoke.')
    assert (items[1]['left_context'], items[1]['right_context']) == ('', '')
    assert (items[2]['left_context'], items[2]['right_context']) == ('She left at noon;', 'behind.')
    assert (items[3]['left_context'], items[3]['right_context']) == ('', '')


def test_word_alignment_costs():
    assert CI.word_cost('Hello', 'hello') == 0 and CI.word_cost('<eps>', ',') == 0 and CI.word_cost('<eps>', 'a') == 1
    assert CI.word_cost('well-known', 'well') == 0.5 and CI.word_cost('known', 'well-known') == 0.5 and CI.word_cost('cat', 'dog') == 1
    tok = SimpleTokenizer()(' yes, no!')
    words = [{'text': ' ', 'start': 0, 'stop': 0}, {'text': 'yes', 'start': 0.0, 'stop': 0.4}, {'text': 'no', 'start': 0.5, 'stop': 0.83}]
    assert CI.align_words(words, tok) == [0, 1, 4]
