"""CPU: the host side of prosody control — the markup reader, the word -> phone mapping of the controls, and the properties of
the integer duration rule as tests/prosody_reference.py restates it (the kernel is held to that restatement exactly in test_prosody_gpu.py)."""
import re

import numpy as np
import pytest

from tests import prosody_reference as PR
from ttscube_amd.io_utils.prosody import NAMED_RATES, Prosody, parse_markup, phone_controls, word_starts


def _offset(excinfo):
    return int(re.search(r'offset (\d+)', str(excinfo.value)).group(1))


# ---- parser ---------------------------------------------------------------------------------------------------------------------------
def test_plain_text_is_one_segment_with_the_base_span():
    segs = parse_markup('a b c', Prosody(rate=2.0))
    assert len(segs) == 1 and segs[0].text == 'a b c' and segs[0].pause == 0
    assert segs[0].spans == [(0, 5, Prosody(rate=2.0))]


def test_nesting_multiplies_rates_adds_semitones_multiplies_ranges():
    text = '<prosody rate="2" pitch="+2st" range="1.5">ab <prosody rate="0.5" pitch="-3st" range="2">cd</prosody></prosody>'
    with pytest.raises(ValueError, match='per-sentence'):       # (two ranges in one sentence)
        parse_markup(text)
    text = '<prosody rate="2" pitch="+2st">ab <prosody rate="fast" pitch="-3.5st">cd</prosody> ef</prosody>'
    seg, = parse_markup(text, Prosody(rate=1.5, pitch=1.0, pitch_range=1.2))
    assert seg.text == 'ab cd ef'
    assert seg.spans == [(0, 3, Prosody(3.0, 3.0, 1.2)), (3, 5, Prosody(3.0 * 1.25, -0.5, 1.2)), (5, 8, Prosody(3.0, 3.0, 1.2))]
    seg, = parse_markup('<prosody range="1.5"><prosody range="2">x</prosody></prosody>')
    assert seg.spans == [(0, 1, Prosody(1.0, 0.0, 3.0))]


def test_named_rates():
    assert NAMED_RATES == {'x-slow': 0.5, 'slow': 0.75, 'medium': 1.0, 'fast': 1.25, 'x-fast': 1.5}
    for name, val in NAMED_RATES.items():
        seg, = parse_markup('<prosody rate="%s">a</prosody>' % name)
        assert seg.spans[0][2].rate == val
    assert Prosody(rate=8.0).dur_scale == 0.25 and Prosody(rate=0.1).dur_scale == 4.0 and Prosody(rate=2.0).dur_scale == 0.5
    assert Prosody(pitch=12.0).pitch_mul == 2.0 and Prosody(pitch=-12.0).pitch_mul == 0.5


def test_breaks_in_ms_and_s_split_segments_and_keep_the_open_span():
    segs = parse_markup('a b<break time="300ms"/><prosody rate="2">c <break time="1.5s"/> d</prosody><break time="10ms"/>')
    assert [s.text for s in segs] == ['a b', 'c ', ' d', '']
    assert [s.pause for s in segs] == [0.3, 1.5, 0.01, 0.0]
    assert [s.pause_samples() for s in segs] == [7200, 36000, 240, 0]
    assert segs[1].spans == [(0, 2, Prosody(rate=2.0))] and segs[2].spans == [(0, 2, Prosody(rate=2.0))] and segs[3].spans == []
    # two breaks in a row: the pauses add up on an empty segment
    segs = parse_markup('a<break time="1s"/><break time="2s"/>b')
    assert [s.text for s in segs] == ['a', '', 'b'] and [s.pause for s in segs] == [1.0, 2.0, 0.0]


def test_a_range_per_segment_may_differ_between_segments():
    segs = parse_markup('<prosody range="1.3">a</prosody><break time="1s"/>b')
    assert segs[0].spans[0][2].pitch_range == 1.3 and segs[1].spans[0][2].pitch_range == 1.0


@pytest.mark.parametrize('text, offset', [
    ('ab <emphasis>c</emphasis>', 3),
    ('abc </prosody>', 4),
    ('a <prosody rate="2">b', 2),
    ('a <prosody rate="quick">b</prosody>', 2),
    ('a <prosody volume="loud">b</prosody>', 2),
    ('a <prosody pitch="high">b</prosody>', 2),
    ('a <prosody pitch="2">b</prosody>', 2),
    ('a <prosody rate="120%">b</prosody>', 2),
    ('a <prosody range="-1">b</prosody>', 2),
    ('01234<break/>', 5),
    ('01234<break time="3min"/>', 5),
    ('012<break time="3s">', 3),
    ('0123456 <prosody', 8),
    ('<prosody rate="2"/>', 0),
])
def test_error_offsets(text, offset):
    with pytest.raises(ValueError) as e:
        parse_markup(text)
    assert _offset(e) == offset, str(e.value)


def test_newline_is_refused_with_its_offset():
    with pytest.raises(ValueError, match='newline') as e:
        parse_markup('ab\ncd')
    assert _offset(e) == 2


def test_conflicting_ranges_in_one_sentence_are_refused_and_the_text_says_why():
    with pytest.raises(ValueError, match='per-sentence') as e:
        parse_markup('ab <prosody range="1.2">cd</prosody>')
    assert _offset(e) == 3
    with pytest.raises(ValueError, match='per-sentence') as e:
        parse_markup('<prosody range="1.2">cd</prosody> ef')
    assert _offset(e) == 33
    # the same range twice is no conflict, and neither is white space outside the span
    parse_markup('<prosody range="1.2">ab</prosody><prosody range="1.2">cd</prosody>')
    parse_markup(' <prosody range="1.2">ab</prosody> ')


# ---- word -> phone mapping -------------------------------------------------------------------------------------------------------------
def _spans(text):
    seg, = parse_markup(text)
    return seg.text, seg.spans


def test_phone_controls_tiling_words():
    """the tokenizer words of Text2FeatBlizzard tile the normalised text '§...§' (every non-letter is a word of its own)"""
    plain, spans = _spans('the <prosody rate="2" pitch="12st">cat sat</prosody> down')
    assert plain == 'the cat sat down'
    feats = {'orig_text': '§' + plain + '§', 'words': ['§', 'the', ' ', 'cat', ' ', 'sat', ' ', 'down', '§'],
             'phones': ['D', 'V', 'k', 'a', 't', 's', 'a', 't', 'd', 'aU', 'n'], 'phon2word': [1, 1, 3, 3, 3, 5, 5, 5, 7, 7, 7]}
    assert word_starts(feats, plain) == [0, 0, 3, 4, 7, 8, 11, 12, 15]
    c = phone_controls(feats, plain, spans)
    assert c['dur_scale'].tolist() == [1, 1, .5, .5, .5, .5, .5, .5, 1, 1, 1]
    assert c['pitch_mul'].tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1] and c['pitch_mul'].dtype == np.float32
    assert c['pitch_range'] == 1.0


def test_phone_controls_bar_separated_words():
    """PhoneText2Feat: '|' separates words, a word is its stripped phone string"""
    from ttscube_amd.api import PhoneText2Feat
    plain, spans = _spans('<prosody range="1.5">a b | <prosody rate="0.5">c d | e</prosody> | a b</prosody>')
    assert plain == 'a b | c d | e | a b'
    feats = PhoneText2Feat()(plain)
    assert feats['words'] == ['a b', 'c d', 'e', 'a b']
    assert word_starts(feats, plain) == [0, 6, 12, 16]           # (the second 'a b' is found behind the first: forward search)
    c = phone_controls(feats, plain, spans)
    assert c['dur_scale'].tolist() == [1, 1, 2, 2, 2, 1, 1] and c['pitch_range'] == 1.5


def test_phone_controls_empty_word_inherits_its_predecessor():
    """the G2P front-end keeps '' words; a word whose first character lies in a span takes that span even when it ends outside"""
    plain, spans = _spans('ab <prosody pitch="-12st">cd</prosody> ef')
    feats = {'orig_text': ' ' + plain + ' ', 'words': ['ab', 'cd', '', 'ef'], 'phones': ['a', 'b', 'c', 'd', 'x', 'e'], 'phon2word': [0, 0, 1, 1, 2, 3]}
    assert word_starts(feats, plain) == [0, 3, 3, 6]
    assert phone_controls(feats, plain, spans)['pitch_mul'].tolist() == [1, 1, .5, .5, .5, 1]
    feats = {'orig_text': plain, 'words': ['', 'ab'], 'phones': ['q', 'a'], 'phon2word': [0, 1]}       # (an empty FIRST word: offset 0)
    assert word_starts(feats, plain) == [0, 0]
    feats = {'orig_text': ' Ab Cd ', 'words': ['ab', 'cd'], 'phones': ['a', 'c'], 'phon2word': [0, 1]}     # (words with their case folded are still found)
    assert word_starts(feats, 'Ab Cd') == [0, 3]


# ---- the duration rule ------------------------------------------------------------------------------------------------------------------
def _rows(seed, count=300):
    rng = np.random.RandomState(seed)
    for _ in range(count):
        n = int(rng.randint(1, 120))
        D = int(rng.choice([8, 101]))
        d = rng.randint(0, D, size=n)
        d[rng.rand(n) < 0.2] = 0
        kind = rng.randint(3)
        s = np.full(n, rng.choice([0.25, 4.0, rng.uniform(0.25, 4)])) if kind == 0 else np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=n))
        yield d, PR.q16(s), rng


def test_rule_identity():
    for d, _, _ in _rows(1):
        nd, emitted, floors, caps = PR.durations_row(d, np.full(len(d), 65536))
        assert np.array_equal(nd, d) and emitted == d.sum() and floors == 0 and caps == 0
        nd2, _, _, _ = PR.durations_row(d)
        assert np.array_equal(nd2, d)


def test_rule_total_follows_the_tempo_and_no_phone_vanishes_or_appears():
    worst = 0.0
    for d, q, _ in _rows(2):
        nd, emitted, floors, caps = PR.durations_row(d, q)
        assert caps == 0 and emitted == nd.sum()
        want = float((d.astype(np.int64) * q.astype(np.int64)).sum()) / 65536.0        # (exact: integers below 2**53)
        assert abs(emitted - want) <= 0.5 + floors, (emitted, want, floors)
        worst = max(worst, abs(emitted - want) - floors)
        assert (nd[d > 0] >= 1).all() and (nd[d == 0] == 0).all()
        # the default cap, ceil((D - 1) * max scale), never engages: a phone gets at most ceil(d * s)
        assert (nd <= -(-d.astype(np.int64) * q.astype(np.int64) // 65536)).all()
    assert worst <= 0.5


def test_rule_dur_set_is_obeyed_and_resynchronises_the_carry():
    for d, q, rng in _rows(3, 200):
        n = len(d)
        ds = np.full(n, -1)
        pick = rng.rand(n) < 0.25
        ds[pick] = rng.randint(0, 30, size=int(pick.sum()))
        if n > 2:
            ds[n // 2] = 0                                     # (a pinned zero: the phone is dropped even when d > 0)
        nd, emitted, floors, caps = PR.durations_row(d, q, ds)
        assert np.array_equal(nd[ds >= 0], ds[ds >= 0]) and emitted == nd.sum()
        # behind a pinned phone the carry starts afresh: the tail equals the rule run on the tail alone
        last = int(np.max(np.nonzero(ds >= 0)[0])) if (ds >= 0).any() else -1
        tail, _, _, _ = PR.durations_row(d[last + 1:], q[last + 1:])
        assert np.array_equal(nd[last + 1:], tail)
    nd, emitted, _, caps = PR.durations_row([3, 5, 2], [4 * 65536] * 3, [-1, 100, -1], dcap=10)
    assert nd.tolist() == [10, 10, 8] and emitted == 28 and caps == 1


def test_restated_mean_is_within_rounding_of_a_sequential_sum():
    rng = np.random.RandomState(4)
    p0 = (rng.rand(333) * 280).astype(np.float32)
    voiced = rng.rand(333) < 0.6
    m = PR.voiced_mean(p0, voiced)
    seq = np.float64(0)
    for v in p0[voiced]:
        seq += np.float64(v)
    assert abs(float(m) - float(seq / voiced.sum())) <= float(np.spacing(np.float32(m)))
    assert PR.voiced_mean(p0, np.zeros(333, bool)) is None
    # range 1 skips the mean altogether (m + 1 * (p0 - m) is not p0 in float32), multiplier 1 is exact
    op = np.stack([rng.rand(50), rng.rand(50)], 1).astype(np.float32)
    want = ((op[:, 0] * np.float32(280)).astype(np.float32) * np.rint(op[:, 1]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(PR.pitch_row(op, 50, 280, np.ones(50, np.float32), 1.0), want)
