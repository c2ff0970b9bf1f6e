"""Prosody controls on the host (not in the reference): what a caller may ask for (`Prosody`), a small markup that asks for it per
stretch of text (`parse_markup`), and the mapping of those stretches onto the phones of a front-end's output (`phone_controls`).  Nothing here
touches the device: the per-phone arrays made here travel in the batch dict (`x_dur_scale`, `x_pitch_mul`, `x_pitch_range`) to the two
controlled launches of csrc/prosody.hip.

The markup is a small subset in the style of SSML, and nothing else that looks like a tag is let through:

    <prosody rate="1.25" pitch="+2st" range="1.2"> ... </prosody>     any subset of the three attributes; may be nested
    <break time="300ms"/>                                             time in ms or s

  * rate: a positive number (1 = unchanged, 2 = twice as fast) or one of the names
        x-slow = 0.5, slow = 0.75, medium = 1.0, fast = 1.25, x-fast = 1.5
  * pitch: semitones, "+2st" / "-1.5st" / "2st"
  * range: a positive factor on the spread of the pitch around the sentence's own voiced mean (1 = unchanged)
  * nesting multiplies rates, adds semitones and multiplies ranges
  * range is a per-sentence quantity: the stretches of one sentence (one segment between breaks) must all end up with the same range
  * a break splits the sentence into segments; each segment is synthesised as a sentence of its own, and round(time * 24000) zero samples are
    put between them (api.py)
  * markup text may not contain a newline (the front-ends rewrite newlines, which would shift every offset behind them)."""
import re

import numpy as np

DUR_SCALE_MIN, DUR_SCALE_MAX = 0.25, 4.0
NAMED_RATES = {'x-slow': 0.5, 'slow': 0.75, 'medium': 1.0, 'fast': 1.25, 'x-fast': 1.5}
SAMPLE_RATE = 24000


class Prosody:
    """rate: > 1 is faster (duration scale = 1 / rate, limited to [0.25, 4]); pitch: semitones (multiplier 2 ** (pitch / 12)); pitch_range: factor
    on the spread of the pitch around the sentence's voiced mean."""
    __slots__ = ('rate', 'pitch', 'pitch_range')

    def __init__(self, rate=1.0, pitch=0.0, pitch_range=1.0):
        rate, pitch, pitch_range = float(rate), float(pitch), float(pitch_range)
        if not (np.isfinite(rate) and rate > 0):
            raise ValueError('Prosody: rate must be a positive number, got %r' % (rate,))
        if not np.isfinite(pitch):
            raise ValueError('Prosody: pitch must be a finite number of semitones, got %r' % (pitch,))
        if not (np.isfinite(pitch_range) and pitch_range > 0):
            raise ValueError('Prosody: pitch_range must be a positive number, got %r' % (pitch_range,))
        self.rate, self.pitch, self.pitch_range = rate, pitch, pitch_range

    @property
    def dur_scale(self):
        return min(max(1.0 / self.rate, DUR_SCALE_MIN), DUR_SCALE_MAX)

    @property
    def pitch_mul(self):
        return float(2.0 ** (self.pitch / 12.0))

    def is_identity(self):
        return self.rate == 1.0 and self.pitch == 0.0 and self.pitch_range == 1.0

    def has_pitch(self):
        return self.pitch != 0.0 or self.pitch_range != 1.0

    def inside(self, outer):
        """this span nested in `outer`: rates multiply, semitones add, ranges multiply"""
        return Prosody(outer.rate * self.rate, outer.pitch + self.pitch, outer.pitch_range * self.pitch_range)

    def __eq__(self, other):
        return isinstance(other, Prosody) and (self.rate, self.pitch, self.pitch_range) == (other.rate, other.pitch, other.pitch_range)

    def __repr__(self):
        return 'Prosody(rate=%g, pitch=%g, pitch_range=%g)' % (self.rate, self.pitch, self.pitch_range)


class Segment:
    """one stretch between breaks: `text` (tag-free), `spans` [(start, end, Prosody)] tiling it in order, `pause` seconds of silence behind it"""
    __slots__ = ('text', 'spans', 'pause')

    def __init__(self, text='', spans=None, pause=0.0):
        self.text, self.spans, self.pause = text, list(spans or []), float(pause)

    def pause_samples(self, sample_rate=SAMPLE_RATE):
        return int(round(self.pause * sample_rate))

    def __repr__(self):
        return 'Segment(%r, %r, pause=%g)' % (self.text, self.spans, self.pause)


_ATTR = re.compile(r'\s*([A-Za-z_][\w-]*)\s*=\s*"([^"]*)"')
_NUM = r'[+-]?(?:\d+\.?\d*|\.\d+)'


def _parse_rate(v, off):
    v = v.strip()
    if v in NAMED_RATES:
        return NAMED_RATES[v]
    m = re.fullmatch(_NUM, v)
    if not m or float(v) <= 0:
        raise ValueError('markup, offset %d: rate="%s" is neither a positive number nor one of %s' % (off, v, '|'.join(NAMED_RATES)))
    return float(v)


def _parse_pitch(v, off):
    m = re.fullmatch(r'(%s)\s*st' % _NUM, v.strip())
    if not m:
        raise ValueError('markup, offset %d: pitch="%s" is not a number of semitones such as "+2st"' % (off, v))
    return float(m.group(1))


def _parse_range(v, off):
    m = re.fullmatch(_NUM, v.strip())
    if not m or float(v) <= 0:
        raise ValueError('markup, offset %d: range="%s" is not a positive factor' % (off, v))
    return float(v)


def _parse_time(v, off):
    m = re.fullmatch(r'(%s)\s*(ms|s)' % _NUM, v.strip())
    if not m or float(m.group(1)) < 0:
        raise ValueError('markup, offset %d: time="%s" is not a non-negative time in ms or s' % (off, v))
    return float(m.group(1)) / (1000.0 if m.group(2) == 'ms' else 1.0)


def _attributes(body, off, allowed, tag):
    out, pos = {}, 0
    while pos < len(body):
        m = _ATTR.match(body, pos)
        if not m:
            if body[pos:].strip() == '':
                break
            raise ValueError('markup, offset %d: cannot read the attributes of <%s>: %r' % (off, tag, body[pos:].strip()))
        if m.group(1) not in allowed or m.group(1) in out:
            raise ValueError('markup, offset %d: <%s> takes %s once each, not %r' % (off, tag, ', '.join(allowed), m.group(1)))
        out[m.group(1)] = m.group(2)
        pos = m.end()
    return out


def parse_markup(text, base=None):
    """markup text -> list of Segment (at least one).  `base`: the Prosody around the whole text (the call-level arguments: the outermost span).
    Raises ValueError, with the character offset in the message, for anything else that looks like a tag, for a tag that is not closed or not
    open, for a newline, and for a segment whose spans end up with two different ranges."""
    base = base if base is not None else Prosody()
    nl = text.find('\n')
    if nl >= 0:
        raise ValueError('markup, offset %d: markup text may not contain a newline' % nl)
    stack = [(base, -1)]                 # (composed Prosody, offset of the tag that opened it)
    segs = [Segment()]
    range_of = {}                        # segment index -> (range, offset of the tag in force when it was first used)

    def emit(chunk, at):
        if not chunk:
            return
        seg, (pros, off) = segs[-1], stack[-1]
        if chunk.strip():
            first = range_of.setdefault(len(segs) - 1, (pros.pitch_range, off))
            if first[0] != pros.pitch_range:
                raise ValueError('markup, offset %d: range is a per-sentence quantity — this stretch asks for range %g, an earlier stretch of the same '
                                 'sentence (between two breaks) for %g; give one range per sentence' % (off if off >= 0 else at, pros.pitch_range, first[0]))
        start = len(seg.text)
        seg.text += chunk
        if seg.spans and seg.spans[-1][2] == pros:
            seg.spans[-1] = (seg.spans[-1][0], start + len(chunk), pros)
        else:
            seg.spans.append((start, start + len(chunk), pros))

    pos = 0
    while pos < len(text):
        lt = text.find('<', pos)
        if lt < 0:
            emit(text[pos:], pos)
            break
        emit(text[pos:lt], pos)
        gt = text.find('>', lt)
        if gt < 0:
            raise ValueError('markup, offset %d: "<" without a closing ">"' % lt)
        tag = text[lt + 1:gt]
        m = re.fullmatch(r'\s*prosody\b(.*)', tag, flags=re.S)
        if m and not tag.rstrip().endswith('/'):
            at = _attributes(m.group(1), lt, ('rate', 'pitch', 'range'), 'prosody')
            inner = Prosody(_parse_rate(at['rate'], lt) if 'rate' in at else 1.0, _parse_pitch(at['pitch'], lt) if 'pitch' in at else 0.0,
                            _parse_range(at['range'], lt) if 'range' in at else 1.0)
            stack.append((inner.inside(stack[-1][0]), lt))
        elif re.fullmatch(r'\s*/\s*prosody\s*', tag):
            if len(stack) == 1:
                raise ValueError('markup, offset %d: </prosody> without an open <prosody>' % lt)
            stack.pop()
        else:
            m = re.fullmatch(r'\s*break\b(.*)/\s*', tag, flags=re.S)
            if not m:
                raise ValueError('markup, offset %d: unsupported tag <%s> (only <prosody rate= pitch= range=>, </prosody> and <break time=/>)' % (lt, tag))
            at = _attributes(m.group(1), lt, ('time',), 'break')
            if 'time' not in at:
                raise ValueError('markup, offset %d: <break/> needs time="..ms" or time="..s"' % lt)
            segs[-1].pause += _parse_time(at['time'], lt)
            segs.append(Segment())
        pos = gt + 1
    if len(stack) > 1:
        raise ValueError('markup, offset %d: <prosody> is never closed' % stack[-1][1])
    # a break directly behind a break (or at the very start) leaves an empty segment: its pause is kept, it takes no batch row
    return segs


def markup_has_pitch(segments):
    """does any span of these segments ask for a pitch or a range (what a model without a pitch input has to refuse)"""
    return any(p.has_pitch() for s in segments for _, _, p in s.spans)


def word_starts(feats, plain_text):
    """character offset, in `plain_text`, of each entry of feats['words'].  Each word is searched in feats['orig_text'] forward from the end of the
    previous one (tiling tokenizer words and PhoneText2Feat's '|'-separated words alike); an empty word, or one the front-end rewrote beyond
    recognition, inherits its predecessor's offset.  The front-ends wrap the text (a leading '§' or blank): offsets are shifted back by the place
    of `plain_text` inside `orig_text`."""
    orig = feats.get('orig_text', plain_text)
    shift = orig.find(plain_text) if plain_text else 0
    if shift < 0:
        shift = 0
    starts, cur, last = [], 0, 0
    folded = orig.lower()
    for w in feats['words']:
        at = orig.find(w, cur) if w else -1
        if w and at < 0 and len(folded) == len(orig):        # (a front-end that folds the case of its words)
            at = folded.find(w.lower(), cur)
        if at >= 0:
            last, cur = at, at + len(w)
        starts.append(min(max(last - shift, 0), max(len(plain_text) - 1, 0)))
    return starts


def phone_controls(feats, plain_text, spans):
    """-> {'dur_scale': float64 [n_phones], 'pitch_mul': float32 [n_phones], 'pitch_range': float}.  A word takes the controls of the span that
    holds its first character, a phone those of word phon2word[i]; the row's range is the (single) range of the spans that hold a word."""
    starts = word_starts(feats, plain_text)

    def span_of(c):
        for s, e, p in spans:
            if s <= c < e:
                return p
        return spans[-1][2] if spans else Prosody()

    per_word = [span_of(c) for c in starts]
    p2w = list(feats['phon2word'])
    n = len(feats['phones'])
    ds, pm = np.ones(n, np.float64), np.ones(n, np.float32)
    for i in range(n):
        p = per_word[p2w[i]] if 0 <= p2w[i] < len(per_word) else (spans[0][2] if spans else Prosody())
        ds[i], pm[i] = p.dur_scale, np.float32(p.pitch_mul)
    ranges = sorted({per_word[p2w[i]].pitch_range for i in range(n) if 0 <= p2w[i] < len(per_word)})
    if len(ranges) > 1:
        raise ValueError('prosody: range is a per-sentence quantity, the words of %r ask for %s' % (plain_text, ranges))
    rng = ranges[0] if ranges else (spans[0][2].pitch_range if spans else 1.0)
    return {'dur_scale': ds, 'pitch_mul': pm, 'pitch_range': float(rng)}
