"""Seeded synthetic "speech" with known boundaries for the forced aligner's tests: eight phones with distinct stationary spectra (five harmonic
tones under different formant envelopes, three band-limited noises), 60 - 200 ms each, words of two to four phones from a small lexicon, silences
(a faint noise floor) of 80 - 250 ms at both ends and between some words but not others.  No import from ttscube_amd."""
import numpy as np

SAMPLE_RATE, HOP = 24000, 240
# (f0 Hz, formant centres Hz) of the voiced phones; (low, high) Hz of the noise bands
VOICED = {'AA': (120.0, (700.0, 1200.0)), 'IY': (150.0, (300.0, 2300.0)), 'UW': (110.0, (350.0, 800.0)), 'EH': (170.0, (550.0, 1800.0)),
          'OW': (135.0, (450.0, 3000.0))}
NOISE = {'S': (5000.0, 9000.0), 'SH': (2200.0, 4500.0), 'F': (800.0, 11000.0)}
PHONES = list(VOICED) + list(NOISE)
LEXICON = {'ASA': ['AA', 'S', 'AA'], 'ISHU': ['IY', 'SH', 'UW'], 'EFO': ['EH', 'F', 'OW'], 'SOSI': ['S', 'OW', 'S', 'IY'], 'UFA': ['UW', 'F', 'AA'],
           'SHE': ['SH', 'EH'], 'OSU': ['OW', 'S', 'UW'], 'IFE': ['IY', 'F', 'EH'], 'AU': ['AA', 'UW'], 'FISH': ['F', 'IY', 'SH']}
N_UTT = 8


def _phone(sym, n, rng):
    t = np.arange(n) / SAMPLE_RATE
    if sym in VOICED:
        f0, formants = VOICED[sym]
        f0 = f0 * rng.uniform(0.9, 1.1)                           # every instance differs a little in pitch, formants and level
        formants = [c * rng.uniform(0.93, 1.07) for c in formants]
        x = np.zeros(n)
        for h in range(1, int(10000.0 / f0)):
            f = h * f0
            amp = sum(np.exp(-0.5 * ((f - c) / 180.0) ** 2) for c in formants) + 0.02
            x += amp * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2.0 * np.pi))
        return 0.25 * rng.uniform(0.7, 1.4) * x / np.sqrt(np.mean(x * x))
    lo, hi = NOISE[sym]
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / SAMPLE_RATE)
    spec[(f < lo) | (f > hi)] = 0
    x = np.fft.irfft(spec, n)
    return 0.12 * rng.uniform(0.7, 1.4) * x / np.sqrt(np.mean(x * x))


def lexicon_text():
    """the lexicon in the format of tests/golden/g2p.lexicon"""
    return ''.join('%s\t%s\n' % (w, ' '.join(p)) for w, p in LEXICON.items())


def corpus(seed=1234, n=N_UTT):
    """-> list of dicts: audio float32 [L], text (the words and a full stop), words (the word tokens, lower case), units [(phone symbol or '' for silence, word index or -1,
    start sample, end sample)] — the truth, silences that are absent left out"""
    rng = np.random.default_rng(seed)
    names = list(LEXICON)
    out = []
    ms = SAMPLE_RATE // 1000
    for u in range(n):
        words = [names[i] for i in rng.choice(len(names), size=3, replace=False)]
        pause = [True] + [bool(rng.integers(0, 2)) for _ in words[1:]] + [True]      # before word k; the ends always pause
        if u == 0:
            pause[1:-1] = [True, False]                           # (both kinds of inner gap occur whatever the seed)
        parts, units, pos = [], [], 0

        def add(sym, w, x):
            nonlocal pos
            parts.append(x)
            units.append((sym, w, pos, pos + len(x)))
            pos += len(x)

        for w, name in enumerate(words):
            if pause[w]:
                add('', -1, 0.002 * rng.standard_normal(int(rng.integers(80, 251)) * ms))
            for sym in LEXICON[name]:
                add(sym, w, _phone(sym, int(rng.integers(60, 201)) * ms, rng))
        add('', -1, 0.002 * rng.standard_normal(int(rng.integers(80, 251)) * ms))
        audio = np.concatenate(parts) + 0.0005 * rng.standard_normal(pos)
        text = ' '.join(w.lower() for w in words) + '.'              # (the importer lands the trailing silence on the full stop)
        out.append(dict(id='utt%02d' % u, audio=audio.astype(np.float32), text=text, words=[w.lower() for w in words], units=units,
                        pause=pause))
    return out


def truth_boundaries(item):
    """the inner boundaries of the truth in seconds (between consecutive units)"""
    return [u[2] / SAMPLE_RATE for u in item['units'][1:]]
