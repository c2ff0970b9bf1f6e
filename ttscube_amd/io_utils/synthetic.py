"""Seeded synthetic training examples in the reference's per-example dict layout (cube/io_utils/io_cubegan.py:20-110: 'meta'
{phones, speaker, frame2phon, phon2word}, 'mgc' [F,80], 'pitch' [F], 'audio' [240 F]) — what the trainers and benches use when
no corpus is on disk (there is none in this environment: no network)."""
import numpy as np


SYNTHETIC_VOCABULARY = ['w%d' % i for i in range(64)]     # what `words=` draws from (a table for them: WordVectors.synthetic)


def _with_words(example, nwords, seed):
    """word fields for one example, from a generator of their own (the example's other fields keep the values they have without `words`):
    `nwords` words over contiguous, non-empty runs of phonemes, one or two words of left context, up to one of right context"""
    rng = np.random.RandomState(seed)
    meta = example['meta']
    nph = len(meta['phones'])
    nw = max(1, min(int(nwords), nph))
    cuts = np.sort(rng.choice(np.arange(1, nph), size=nw - 1, replace=False)) if nw > 1 else np.zeros(0, dtype=np.int64)
    meta['phon2word'] = [int(v) for v in np.searchsorted(cuts, np.arange(nph), side='right')]
    pick = lambda k: [SYNTHETIC_VOCABULARY[int(i)] for i in rng.randint(0, len(SYNTHETIC_VOCABULARY), size=k)]
    meta['words'], meta['words_left'], meta['words_right'] = pick(nw), pick(int(rng.randint(1, 3))), pick(int(rng.randint(0, 2)))
    return example


def synthetic_examples(n, seed, nphones=40, min_ph=20, max_ph=60, speakers=2, words=None):
    """`words` (optional): about that many words per sentence (`words`, `words_left`, `words_right` and a `phon2word` that points at them) — the
    fields the word-conditioned collate reads; None = none of them, every phoneme in word 0"""
    rng = np.random.RandomState(seed)
    for k in range(n):
        nph = int(rng.randint(min_ph, max_ph))
        durs = rng.randint(2, 12, size=nph)
        f2p = [p for p, d in enumerate(durs) for _ in range(d)]
        F_ = len(f2p)
        done = (lambda ex: ex) if words is None else (lambda ex, k=k: _with_words(ex, words, (seed * 7919 + k) % (2 ** 31)))
        yield done({'meta': {'phones': ['p%d' % v for v in rng.randint(0, nphones, size=nph)], 'speaker': 's%d' % rng.randint(0, speakers),
                        'frame2phon': f2p, 'phon2word': [0] * nph},
               'mgc': np.clip(rng.randn(F_, 80) - 2, -5, 1), 'pitch': rng.randint(60, 300, size=F_).astype(np.float64),
               'audio': (0.3 * np.sin(np.cumsum(rng.uniform(0.01, 0.3, size=F_ * 240)))).astype(np.float32)})


def synthetic_encodings(nphones=40, speakers=2):
    """encodings covering everything synthetic_examples can emit (identical on every rank)"""
    from .io_cubegan import CubeganEncodings
    enc = CubeganEncodings()
    enc.phon2int = {'p%d' % i: i for i in range(nphones)}
    enc.speaker2int = {'s%d' % i: i for i in range(speakers)}
    enc.max_pitch, enc.max_duration = 300, 12
    return enc


def synthetic_sentences(n, seed=1234, nphones=50, min_ph=20, max_ph=120):
    """BASELINE configs[4] text side: n random phoneme-id sentences, ids U{1..nphones} (0 = padding, the collate's
    `id + 1` convention of io_cubegan.py:219-231), lengths U{min_ph..max_ph}.  Returns (x_char [n, max_len] int64 zero-padded, lens)."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(min_ph, max_ph + 1, size=n)
    xc = np.zeros((n, int(lens.max())), dtype=np.int64)
    for b, l in enumerate(lens):
        xc[b, :l] = rs.randint(1, nphones + 1, size=l)
    return xc, lens
