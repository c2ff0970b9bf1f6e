"""Mirror of cube/io_utils/io_phonemizer.py: the phonemizer's dataset, encodings and collate (same names, files, keys, dtypes and shapes).

An example is a dict {'orig_text', 'phones', 'words', 'phon2word'[, 'hybrid']}: `phones` holds one tag per character of `orig_text` ('_' where
a character is silent), `hybrid` the same sequence without the '_' tags.  One addition to the reference's interface: `PhonemizerCollate(encodings,
targets=...)` — the reference's collate prefers `hybrid`, which only fits its many-to-many model; the character tagger (CubenetPhonemizer, the model
the runtime loads) needs one target per character: targets='aligned'."""
import json

import numpy as np
import torch


class PhonemizerDataset:
    def __init__(self, filename: str):
        with open(filename) as f:
            self._examples = json.load(f)

    def __len__(self):
        return len(self._examples)

    def __getitem__(self, index):
        return self._examples[index]


class PhonemizerEncodings:
    def __init__(self, filename: str = None):
        self._grapheme2int = {}
        self._phon2int = {}
        if filename is not None:
            self.load(filename)

    def save(self, filename: str):
        with open(filename, 'w') as f:
            json.dump({'grapheme2int': self._grapheme2int, 'phon2int': self._phon2int}, f)

    def load(self, filename: str):
        with open(filename) as f:
            obj = json.load(f)
        self._grapheme2int, self._phon2int = obj['grapheme2int'], obj['phon2int']

    def compute(self, dataset):
        """ids in order of first appearance, 0 = 'PAD'; graphemes are lower-cased (the case travels in x_case)"""
        self._grapheme2int, self._phon2int = {'PAD': 0}, {'PAD': 0}
        for i in range(len(dataset)):
            example = dataset[i]
            for g in example['orig_text']:
                self._grapheme2int.setdefault(g.lower(), len(self._grapheme2int))
            for p in example['phones']:
                self._phon2int.setdefault(p, len(self._phon2int))

    @property
    def phonemes(self):
        return self._phon2int

    @property
    def graphemes(self):
        return self._grapheme2int


def encode_text(encodings, text, x_char, x_case):
    """fills one row of the collate's x_char / x_case: the id of the lower-cased character (0 when unknown) and 1 where lower-casing changed it"""
    g2i = encodings._grapheme2int
    for j, g in enumerate(text):
        low = g.lower()
        x_case[j] = int(low != g)
        x_char[j] = g2i.get(low, 0)


class PhonemizerCollate:
    def __init__(self, encodings: PhonemizerEncodings, targets: str = 'auto'):
        """targets: 'auto' — an example's `hybrid` list when it has one, else `phones` (the reference's behaviour); 'aligned' — always `phones`,
        which must then hold one tag per character of `orig_text` (y_phon.shape == x_char.shape)."""
        if targets not in ('auto', 'aligned'):
            raise ValueError("PhonemizerCollate: targets must be 'auto' or 'aligned', got %r" % (targets,))
        self._encodings = encodings
        self._targets = targets

    def _target_list(self, example):
        if self._targets == 'aligned':
            if len(example['phones']) != len(example['orig_text']):
                raise ValueError("PhonemizerCollate(targets='aligned'): %d phones for %d characters in %r — the tagger needs one tag per "
                                 "character ('_' for a silent one)" % (len(example['phones']), len(example['orig_text']), example['orig_text']))
            return example['phones']
        return example['hybrid'] if 'hybrid' in example else example['phones']

    def collate_fn(self, batch):
        B = len(batch)
        targets = [self._target_list(ex) for ex in batch]
        n_char = max(len(ex['orig_text']) for ex in batch)
        n_phon = max(len(ex['phones']) for ex in batch)      # (the reference sizes the targets by `phones` even when it fills in `hybrid`)
        x_char = np.zeros((B, n_char), dtype=np.int64)
        x_case = np.zeros((B, n_char), dtype=np.int64)
        y_phon = np.zeros((B, n_phon), dtype=np.int64)
        y_new_word = np.zeros((B, n_phon), dtype=np.int64)
        x_words = []
        p2i = self._encodings._phon2int
        for b, (ex, phones) in enumerate(zip(batch, targets)):
            spans, start = [], 0
            for w in ex['words']:
                spans.append({'word': w, 'start': start, 'stop': start + len(w)})
                start += len(w)
            x_words.append(spans)
            encode_text(self._encodings, ex['orig_text'], x_char[b], x_case[b])
            p2w = ex['phon2word']
            if self._targets == 'aligned' and len(p2w) != len(phones):
                # an example's phon2word indexes its '_'-free list; one tag per character lies in the word that character lies in
                p2w = [i for i, sp in enumerate(spans) for _ in range(sp['stop'] - sp['start'])]
                p2w = (p2w + [max(len(spans) - 1, 0)] * len(phones))[:len(phones)]
            for j, p in enumerate(phones):
                # 1 inside a word; at a word's last phone 1 + the number of words the next phone lies ahead (the very last phone counts one ahead)
                nxt = p2w[j + 1] if j + 1 < len(phones) else p2w[j] + 1
                y_new_word[b, j] = nxt - p2w[j] + 1 if nxt != p2w[j] else 1
                y_phon[b, j] = p2i.get(p, 0)
        return {'x_char': torch.from_numpy(x_char), 'x_case': torch.from_numpy(x_case), 'y_phon': torch.from_numpy(y_phon),
                'y_new_word': torch.from_numpy(y_new_word), 'x_words': x_words}
