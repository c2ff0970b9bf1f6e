"""Word vectors from a LOCAL file, for `conditioning='fasttext:<lang>'` (cube/io_utils/io_cubegan.py:161-165, 233-244: the reference downloads
`cc.<lang>.300.bin` and asks the fastText library for every word's vector).  Neither the download nor the library is available to this build; the table
the user already has is read instead."""
import os

import numpy as np


class WordVectors:
    """`WordVectors(path)` reads

      * fastText's TEXT format (`.vec`, what `cc.<lang>.300.vec` is): a header line `count dim`, then one `word v1 ... vdim` line per word; or
      * an `.npz` with `words` (array of strings) and `vectors` (float [count, dim]).

    `dim`, `get_word_vector(word) -> float32 [dim]` and `word in table` are the surface the collate uses (the first two are the fastText model's own).

    Stated deviation: a word that is not in the table gives the ZERO vector.  fastText's `.bin` models compose a vector for such a word from its
    character n-grams; that needs the binary model and the library and is not rebuilt here.  A model trained with this table must be run with it."""

    def __init__(self, path=None, words=None, vectors=None):
        if path is not None:
            words, vectors = self._read_npz(path) if str(path).endswith('.npz') else self._read_vec(path)
        vectors = np.ascontiguousarray(np.asarray(vectors, dtype=np.float32))
        words = [str(w) for w in words]
        if vectors.ndim != 2 or vectors.shape[0] != len(words) or vectors.shape[1] == 0:
            raise ValueError('WordVectors: %d words but vectors of shape %s' % (len(words), vectors.shape))
        self._vectors = vectors
        self._index = {}
        for i, w in enumerate(words):
            self._index.setdefault(w, i)          # (a repeated word keeps its first vector)
        self._zero = np.zeros(vectors.shape[1], dtype=np.float32)
        self.path = path

    @staticmethod
    def _read_npz(path):
        with np.load(path, allow_pickle=False) as z:
            if 'words' not in z.files or 'vectors' not in z.files:
                raise ValueError('%s: an .npz word-vector table holds `words` and `vectors` (found %s)' % (path, z.files))
            return list(z['words']), z['vectors']

    @staticmethod
    def _read_vec(path):
        with open(path, encoding='utf-8', errors='replace') as f:
            head = f.readline().split()
            if len(head) != 2 or not all(t.isdigit() for t in head):
                raise ValueError('%s: the first line of a .vec file is `count dim` (got %r)' % (path, ' '.join(head)[:60]))
            count, dim = int(head[0]), int(head[1])
            words, rows = [], np.zeros((count, dim), dtype=np.float32)
            for line in f:
                parts = line.rstrip('\n').rstrip(' ').rsplit(' ', dim)     # (a "word" may itself contain blanks: the LAST dim fields are the vector)
                if len(parts) != dim + 1:
                    if not line.strip():
                        continue
                    raise ValueError('%s: line %d has %d fields, expected a word and %d values' % (path, len(words) + 2, len(parts), dim))
                if len(words) == count:
                    raise ValueError('%s: more than the %d words its header announces' % (path, count))
                rows[len(words)] = np.asarray(parts[1:], dtype=np.float32)
                words.append(parts[0])
        if len(words) != count:
            raise ValueError('%s: header announces %d words, file holds %d' % (path, count, len(words)))
        return words, rows

    @classmethod
    def synthetic(cls, words, dim=300, seed=0, scale=0.3):
        """seeded N(0, scale^2) vectors for `words` (trainers and benches without a table on disk)"""
        words = list(dict.fromkeys(str(w) for w in words))
        return cls(words=words, vectors=np.random.RandomState(seed).randn(len(words), dim).astype(np.float32) * scale)

    @classmethod
    def resolve(cls, source):
        """a table from what the public entry points accept: a WordVectors, or a path"""
        if source is None or isinstance(source, cls):
            return source
        if isinstance(source, (str, os.PathLike)):
            return cls(os.fspath(source))
        raise TypeError('word_vectors: a path or a WordVectors, not %r' % type(source).__name__)

    @property
    def dim(self):
        return int(self._vectors.shape[1])

    def __len__(self):
        return len(self._index)

    def __contains__(self, word):
        return str(word) in self._index

    def get_word_vector(self, word):
        i = self._index.get(str(word))
        return self._zero if i is None else self._vectors[i]

    def subset(self, words):
        """the table cut down to those of `words` it holds (what a trainer stores beside a checkpoint: a corpus uses a few thousand of the
        millions of words of a distributed table; every other word gave the zero vector in training and does so again at run time)"""
        keep = [w for w in dict.fromkeys(str(w) for w in words) if w in self._index]
        return WordVectors(words=keep, vectors=self._vectors[[self._index[w] for w in keep]].reshape(len(keep), self.dim))

    def save_npz(self, path):
        words = list(self._index)
        np.savez_compressed(path, words=np.asarray(words), vectors=self._vectors[[self._index[w] for w in words]])
