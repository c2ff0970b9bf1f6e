"""Mirror of cube/io_utils/io_text.py:13-96 and cube/networks/g2p.py:247-264: the runtime text front-ends — plain text in, the
{'orig_text', 'words', 'phones', 'phon2word'} dict the synthesis collate reads out.

    text -> '§' wrapping / newline rules -> SimpleTokenizer (words) -> CubenetPhonemizer.tag (one tag per character, on the HIP kernels)
         -> curation: '_' tags dropped, every kept phone mapped to the word its character lies in

`batch(texts)` tags many sentences with one padded, length-aware `tag` call; each result equals the single call's.

``Text2Feat`` is the other front-end of the reference (io_text.py:64-96), for model directories whose phonemizer files are a word-level G2P:

    text -> newline rules / space wrapping -> networks.g2p.G2P (tokenizer, lexicon, attention decoder on ttsc_g2p_decode, non-word rules)
         -> '_' phones dropped, the empty-string phones of punctuation kept, every kept phone mapped to its token"""
import numpy as np
import torch

from .io_phonemizer import PhonemizerCollate, PhonemizerEncodings, encode_text


class Token:
    def __init__(self, word='', transcription=(), is_word=False):
        self.word = word
        self.transcription = list(transcription)
        self.is_word = is_word

    def __repr__(self):
        return '"%s"' % self.word if not self.transcription else '%s' % self.transcription


class SimpleTokenizer:
    """runs of letters and apostrophes are words; every other character is a token of its own"""

    def __call__(self, utterance):
        tokens, run = [], ''
        for ch in utterance:
            if ch.isalpha() or ch == '\'':
                run += ch
                continue
            if run:
                tokens.append(Token(word=run, is_word=True))
                run = ''
            tokens.append(Token(word=ch, is_word=False))
        if run:
            tokens.append(Token(word=run, is_word=True))
        return tokens


def normalize_text(text):
    """a blank line is a paragraph mark '§', a single newline a space; the sentence is wrapped in '§'"""
    text = text.replace('\n\n', '§').replace('\n', ' ')
    if not text.startswith('§'):
        text = '§' + text
    if not text.endswith('§'):
        text = text + '§'
    return text


def curate(text, words, tag_names):
    """tag_names: one tag per character of `text`; words: the tokenizer's words (they tile `text`).  Drops the '_' tags and walks characters and
    words in step: phon2word[i] = index of the word that holds the character phone i came from."""
    phones, phon2word = [], []
    w_index = c_pos = 0
    for name in tag_names:
        if name != '_':
            phones.append(name)
            phon2word.append(w_index)
        c_pos += 1
        if c_pos == len(words[w_index]):
            c_pos = 0
            w_index += 1
    return {'orig_text': text, 'words': words, 'phones': phones, 'phon2word': phon2word}


class Text2FeatBlizzard:
    def __init__(self, phonemizer_path: str, device='cuda:0'):
        from ..networks.phonemizer import CubenetPhonemizer
        self._encodings = PhonemizerEncodings('{0}.encodings'.format(phonemizer_path))
        self._phonemizer = CubenetPhonemizer(self._encodings)
        self._phonemizer.load('{0}.model'.format(phonemizer_path))
        self._phonemizer.eval()
        self._phonemizer.to(device)
        self._device = torch.device(device)
        self._tokenizer = SimpleTokenizer()
        self._collate = PhonemizerCollate(self._encodings)
        self._grapheme_list = [' '] * len(self._encodings.phonemes)     # (the reference's name: tag index -> phoneme symbol)
        for name, index in self._encodings.phonemes.items():
            self._grapheme_list[index] = name

    def _tags(self, texts):
        """normalised texts -> list of per-character tag index lists: ids, case flags and lengths go up in ONE copy, the tags come back in one"""
        B, N = len(texts), max(len(t) for t in texts)
        host = np.zeros(2 * B * N + B, dtype=np.int32)
        x_char, x_case = host[:B * N].reshape(B, N), host[B * N:2 * B * N].reshape(B, N)
        for b, t in enumerate(texts):
            encode_text(self._encodings, t, x_char[b], x_case[b])
            host[2 * B * N + b] = len(t)
        dev = torch.from_numpy(host).pin_memory().to(self._device, non_blocking=True)
        X = {'x_char': dev[:B * N].view(B, N), 'x_case': dev[B * N:2 * B * N].view(B, N)}
        lengths = None
        if B > 1:
            from .. import _lib
            lengths = _lib.DevLengths([len(t) for t in texts], dev_tensor=dev[2 * B * N:])
        tags = self._phonemizer.tag(X, lengths=lengths).cpu().numpy()
        return [tags[b, :len(t)].tolist() for b, t in enumerate(texts)]

    def _finish(self, text, tags):
        words = [w.word for w in self._tokenizer(text)]
        return curate(text, words, [self._grapheme_list[i] for i in tags])

    def __call__(self, text):
        text = normalize_text(text)
        return self._finish(text, self._tags([text])[0])

    def batch(self, texts):
        texts = [normalize_text(t) for t in texts]
        if not texts:
            return []
        return [self._finish(t, tags) for t, tags in zip(texts, self._tags(texts))]


def wrap_text(text):
    """io_text.py:73-79: newlines become spaces; the sentence is wrapped in spaces"""
    text = text.replace('\n\n', ' ').replace('\n', ' ')
    if not text.startswith(' '):
        text = ' ' + text
    if not text[-1] == ' ':
        text = text + ' '
    return text


def assemble(text, trace):
    """io_text.py:82-96: trace = [{'word', 'transcription'}] per token -> the front-end dict ('_' dropped, '' kept, as the reference keeps them)"""
    words, phones, phon2word = [], [], []
    for i, tok in enumerate(trace):
        words.append(tok['word'])
        for ph in tok['transcription']:
            if ph != '_':
                phones.append(ph)
                phon2word.append(i)
    return {'orig_text': text, 'words': words, 'phones': phones, 'phon2word': phon2word}


class Text2Feat:
    def __init__(self, phonemizer_path: str, device='cuda:0'):
        from ..networks.g2p import G2P
        g2p = G2P()
        g2p.load(phonemizer_path)
        g2p.load_lexicon('{0}.lexicon'.format(phonemizer_path))
        g2p.eval()
        g2p.to(device)
        self._phonemizer = g2p
        self._tokenizer = SimpleTokenizer()

    @classmethod
    def from_g2p(cls, g2p):
        """a front-end around an existing G2P object (its model already on its device)"""
        self = cls.__new__(cls)
        self._phonemizer = g2p
        self._tokenizer = SimpleTokenizer()
        return self

    def __call__(self, text):
        text = wrap_text(text)
        _, trace = self._phonemizer(text, trace=True)
        return assemble(text, trace)

    def batch(self, texts):
        """the words of all sentences in one decoder launch, each padded to its own sentence's N: every result equals the single call's"""
        texts = [wrap_text(t) for t in texts]
        if not texts:
            return []
        return [assemble(t, trace) for t, (_, trace) in zip(texts, self._phonemizer.batch(texts, trace=True))]
