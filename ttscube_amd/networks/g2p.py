"""Mirror of cube/networks/g2p.py: ``G2P`` — the word-level grapheme-to-phoneme front-end (attention seq2seq + pronunciation lexicon) behind
``io_utils.io_text.Text2Feat`` — ``G2PDataset`` and the command line of the reference's file.  Inference; the training path is networks/g2p_train.py.

    words -> token ids (g2p.py:123-137: lower-cased characters, <UNK> = 1, <EOS> = 2 at position len, <PAD> = 0 after; N = longest word + 1)
          -> Seq2Seq.transcribe_ids (one ttsc_g2p_decode launch for all words, each stopping at its own first <EOS>)
          -> labels: <PAD> / <UNK> dropped, cut at the first <EOS>

A per-word stop gives the transcriptions the reference gives: its batch-wide loop only computes steps ``transcribe`` throws away.
``__call__`` applies the lexicon and the non-word rules (g2p.py:189-206).  Words the lexicon holds are not decoded, but they count towards N, so
the other words see the reference's padding; when every word is a lexicon hit no kernel is launched.  ``batch`` does the same for many
utterances in one launch, every word padded to its own utterance's N.

    python -m ttscube_amd.networks.g2p --test-file FILE --load BASE                        word accuracy
    python -m ttscube_amd.networks.g2p --transcribe-file FILE --model BASE --output-file OUT
Training (the reference's third mode) is not built INTO THIS COMMAND, which exits non-zero there: it is scripts/train_g2p.py (same flags and files) on
networks/g2p_train.py (learn_batch, g2p_training_step: the HIP attention-decoder forward / backward)."""
import json
import optparse
import os
import sys

import numpy as np
import torch

from ..io_utils.io_text import SimpleTokenizer, Token  # noqa: F401  (re-exported under the reference's names)
from .seq2seq import Seq2Seq, check_status


class G2P:
    def __init__(self):
        self.seq2seq = None
        self.token2int = {'<PAD>': 0, '<UNK>': 1, '<EOS>': 2}
        self.label2int = {'<PAD>': 0, '<UNK>': 1, '<EOS>': 2}
        self.label_list = ['<PAD>', '<UNK>', '<EOS>']
        self.simple_tokenizer = SimpleTokenizer()
        self.lookup = {}

    def to(self, device):
        self.seq2seq.to(device)

    def load(self, path, load_last=False):
        with open('{0}.encodings'.format(path), 'r') as f:
            json_obj = json.load(f)
        self.token2int = json_obj['token2int']
        self.label2int = json_obj['label2int']
        self.label_list = json_obj['label_list']
        self.initialize_network()
        if load_last:
            self.seq2seq.load('{0}.last'.format(path))
        elif os.path.exists('{0}.best'.format(path)):
            self.seq2seq.load('{0}.best'.format(path))
        else:
            self.seq2seq.load('{0}.model'.format(path))

    def save(self, path):
        with open('{0}.encodings'.format(path), 'w') as f:
            json.dump({'token2int': self.token2int, 'label_list': self.label_list, 'label2int': self.label2int}, f, indent=2)

    def update_encodings(self, dataset, cutoff=2):
        """g2p.py:63-86: characters / phones seen at least `cutoff` times, in order of first appearance"""
        token2count, label2count = {}, {}
        for word, trans in dataset.examples:
            for char in word.lower():
                token2count[char] = token2count.get(char, 0) + 1
            for phon in trans:
                label2count[phon] = label2count.get(phon, 0) + 1
        for token, cnt in token2count.items():
            if cnt >= cutoff:
                self.token2int[token] = len(self.token2int)
        for label, cnt in label2count.items():
            if cnt >= cutoff:
                self.label2int[label] = len(self.label2int)
                self.label_list.append(label)

    def initialize_network(self):
        self.seq2seq = Seq2Seq(len(self.token2int), len(self.label2int))

    def eval(self):
        self.seq2seq.eval()

    def train(self):
        self.seq2seq.train()

    def _get_device(self):
        return self.seq2seq._get_device()

    # ---- words -> transcriptions ------------------------------------------------------------------------------------------------------------
    def encode_words(self, words, N=None):
        """g2p.py:125-136 -> int64 [len(words), N] (N: longest word + 1 unless given)"""
        if N is None:
            N = max(len(w) for w in words) + 1
        pad, unk, eos = self.token2int['<PAD>'], self.token2int['<UNK>'], self.token2int['<EOS>']
        x = np.full((len(words), N), pad, dtype=np.int64)
        for i, w in enumerate(words):
            for j, ch in enumerate(w):
                x[i, j] = self.token2int.get(ch.lower(), unk)
            x[i, len(w)] = eos
        return x

    def labels_to_phones(self, labels):
        """g2p.py:144-152 on one word's arg-max labels"""
        pad, unk, eos = self.label2int['<PAD>'], self.label2int['<UNK>'], self.label2int['<EOS>']
        tr = []
        for index in labels:
            if index == eos:
                break
            if index != pad and index != unk:
                tr.append(self.label_list[index])
        return tr

    def _decode_words(self, words, ns):
        """words with their padded lengths ns (one launch) -> transcriptions"""
        N = max(ns)
        x = torch.from_numpy(self.encode_words(words, N)).to(self._get_device())
        idx, count = self.seq2seq.transcribe_ids(x, n=None if all(v == N for v in ns) else list(ns))
        idx, count = idx.cpu().numpy(), count.cpu().numpy()
        check_status('G2P.transcribe')
        return [self.labels_to_phones(idx[i, :count[i]].tolist()) for i in range(len(words))]

    def transcribe(self, words):
        """g2p.py:123-154: every word padded to the longest of the list + 1"""
        N = max(len(w) for w in words) + 1
        return self._decode_words(list(words), [N] * len(words))

    def load_lexicon(self, path):
        """g2p.py:156-166: 'word<TAB>phones separated by blanks'; other lines are skipped"""
        with open(path) as f:
            for line in f:
                parts = line.strip().split('\t')
                if len(parts) != 2:
                    continue
                self.lookup[parts[0].lower()] = parts[1].split(' ')

    # ---- utterances ---------------------------------------------------------------------------------------------------------------------------
    def _plan(self, utterance):
        tokens = self.simple_tokenizer(utterance)
        words = [t.word.lower() for t in tokens if t.is_word]
        N = max(len(w) for w in words) + 1 if words else 0      # lexicon hits count: the other words see the reference's padding
        return tokens, words, N

    def _finish(self, tokens, decoded, trace):
        """g2p.py:187-210; decoded: {word: transcription} of the words the lexicon does not hold"""
        trace_words = []
        for token in tokens:
            if token.is_word:
                w = token.word.lower()
                token.transcription = self.lookup[w] if w in self.lookup else decoded[w]
            elif token.word == ' ':
                token.transcription = [' ']
            elif token.word == '-' or token.word == '"':
                token.transcription = ['_']
            else:
                token.transcription = ['']
            trace_words.append({'word': token.word, 'transcription': token.transcription})
        return (tokens, trace_words) if trace else tokens

    def batch(self, utterances, trace=False):
        """many utterances, ONE decoder launch: each word is padded to its own utterance's N, so every result equals the single call's"""
        plans = [self._plan(u) for u in utterances]
        todo = {}
        for _, words, N in plans:
            for w in words:
                if w not in self.lookup:
                    todo.setdefault((w, N), None)
        keys = list(todo)
        if keys:
            for k, tr in zip(keys, self._decode_words([k[0] for k in keys], [k[1] for k in keys])):
                todo[k] = tr
        return [self._finish(tokens, {w: todo[(w, N)] for w in words if w not in self.lookup}, trace) for tokens, words, N in plans]

    def __call__(self, utterance, trace=False):
        return self.batch([utterance], trace=trace)[0]

    def evaluate(self, dataset):
        """g2p.py:212-225: word accuracy.  Deviation: batches of 64 INCLUDING the last partial one and never an empty one — the reference's
        _get_batches drops every example when there are fewer than 64 and crashes on an exact multiple of 64 (its trailing empty batch)."""
        err, total = 0, len(dataset.examples)
        for s in range(0, total, 64):
            chunk = dataset.examples[s:s + 64]
            for (_, gold), pred in zip(chunk, self.transcribe([ex[0] for ex in chunk])):
                err += int(pred != gold)
        return 1.0 - err / total


class G2PDataset:
    def __init__(self, file):
        self.examples = []
        with open(file) as f:
            for line in f:
                parts = line.strip().split('\t')
                if len(parts) != 2:
                    continue
                self.examples.append((parts[0], parts[1].split(' ')))


def _eval(params):
    dev = G2PDataset(params.test_file)
    g2p = G2P()
    g2p.load(params.model_path)
    g2p.to(params.device)
    g2p.eval()
    sys.stdout.write('Word accuracy rate is {0:.2f}%\n'.format(g2p.evaluate(dev) * 100))


def _transcribe(params):
    g2p = G2P()
    g2p.load(params.model_base)
    g2p.to(params.device)
    g2p.eval()
    with open(params.transcribe_file) as f:
        lines = f.readlines()
    BS = 128
    with open(params.output_file, 'w') as f:
        for start in range(0, len(lines), BS):
            words = [p.split('\t')[0].strip() for p in lines[start:start + BS]]
            for w, t in zip(words, g2p.transcribe(words)):
                f.write('{0}\t{1}\n'.format(w, ' '.join(t)))


def main(argv):
    parser = optparse.OptionParser()
    parser.add_option('--patience', action='store', dest='patience', default=20, type='int', help='Num epochs without improvement (default=20)')
    parser.add_option('--train-file', action='store', dest='train_file', help='Training file for g2p')
    parser.add_option('--dev-file', action='store', dest='dev_file', help='Validation file for g2p')
    parser.add_option('--store', action='store', dest='output_path', help='Base path for storing output model')
    parser.add_option('--batch-size', action='store', dest='batch_size', default='32', type='int',
                      help='number of samples in a single batch (default=32)')
    parser.add_option('--resume', action='store_true', dest='resume', help='Resume from previous checkpoint')
    parser.add_option('--device', action='store', dest='device', default='cuda:0')
    parser.add_option('--lr', action='store', dest='lr', default=1e-3, type=float)
    parser.add_option('--load', action='store', dest='model_path')
    parser.add_option('--test-file', action='store', dest='test_file')
    parser.add_option('--transcribe-file', action='store', dest='transcribe_file')
    parser.add_option('--output-file', action='store', dest='output_file')
    parser.add_option('--model', action='store', dest='model_base')
    (params, _) = parser.parse_args(argv)
    if params.test_file and params.model_path:
        _eval(params)
    elif params.transcribe_file:
        _transcribe(params)
    else:
        sys.stderr.write('G2P training is not built here (no attention / decoder backward); checkpoints trained by the reference load unchanged. '
                         'Use --test-file FILE --load BASE or --transcribe-file FILE --model BASE --output-file OUT; to train, run scripts/train_g2p.py '
                         '(networks/g2p_train.py).\n')
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
