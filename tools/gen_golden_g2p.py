"""Golden vectors for the word-level G2P front-end, produced by the REFERENCE ITSELF (build container only; the reference never travels).

    python tools/gen_golden_g2p.py   ->  tests/golden/g2p.lexicon, g2p.encodings, g2p_a.npz, g2p_b.npz, g2p_c.npz

g2p.lexicon: at most 2 000 lines of the reference's data/models/en-g2p.lexicon (data its programs read): every STRIDE-th line plus the lines of
a few words the fixture texts use.  g2p.encodings: what the reference's G2P.update_encodings + save produce from that subset.
Weights: the reference's Seq2Seq filled by oracle.meldecoder_ref.fill_state_dict (the fixtures store seed + shapes) with EOS_OFFSET added to
output.bias[<EOS>] — without it seeded weights never emit <EOS> and every word runs 10 N + 1 steps; with it words stop at varied step counts.

  g2p_a   a padded batch of lexicon words: x, teacher labels y, the teacher-forced logits, the reference's `transcribe` of the words
  g2p_b   the words of two sentences and one long text: x, the free-running logits of Seq2Seq.forward(x) (kept at the steps each word uses,
          zero elsewhere, with the reference's shape), step counts, `transcribe` output, per-word smallest top-2 margin over the used steps
  g2p_c   the whole dict the reference's Text2Feat returns for one text (a lexicon hit, an out-of-lexicon word, an apostrophe word, '-', '"',
          other punctuation, a newline) and the reference's own transcription of each of its words

The generator prints every fixture's smallest top-2 logit margin over the steps each word actually uses; g2p_c is refused when any word has a
step below 2e-4, the others when more than 5 % of their words have one (the phonemizer fixtures' conditions)."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

ref_import.setup()
from cube.io_utils.io_text import Text2Feat  # noqa: E402
from cube.networks.g2p import G2P, G2PDataset  # noqa: E402
from oracle import meldecoder_ref as M  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
REF_LEXICON = os.path.join(ref_import.REF, 'data', 'models', 'en-g2p.lexicon')
MARGIN = 2e-4
MAX_LINES = 2000
SEED = 33
EOS_OFFSET = 0.15
EOS = 2
KEEP_WORDS = ('GOOD', 'MORNING', 'WELCOME', 'WORLD', 'SPEECH', "DON'T", 'ABOUT', 'THE', 'AND', 'TO')

TEXT_C = 'Good morning - and welcome, to the "zorblax" world!\nDon\'t panic.'
TEXTS_B = {
    's1': 'Good morning and welcome to the world of speech synthesis',
    's2': "Don't feel bad about us we're only here to help",
    'long': ('It was the best of times it was the worst of times it was the age of wisdom it was the age of foolishness '
             "nobody's fault said the extraordinarily uncharacteristic gentleman smiling the quick brown fox jumps over the lazy dog"),
}


def lexicon_subset():
    with open(REF_LEXICON) as f:
        lines = f.readlines()
    keep = [i for i, l in enumerate(lines) if l.split('\t')[0] in KEEP_WORDS]
    stride = len(lines) // (MAX_LINES - len(keep)) + 1
    idx = sorted(set(range(0, len(lines), stride)) | set(keep))
    assert len(idx) <= MAX_LINES
    return [lines[i] for i in idx]


def seeded(g2p):
    torch.manual_seed(0)
    g2p.initialize_network()
    shapes = M.named_shapes(g2p.seq2seq)
    sd = M.fill_state_dict(shapes, SEED)
    sd['output.bias'][EOS] += EOS_OFFSET
    g2p.seq2seq.load_state_dict(sd, strict=True)
    g2p.seq2seq.eval()
    return shapes


def encode(g2p, words):
    """the id matrix G2P.transcribe builds (g2p.py:125-136)"""
    N = max(len(w) for w in words) + 1
    x = np.zeros((len(words), N), dtype=np.int64)
    for i, w in enumerate(words):
        for j in range(N):
            if j < len(w):
                x[i, j] = g2p.token2int.get(w[j].lower(), g2p.token2int['<UNK>'])
            elif j == len(w):
                x[i, j] = g2p.token2int['<EOS>']
    return x


def used_steps(logits):
    """steps each word uses: up to and including its first <EOS>, all of them when it has none"""
    am = logits.argmax(dim=-1).numpy()
    out = []
    for row in am:
        hit = np.nonzero(row == EOS)[0]
        out.append(int(hit[0]) + 1 if len(hit) else len(row))
    return np.asarray(out)


def word_margins(logits, counts):
    top = torch.topk(logits, 2, dim=-1).values
    mg = (top[..., 0] - top[..., 1]).numpy()
    return np.asarray([mg[i, :c].min() for i, c in enumerate(counts)])


def report(name, logits, counts, margins, strict):
    low = float((margins < MARGIN).mean())
    print('%s: %d words, T %d, steps %s, logit rms %.3f, min margin %.3e, words below %.0e: %.1f %%'
          % (name, logits.shape[0], logits.shape[1], sorted(set(counts.tolist())), float(logits.pow(2).mean().sqrt()), margins.min(), MARGIN, 100 * low))
    if strict and margins.min() < MARGIN:
        raise SystemExit('%s: a word has a step below %g — pick another seed / text' % (name, MARGIN))
    if low > 0.05:
        raise SystemExit('%s: more than 5 %% of the words have a step below the margin — pick another seed / text' % name)


def free_run(g2p, words):
    x = encode(g2p, words)
    with torch.no_grad():
        logits = g2p.seq2seq(torch.from_numpy(x))
    counts = used_steps(logits)
    margins = word_margins(logits, counts)
    trans = g2p.transcribe(words)
    kept = logits.clone()
    for i, c in enumerate(counts):
        kept[i, c:] = 0
    return x, logits, kept, counts, margins, trans


if __name__ == '__main__':
    lex = lexicon_subset()
    with open(os.path.join(OUT, 'g2p.lexicon'), 'w') as f:
        f.writelines(lex)
    ds = G2PDataset(os.path.join(OUT, 'g2p.lexicon'))
    g2p = G2P()
    g2p.update_encodings(ds)
    g2p.save(os.path.join(OUT, 'g2p'))
    with open(os.path.join(OUT, 'g2p.encodings')) as f:
        enc_json = f.read()
    shapes = seeded(g2p)
    print('g2p.lexicon: %d lines, %d tokens, %d labels' % (len(lex), len(g2p.token2int), len(g2p.label2int)))
    common = dict(seed=SEED, shapes=json.dumps(shapes), enc=enc_json, eos_offset=EOS_OFFSET)

    # (a) teacher forcing on a padded batch of lexicon words
    exs = [ds.examples[i] for i in range(7, len(ds.examples), len(ds.examples) // 13)][:13]
    words = [w for w, _ in exs]
    x = encode(g2p, words)
    T = max(len(t) for _, t in exs) + 1
    y = np.zeros((len(exs), T), dtype=np.int64)
    for i, (_, t) in enumerate(exs):
        for j in range(T):
            if j < len(t):
                y[i, j] = g2p.label2int.get(t[j], g2p.label2int['<UNK>'])
            elif j == len(t):
                y[i, j] = g2p.label2int['<EOS>']
    with torch.no_grad():
        logits = g2p.seq2seq(torch.from_numpy(x), gs_output=torch.from_numpy(y))
    _, flog, _, counts, margins, trans = free_run(g2p, words)
    report('g2p_a (free run of its words)', flog, counts, margins, False)
    np.savez_compressed(os.path.join(OUT, 'g2p_a.npz'), words=json.dumps(words), x=x, y=y, logits=logits.numpy(), transcriptions=json.dumps(trans),
                        free_counts=counts, free_margins=margins, **common)

    # (b) free running: the words of two sentences and one long text
    out = dict(common, names=json.dumps(list(TEXTS_B)))
    for name, text in TEXTS_B.items():
        words = [w.lower() for w in text.split(' ')]
        x, logits, kept, counts, margins, trans = free_run(g2p, words)
        report('g2p_b/' + name, logits, counts, margins, False)
        out.update({name + '/words': json.dumps(words), name + '/x': x, name + '/logits': kept.numpy(), name + '/counts': counts,
                    name + '/margins': margins, name + '/transcriptions': json.dumps(trans)})
    np.savez_compressed(os.path.join(OUT, 'g2p_b.npz'), **out)

    # (c) the whole front-end
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, 'en-g2p')
        g2p.save(base)
        g2p.seq2seq.save(base + '.best')
        with open(base + '.lexicon', 'w') as f:
            f.writelines(lex)
        t2f = Text2Feat(base)
        rez = t2f(TEXT_C)
        words = [t.word.lower() for t in t2f._tokenizer(rez['orig_text']) if t.is_word]
        x, logits, _, counts, margins, trans = free_run(t2f._phonemizer, words)
        hits = [w for w in words if w in t2f._phonemizer.lookup]
    assert hits and len(hits) < len(words) and any("'" in w for w in words) and '' in rez['phones']
    report('g2p_c', logits, counts, margins, True)
    np.savez_compressed(os.path.join(OUT, 'g2p_c.npz'), text=TEXT_C, result=json.dumps(rez), words=json.dumps(words),
                        transcriptions=json.dumps(trans), counts=counts, margins=margins, **common)
    for fn in ('g2p.lexicon', 'g2p.encodings', 'g2p_a.npz', 'g2p_b.npz', 'g2p_c.npz'):
        print('%-16s %7d bytes' % (fn, os.path.getsize(os.path.join(OUT, fn))))
