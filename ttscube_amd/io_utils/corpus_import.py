"""Corpus import: a folder of `<name>.wav` + `<name>.TextGrid` pairs from Montreal Forced Aligner -> the processed corpus
`<out>/{train,dev}/<id>.{json,mgc,pitch,wav}` every trainer here reads.  The text side restates the reference's scripts/import_textgrid.py (word
alignment, phone merging, train/dev split, context lookup); the audio side is batched on the GPU: up to `batch` utterances go through ONE
MelVocoder.melspectrogram call and ONE PitchTracker call (io_utils/pitch.py).  librosa, soundfile, textgrid and pysptk are not needed; no `.png` is
rendered (nothing reads it).

TextGrid layout (MFA): tier 0 words, tier 1 phones, tier 2 one interval holding the original text."""
import datetime
import json
import os

import numpy as np

from .io_text import SimpleTokenizer
from .textgrid import TextGrid

FRAMES_PER_SECOND = 100     # frame2phon is at 10 ms whatever the hop size (the reference fixes 240 samples at 24 kHz)
N_FFT = 1024


# ---- text side ---------------------------------------------------------------------------------------------------------------------------------------

def word_cost(tg_text, tok_word):
    """0 for the same word (and for a pause against a non-letter token), 0.5 when one is a prefix or suffix of the other, else 1"""
    a, b = tg_text.lower(), tok_word.lower()
    if a == b or (a == '<eps>' and not b.isalpha()):
        return 0
    if a.startswith(b) or b.startswith(a) or a.endswith(b) or b.endswith(a):
        return 0.5
    return 1


def align_words(tg_words, tok_words):
    """Edit-distance alignment.  tg_words: dicts {'text', 'start', 'stop'} of the TextGrid's word tier, tok_words: the tokenizer's Tokens ->
    for every TextGrid word the index of the token it lands on.  Every move pays the pair's cost; the walk back prefers the diagonal, then
    dropping a TextGrid word."""
    n, m = len(tg_words), len(tok_words)
    d = [[0.0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        d[i][0] = float(i)
    for j in range(m + 1):
        d[0][j] = float(j)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            d[i][j] = min(d[i - 1][j - 1], d[i - 1][j], d[i][j - 1]) + word_cost(tg_words[i - 1]['text'], tok_words[j - 1].word)
    i, j = n, m
    tg2tok = [0] * n
    tg2tok[i - 1] = j - 1
    while i > 1 or j > 1:
        if i == 1:
            j -= 1
        elif j == 1:
            i -= 1
        elif d[i - 1][j - 1] <= d[i - 1][j] and d[i - 1][j - 1] <= d[i][j - 1]:
            i, j = i - 1, j - 1
        elif d[i - 1][j] <= d[i][j - 1]:
            i -= 1
        else:
            j -= 1
        tg2tok[i - 1] = j - 1
    return tg2tok


def merge(aligned_words, aligned_phons, tokenized_words):
    """-> phones (one symbol per phone; a token without aligned phones stands for itself with zero duration), phon2word (token index per phone),
    frame2phon (phone index per 10 ms frame over the span of the word tier)."""
    tg2tok = align_words(aligned_words, tokenized_words)
    tok2tg = {tok: tg for tg, tok in enumerate(tg2tok)}       # several TextGrid words on one token: the last one stands
    taken = [False] * len(aligned_phons)
    per_word, cursor = [], 0
    for ti, tok in enumerate(tokenized_words):
        if ti not in tok2tg:
            per_word.append([(tok.word, cursor, cursor)])
            continue
        w = aligned_words[tok2tg[ti]]
        mine = []
        for pi, ph in enumerate(aligned_phons):
            if not taken[pi] and ph['start'] >= w['start'] and ph['stop'] <= w['stop']:
                taken[pi] = True
                mine.append((ph['text'], ph['start'], ph['stop']))
        per_word.append(mine)
        cursor = w['stop']
    phones, phon2word, spans, cursor = [], [], [], 0
    for wi, tok in enumerate(tokenized_words):
        for sym, start, stop in per_word[wi] or [(tok.word, cursor, cursor)]:
            phones.append(sym)
            phon2word.append(wi)
            spans.append((start, stop))
        cursor = spans[-1][1]
    lo = min(w['start'] for w in aligned_words)
    hi = max(w['stop'] for w in aligned_words)
    frame2phon, pi = [], 0
    for frame in range(int((hi - lo) * FRAMES_PER_SECOND)):
        now = frame / FRAMES_PER_SECOND
        while pi < len(phones) and now > spans[pi][1]:
            pi += 1
        frame2phon.append(pi)
    return phones, phon2word, frame2phon


def fix_item(item, errors=None):
    """a phone symbol with a lower-case letter in it is not a phone of the aligner's set (a word that fell through): it becomes ' '.  `errors`
    collects the symbols met."""
    for i, ph in enumerate(item['phones']):
        if any(ch.isalpha() and ch.upper() != ch for ch in ph):
            if errors is not None:
                errors.setdefault(ph, len(errors))
            item['phones'][i] = ' '
    return item


def _squeeze(text, what, to):
    while what in text:
        text = text.replace(what, to)
    return text


def fetch_context(dataset, full_text):
    """full_text: the corpus' running text, paragraphs apart by blank lines.  Every item whose text occurs in a paragraph (case ignored) gets the
    rest of that paragraph as left_context / right_context.  -> number of items matched"""
    full_text = _squeeze(_squeeze(full_text, '\n\n\n', '\n\n'), '  ', ' ')
    paragraphs = [_squeeze(par.replace('\n', ' '), '  ', ' ') for par in full_text.split('\n\n')]
    matched = 0
    for item in dataset:
        text = item['orig_text'].strip().lower()
        for par in paragraphs:
            at = par.lower().find(text)
            if at >= 0:
                item['left_context'] = par[:at].strip()
                item['right_context'] = par[at + len(text):].strip()
                matched += 1
                break
    return matched


def split_train_dev(dataset, dev_ratio):
    """every int(1 / dev_ratio)-th item goes to the dev set; a ratio above 1 keeps everything for training, one in (0.5, 1] for dev"""
    every = int(1.0 / dev_ratio)
    if every == 0:
        print('Warning: invalid value for dev-ratio. Everything will be in the training set.')
        return list(dataset), []
    if every == 1:
        print('Warning: invalid value for dev-ratio. Everything will be in the dev set.')
        return [], list(dataset)
    train = [it for i, it in enumerate(dataset) if (i + 1) % every != 0]
    dev = [it for i, it in enumerate(dataset) if (i + 1) % every == 0]
    return train, dev


def find_pairs(folder):
    """(path without extension, TextGrid path) of every *.TextGrid below `folder` that has a .wav beside it, sorted"""
    found = []
    for root, _, files in os.walk(folder):
        for name in files:
            if name.lower().endswith('.textgrid') and os.path.exists(os.path.join(root, name[:-9] + '.wav')):
                found.append((os.path.join(root, name[:-9]), os.path.join(root, name)))
    return sorted(found)


def _tier(tier):
    return [{'text': iv.mark, 'start': iv.minTime, 'stop': iv.maxTime} for iv in tier]


def read_item(base, speaker, tokenizer=None, tg_path=None):
    """one TextGrid (`<base>.TextGrid` unless tg_path names it) -> the item dict of `<id>.json` (without 'id' and the contexts)"""
    tokenizer = tokenizer or SimpleTokenizer()
    tg = TextGrid.fromFile(tg_path or base + '.TextGrid')
    orig_text = ' ' + tg[2][0].mark
    words = _tier(tg[0])
    if words[0]['text'] not in ('<eps>', ''):
        words.insert(0, {'text': ' ', 'start': 0, 'stop': 0})     # the dummy leading pause: the sentence starts on a word
    tokens = tokenizer(orig_text)
    phones, phon2word, frame2phon = merge(words, _tier(tg[1]), tokens)
    return {'orig_start': 0, 'orig_end': len(frame2phon) * 10, 'orig_filename': os.path.basename(base), 'orig_text': orig_text, 'phones': phones,
            'words': [t.word for t in tokens], 'phon2word': phon2word, 'frame2phon': frame2phon, 'speaker': speaker}


# ---- audio side --------------------------------------------------------------------------------------------------------------------------------------

def _write_item(folder, item, seg, mel, pitch, sample_rate):
    from .audio import save_wav
    base = os.path.join(folder, item['id'])
    save_wav(base + '.wav', np.asarray(seg * 32767, dtype=np.int16), sample_rate)
    with open(base + '.mgc', 'wb') as f:                           # bare np.save streams: the readers open these names as they are
        np.save(f, mel)
    with open(base + '.pitch', 'wb') as f:
        np.save(f, pitch)
    with open(base + '.json', 'w') as f:
        json.dump(item, f)


def import_audio(dataset, paths, output_folder, sample_rate, hop_size, prefix, batch=32, device='cuda:0', fmin=60, fmax=400, resampler=None):
    """dataset: item dicts (sorted here by file name; ids are '<prefix>_<index:08d>' in that order), paths: orig_filename -> path without
    extension; resampler: an io_utils.resample.Resampler brings the files to sample_rate on the GPU (default: scipy on the host).
    -> number of utterances written"""
    from .audio import load_wav
    from .pitch import PitchTracker
    from .vocoder import MelVocoder
    os.makedirs(output_folder, exist_ok=True)
    vocoder, tracker = MelVocoder(device), PitchTracker(device)
    dataset.sort(key=lambda it: it['orig_filename'])
    per_ms = sample_rate / 1000
    half = N_FFT // 2
    pending, written = [], 0

    def flush():
        nonlocal written
        if not pending:
            return
        lens = [len(seg) for _, seg in pending]
        Lmax = max(lens)
        # one row per utterance.  The spectrogram reflects a signal about its last sample; a shorter row of a padded batch carries its own reflection
        # behind its end, so that its frames see the samples they see when it is analysed alone, whatever else is in the batch
        rows = np.zeros((len(pending), Lmax + half), dtype=np.float32)
        for r, (_, seg) in enumerate(pending):
            rows[r, :len(seg)] = seg
            rows[r, len(seg):len(seg) + half] = seg[-2:-2 - half:-1]
        mels = vocoder.melspectrogram(rows, sample_rate, 80, hop_size, False)
        f0 = tracker(rows[:, :Lmax], sample_rate, hop_size, fmin=fmin, fmax=fmax, lengths=lens)
        for r, (item, seg) in enumerate(pending):
            _write_item(output_folder, item, seg, np.ascontiguousarray(mels[r, :1 + lens[r] // hop_size]), np.ascontiguousarray(f0[r, :lens[r] // hop_size]),
                        sample_rate)
            written += 1
        pending.clear()

    wav, loaded = None, None
    for index, item in enumerate(dataset):
        item['id'] = '{0}_{1:08d}'.format(prefix, index)
        if loaded != item['orig_filename']:
            wav, _ = load_wav(paths[item['orig_filename']] + '.wav', sample_rate, resampler=resampler)
            loaded = item['orig_filename']
        seg = np.asarray(wav[int(item['orig_start'] * per_ms):int(item['orig_end'] * per_ms)], dtype=np.float32)
        peak = float(np.max(np.abs(seg))) if seg.size else 0.0
        if peak == 0.0:
            print('Skipping {0} ({1}): the segment is empty or all zeros'.format(item['id'], item['orig_filename']))
            continue
        if seg.size <= half:
            print('Skipping {0} ({1}): {2} samples are fewer than half an analysis window'.format(item['id'], item['orig_filename'], seg.size))
            continue
        pending.append((item, (seg / np.float32(peak)) * np.float32(0.98)))
        if len(pending) >= batch:
            flush()
    flush()
    return written


def import_dataset(input_folder, output_folder='data/processed', dev_ratio=0.001, speaker='none', sample_rate=24000, hop_size=240, prefix='FILE',
                   original_text=None, batch=32, device='cuda:0', resampler=None):
    """-> (utterances written to train, to dev)"""
    print('Search input folder for valid files')
    bases = find_pairs(input_folder)
    print('Found {0} aligned files'.format(len(bases)))
    tokenizer = SimpleTokenizer()
    dataset, paths = [], {}
    for base, tg_path in bases:
        item = read_item(base, speaker, tokenizer, tg_path)
        item['left_context'] = item['right_context'] = ''
        paths[item['orig_filename']] = base
        dataset.append(item)
    total_ms = sum(it['orig_end'] for it in dataset)
    train, dev = split_train_dev(dataset, dev_ratio)
    print('Found {0} valid sentences, with a total audio time of {1}.'.format(len(dataset), datetime.timedelta(seconds=total_ms / 1000)))
    print('Trainset will contain {0} examples and devset {1} examples'.format(len(train), len(dev)))
    if original_text:
        print('Fetching context')
        with open(original_text) as f:
            full_text = f.read()
        for part in (train, dev):
            print('Matched {0} from {1}'.format(fetch_context(part, full_text), len(part)))
    errors = {}
    for part in (train, dev):
        for item in part:
            fix_item(item, errors)
    counts = []
    for name, part in (('train', train), ('dev', dev)):
        print('Processing {0}set'.format(name))
        counts.append(import_audio(part, paths, os.path.join(output_folder, name), sample_rate, hop_size, prefix, batch=batch, device=device, resampler=resampler))
    return tuple(counts)
