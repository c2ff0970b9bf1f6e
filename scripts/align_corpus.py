"""Align a folder of recordings with their transcripts (io_utils/forced_align.py) and write the `<name>.TextGrid` files that
scripts/import_textgrid.py reads: `<name>.wav` with `<name>.txt` or `<name>.lab` (one line of text) in, word / phone / text tiers out.  The aligner
is a monophone Gaussian model trained here by Viterbi re-estimation on the very files it aligns (or loaded with --model-in, which trains nothing);
its boundaries are not Montreal Forced Aligner's.

    python scripts/align_corpus.py --input-folder recordings/ --lexicon en.lexicon --output-folder aligned/ --model-out aligner.npz
    python scripts/import_textgrid.py --input-folder aligned/ --speaker anna --prefix ANNA"""
import argparse
import os
import shutil
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def build_parser():
    p = argparse.ArgumentParser(description='Forced alignment of <name>.wav + <name>.txt / .lab pairs into <name>.TextGrid files')
    p.add_argument('--input-folder', dest='input_folder', required=True, help='Folder with <name>.wav and <name>.txt or <name>.lab (one line of text)')
    p.add_argument('--lexicon', required=True, help="'WORD<TAB>phones separated by blanks' per line; the first entry of a word stands")
    p.add_argument('--g2p', default=None, help='G2P checkpoint prefix for the words the lexicon lacks (default: such files are skipped)')
    p.add_argument('--output-folder', dest='output_folder', default=None, help='Where the TextGrids go (default: the input folder); the .wav files '
                   'are copied beside them when it is another folder')
    p.add_argument('--model-out', dest='model_out', default=None, help='Save the trained aligner here (.npz)')
    p.add_argument('--model-in', dest='model_in', default=None, help='Align with this model; nothing is trained')
    p.add_argument('--iterations', type=int, default=4, help='Re-estimation passes behind the flat start (default=4)')
    p.add_argument('--batch', type=int, default=32, help='Utterances per GPU call (default=32)')
    p.add_argument('--device', default='cuda:0', help='HIP device (default=cuda:0)')
    p.add_argument('--sample-rate', dest='sample_rate', type=int, default=24000, help='The files are brought to this rate (default=24000)')
    p.add_argument('--gpu-resample', dest='gpu_resample', action='store_true', help='Bring the files to --sample-rate on the GPU instead of with scipy')
    return p


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if a.batch < 1:
        p.error('--batch must be at least 1')
    if a.iterations < 0:
        p.error('--iterations must not be negative')
    if a.model_in and a.model_out:
        p.error('--model-in trains nothing: there is no model to write to --model-out')
    return a


def read_lexicon(path):
    """-> {WORD (upper case): [phones]}; the first entry of a word stands, lines without a tab are skipped"""
    lex = {}
    with open(path, encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split('\t')
            if len(parts) == 2 and parts[0].upper() not in lex:
                lex[parts[0].upper()] = parts[1].split()
    return lex


def find_files(folder):
    """(name, wav path, text) of every <name>.wav with a <name>.txt or <name>.lab beside it, sorted"""
    found = []
    for name in sorted(os.listdir(folder)):
        if not name.lower().endswith('.wav'):
            continue
        base = os.path.join(folder, name[:-4])
        for ext in ('.txt', '.lab'):
            if os.path.exists(base + ext):
                with open(base + ext, encoding='utf-8') as f:
                    found.append((name[:-4], os.path.join(folder, name), f.readline().strip()))
                break
    return found


def pronounce(text, lexicon, tokenizer, g2p=None):
    """-> (words, prons, unknown): the tokenizer's tokens (the importer tokenises the same text, so its tokens line up with the word tier), the
    phones of every word token ([] for the others) and the words neither the lexicon nor the G2P gave"""
    tokens = tokenizer(text)
    words, prons, unknown = [t.word for t in tokens], [], []
    for t in tokens:
        if not t.is_word:
            prons.append([])
        elif t.word.upper() in lexicon:
            prons.append(list(lexicon[t.word.upper()]))
        elif g2p is not None:
            prons.append([p for p in g2p.transcribe([t.word.lower()])[0] if p.strip() and p != '_'])
        else:
            prons.append([])
            unknown.append(t.word)
    return words, prons, unknown


def main(argv=None, make_aligner=None, out=None):
    """make_aligner (tests): callable(phones, device, model_in) -> a ForcedAligner built elsewhere, e.g. around injected host restatements"""
    a = parse_args(argv)
    out = out if out is not None else sys.stdout
    say = lambda line: out.write(line + '\n')
    from ttscube_amd.io_utils import forced_align as FA
    from ttscube_amd.io_utils.audio import load_wav
    from ttscube_amd.io_utils.io_text import SimpleTokenizer
    lexicon = read_lexicon(a.lexicon)
    g2p = None
    if a.g2p:
        from ttscube_amd.networks.g2p import G2P
        g2p = G2P()
        g2p.load(a.g2p)
        g2p.eval()
        g2p.to(a.device)
    resampler = None
    if a.gpu_resample:
        from ttscube_amd.io_utils.resample import Resampler
        resampler = Resampler(a.device)
    tokenizer = SimpleTokenizer()
    items, texts, skipped = [], {}, []
    for name, wav, text in find_files(a.input_folder):
        words, prons, unknown = pronounce(text, lexicon, tokenizer, g2p)
        if unknown:
            skipped.append((name, 'unknown words: ' + ' '.join(unknown)))
            continue
        if not any(prons):
            skipped.append((name, 'no word to align'))
            continue
        items.append({'id': name, 'audio': load_wav(wav, a.sample_rate, resampler=resampler)[0], 'words': words, 'prons': prons, 'wav': wav})
        texts[name] = text
    say('Found {0} files to align, {1} skipped'.format(len(items), len(skipped)))
    if make_aligner is not None:
        aligner = make_aligner(sorted({p for it in items for ph in it['prons'] for p in ph}), a.device, a.model_in)
    elif a.model_in:
        aligner = FA.ForcedAligner.load(a.model_in, device=a.device)
    else:
        aligner = FA.ForcedAligner(sorted({p for it in items for ph in it['prons'] for p in ph}), device=a.device, sample_rate=a.sample_rate)
    known = set(aligner.phones)
    for it in list(items):
        strange = sorted({p for ph in it['prons'] for p in ph} - known)
        if strange:
            skipped.append((it['id'], 'phones outside the model: ' + ' '.join(strange)))
            items.remove(it)
    if not a.model_in and items:
        aligner.fit(items, iterations=a.iterations, batch=a.batch, log=say)
        if a.model_out:
            aligner.save(a.model_out)
    out_dir = a.output_folder or a.input_folder
    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for it, rec in zip(items, aligner.align(items, batch=a.batch) if items else []):
        if not rec['ok']:
            skipped.append((it['id'], 'infeasible: fewer frames than lattice positions, or no finite path'))
            continue
        FA.to_textgrid(rec, texts[it['id']]).write(os.path.join(out_dir, it['id'] + '.TextGrid'))
        if os.path.abspath(out_dir) != os.path.abspath(a.input_folder):
            shutil.copyfile(it['wav'], os.path.join(out_dir, it['id'] + '.wav'))
        written += 1
    for name, why in skipped:
        say('Skipped {0}: {1}'.format(name, why))
    say('Wrote {0} TextGrid files to {1}'.format(written, out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
