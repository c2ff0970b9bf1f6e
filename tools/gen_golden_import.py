"""Build machine only: record what the reference's `_merge` (scripts/import_textgrid.py) returns for a handful of hand-written alignments, as
tests/golden/import_textgrid_merge.json.  The four modules the reference script imports and this machine lacks (librosa, soundfile, textgrid, pysptk)
— and tqdm / PIL where absent — are stubbed in sys.modules: `_merge` touches none of them.  The file holds the inputs (ours) and the three returned
lists (data); no text of the reference.

    python tools/gen_golden_import.py"""
import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402


def W(text, start, stop):
    return {'text': text, 'start': start, 'stop': stop}


# (name, orig text without the leading blank, TextGrid words, TextGrid phones)
CASES = [
    ('no_leading_pause', 'hello world',
     [W('hello', 0.0, 0.42), W('world', 0.42, 0.9)],
     [W('HH', 0.0, 0.1), W('AH0', 0.1, 0.2), W('L', 0.2, 0.3), W('OW1', 0.3, 0.42), W('W', 0.42, 0.55), W('ER1', 0.55, 0.7), W('L', 0.7, 0.8),
      W('D', 0.8, 0.9)]),
    ('leading_eps', 'good day',
     [W('<eps>', 0.0, 0.25), W('good', 0.25, 0.6), W('day', 0.6, 1.05)],
     [W('sil', 0.0, 0.25), W('G', 0.25, 0.35), W('UH1', 0.35, 0.5), W('D', 0.5, 0.6), W('D', 0.6, 0.75), W('EY1', 0.75, 1.05)]),
    ('punctuation_without_words', 'yes, no!',
     [W('yes', 0.0, 0.4), W('no', 0.5, 0.83)],
     [W('Y', 0.0, 0.1), W('EH1', 0.1, 0.25), W('S', 0.25, 0.4), W('N', 0.5, 0.6), W('OW1', 0.6, 0.83)]),
    ('word_without_phones', 'a b c',
     [W('a', 0.0, 0.2), W('b', 0.2, 0.3), W('c', 0.3, 0.61)],
     [W('EY1', 0.0, 0.2), W('S', 0.3, 0.4), W('IY1', 0.4, 0.61)]),
    ('tokenizer_splits_a_word', 'well-known fact',
     [W('well-known', 0.0, 0.7), W('fact', 0.7, 1.2)],
     [W('W', 0.0, 0.1), W('EH1', 0.1, 0.2), W('L', 0.2, 0.3), W('N', 0.3, 0.45), W('OW1', 0.45, 0.7), W('F', 0.7, 0.8), W('AE1', 0.8, 1.0),
      W('K', 1.0, 1.1), W('T', 1.1, 1.2)]),
    ('trailing_silence', 'stop now.',
     [W('stop', 0.0, 0.5), W('now', 0.5, 0.9), W('', 0.9, 1.37)],
     [W('S', 0.0, 0.1), W('T', 0.1, 0.2), W('AA1', 0.2, 0.4), W('P', 0.4, 0.5), W('N', 0.5, 0.65), W('AW1', 0.65, 0.9), W('sil', 0.9, 1.37)]),
    ('pause_inside_and_unknown_word', 'one, <eps> two zzz',
     [W('', 0.0, 0.1), W('one', 0.1, 0.45), W('<eps>', 0.45, 0.7), W('two', 0.7, 1.0), W('zzz', 1.0, 1.33)],
     [W('', 0.0, 0.1), W('W', 0.1, 0.2), W('AH1', 0.2, 0.3), W('N', 0.3, 0.45), W('sp', 0.45, 0.7), W('T', 0.7, 0.8), W('UW1', 0.8, 1.0),
      W('spn', 1.0, 1.33)]),
]


def main():
    ref_import.setup()
    for name in ('librosa', 'soundfile', 'textgrid', 'pysptk', 'tqdm', 'PIL', 'PIL.Image'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules['PIL'], 'Image'):
        sys.modules['PIL'].Image = sys.modules['PIL.Image']
    spec = importlib.util.spec_from_file_location('ref_import_textgrid', os.path.join(ref_import.REF, 'scripts', 'import_textgrid.py'))
    ref = importlib.util.module_from_spec(spec)
    cwd = os.getcwd()
    os.chdir(ref_import.REF)
    try:
        spec.loader.exec_module(ref)
    finally:
        os.chdir(cwd)
    out = []
    for name, text, words, phones in CASES:
        orig_text = ' ' + text
        words = [dict(w) for w in words]
        if words[0]['text'] not in ('<eps>', ''):
            words.insert(0, W(' ', 0, 0))
        tokens = ref.tokenizer(orig_text)
        hybrid, phon2word, frame2phon = ref._merge(words, phones, tokens)
        out.append({'name': name, 'orig_text': orig_text, 'words': words, 'phones': phones, 'tokens': [t.word for t in tokens],
                    'merged_phones': hybrid, 'phon2word': phon2word, 'frame2phon': frame2phon})
        print(name, len(hybrid), 'phones,', len(frame2phon), 'frames')
    path = os.path.join(ROOT, 'tests', 'golden', 'import_textgrid_merge.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', path)


if __name__ == '__main__':
    main()
