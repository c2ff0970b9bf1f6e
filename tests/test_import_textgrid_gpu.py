"""GPU: scripts/import_textgrid.py end to end — three synthetic wav + TextGrid pairs become a processed corpus the Cubegan and Textcoder readers
accept, and the batch size does not change a byte of it."""
import filecmp
import importlib.util
import json
import os

import numpy as np
import pytest
import scipy.io.wavfile

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

SR, HOP = 24000, 240
# (name, seconds, F0, words with phones, text); both tiers span the whole file, silences included, as the aligner writes them
UTTS = [
    ('utt_a', 1.23, 110.0, [('', ['']), ('hello', ['HH', 'AH0', 'L', 'OW1']), ('world', ['W', 'ER1', 'L', 'D']), ('', [''])], 'Hello, world!'),
    ('utt_b', 0.91, 180.0, [('yes', ['Y', 'EH1', 'S']), ('no', ['N', 'OW1'])], 'Yes no'),
    ('utt_c', 1.5, 140.0, [('<eps>', ['sil']), ('stop', ['S', 'T', 'AA1', 'P']), ('now', ['N', 'AW1']), ('', [''])], 'stop now.'),
]


def _textgrid(dur, words, text):
    """long-format TextGrid: words share the duration evenly, a word's phones share the word"""
    def tier(name, items):
        out = ['    item []:', '        class = "IntervalTier"', '        name = "%s"' % name, '        xmin = 0', '        xmax = %r' % dur,
               '        intervals: size = %d' % len(items)]
        for i, (a, b, mark) in enumerate(items):
            out += ['        intervals [%d]:' % (i + 1), '            xmin = %r' % a, '            xmax = %r' % b, '            text = "%s"' % mark]
        return out
    edges = [round(dur * i / len(words), 3) for i in range(len(words))] + [dur]
    wi = [(edges[i], edges[i + 1], w) for i, (w, _) in enumerate(words)]
    pi = []
    for (a, b, _), (_, phones) in zip(wi, words):
        for j, ph in enumerate(phones):
            pi.append((round(a + (b - a) * j / len(phones), 3), round(a + (b - a) * (j + 1) / len(phones), 3) if j + 1 < len(phones) else b, ph))
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', '', 'xmin = 0', 'xmax = %r' % dur, 'tiers? <exists>', 'size = 3', 'item []:']
    lines += tier('words', wi) + tier('phones', pi) + tier('text', [(0, dur, text)])
    return '\n'.join(lines) + '\n'


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp('import')
    src = root / 'aligned'
    src.mkdir()
    for k, (name, dur, f0, words, text) in enumerate(UTTS):
        t = np.arange(int(round(dur * SR))) / SR
        x = 0.4 * sum(np.sin(2 * np.pi * h * f0 * t) / h for h in range(1, 7)) * np.minimum(1.0, 8.0 * t)
        scipy.io.wavfile.write(str(src / (name + '.wav')), SR, np.asarray(x / np.abs(x).max() * 0.5 * 32767, dtype=np.int16))
        (src / (name + '.TextGrid')).write_text(_textgrid(dur, words, text), encoding='utf-8')
    spec = importlib.util.spec_from_file_location('import_textgrid_script', os.path.join(ROOT, 'scripts', 'import_textgrid.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    outs = {}
    for batch in (1, 3):
        outs[batch] = root / ('out_b%d' % batch)
        rc = script.main(['--input-folder', str(src), '--output-folder', str(outs[batch]), '--dev-ratio', '0.34', '--speaker', 'anna', '--prefix',
                          'SYN', '--batch', str(batch)])
        assert rc == 0
    return src, outs


def test_round_trip_into_the_dataset_readers(corpus):
    from ttscube_amd.io_utils.io_cubegan import CubeganCollate, CubeganDataset, CubeganEncodings
    from ttscube_amd.io_utils.io_textcoder import TextcoderDataset
    src, outs = corpus
    train, dev = str(outs[3] / 'train'), str(outs[3] / 'dev')
    assert sorted(os.listdir(train)) == ['SYN_%08d.%s' % (i, e) for i in range(2) for e in ('json', 'mgc', 'pitch', 'wav')]
    assert sorted(os.listdir(dev)) == ['SYN_00000000.%s' % e for e in ('json', 'mgc', 'pitch', 'wav')]
    ds, tds = CubeganDataset(train), TextcoderDataset(train)
    assert len(ds) == 2 and len(tds) == 2 and len(CubeganDataset(dev)) == 1
    by_name = {u[0]: u for u in UTTS}
    for i in range(len(ds)):
        ex = ds[i]
        meta = ex['meta']
        name, dur = meta['orig_filename'], by_name[meta['orig_filename']][1]
        assert name in ('utt_a', 'utt_c') and meta['speaker'] == 'anna' and meta['id'] == 'SYN_%08d' % i
        assert len(meta['frame2phon']) == int(dur * 100) and max(meta['frame2phon']) < len(meta['phones'])
        L = int(len(meta['frame2phon']) * 10 * SR / 1000)
        rate, wav = scipy.io.wavfile.read(os.path.join(train, meta['id'] + '.wav'))
        assert rate == SR and wav.dtype == np.int16 and wav.shape[0] == L
        assert abs(int(np.abs(wav.astype(np.int32)).max()) - 0.98 * 32767) <= 1
        assert ex['mgc'].shape == (1 + L // HOP, 80) and ex['mgc'].dtype == np.float32
        assert ex['pitch'].shape == (L // HOP,)
        assert tds[i]['mgc'].shape == ex['mgc'].shape and tds[i]['pitch'].shape == ex['pitch'].shape
        raw = np.load(open(os.path.join(train, meta['id'] + '.pitch'), 'rb'))
        voiced = raw[raw > 0]
        rel = np.abs(voiced - by_name[name][2]) / by_name[name][2]          # (a steady harmonic tone from end to end)
        assert voiced.size > 0.5 * raw.size and np.median(rel) < 0.02 and np.mean(rel < 0.03) >= 0.9
        assert json.load(open(os.path.join(train, meta['id'] + '.json')))['words'] == meta['words']
    enc = CubeganEncodings()
    enc.compute(ds.meta_items())
    assert 0 < enc.max_pitch <= 400 and 'anna' in enc.speaker2int and 'HH' in enc.phon2int
    batch = CubeganCollate(enc).collate_fn([ds[0], ds[1]])
    assert batch['y_pitch'].shape == batch['y_mgc'].shape[:2] and batch['y_pitch'].max() > 0
    assert batch['y_audio'].shape[1] == batch['y_mgc'].shape[1] * HOP


def test_batch_size_does_not_change_a_byte(corpus):
    _, outs = corpus
    for part in ('train', 'dev'):
        names = sorted(os.listdir(str(outs[1] / part)))
        assert names == sorted(os.listdir(str(outs[3] / part))) and names
        match, mismatch, errors = filecmp.cmpfiles(str(outs[1] / part), str(outs[3] / part), names, shallow=False)
        assert not mismatch and not errors, (mismatch, errors)
