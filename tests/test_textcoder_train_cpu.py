"""CPU: CubenetTextcoder training's data side and trainer CLI — TextcoderCollate against the reference's own collate output
(tests/golden/textcoder_collate.npz, tools/gen_golden_textcoder_train.py), TextcoderEncodings round trip, TextcoderDataset's file rule,
train_textcoder.py's argument parsing and its single-process guard."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from tests.conftest import ROOT


def _examples(z):
    metas = json.loads(str(z['ex_meta']))
    out, o = [], 0
    for meta, n in zip(metas, z['ex_len']):
        n = int(n)
        out.append({'meta': meta, 'mgc': z['ex_mgc'][o:o + n], 'pitch': z['ex_pitch'][o:o + n]})
        o += n
    return out


def test_collate_matches_the_reference():
    from ttscube_amd.io_utils.io_textcoder import TextcoderCollate, TextcoderEncodings
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'textcoder_collate.npz'))
    enc = TextcoderEncodings()
    for k, v in json.loads(str(z['enc'])).items():
        setattr(enc, k, v)
    b = TextcoderCollate(enc).collate_fn(_examples(z))
    for k in ('x_char', 'x_speaker', 'y_mgc', 'y_pitch', 'y_dur'):
        ref = z['out_' + k]
        assert b[k].dtype == torch.from_numpy(ref).dtype, k
        assert b[k].shape == ref.shape and np.array_equal(b[k].numpy(), ref), k
    assert b['y_frame2phone'] == json.loads(str(z['out_f2p']))
    assert int(b['x_char'][0, 0]) == 0       # an unknown phoneme stays 0


def test_encodings_round_trip(tmp_path):
    from ttscube_amd.io_utils.io_textcoder import TextcoderEncodings
    from ttscube_amd.io_utils.synthetic import synthetic_examples
    enc = TextcoderEncodings()
    enc.compute(list(synthetic_examples(4, 11)))
    assert enc.phon2int and enc.speaker2int and enc.max_duration > 0 and enc.max_pitch > 0
    enc.save(str(tmp_path / 'x.encodings'))
    blob = json.load(open(str(tmp_path / 'x.encodings')))
    assert sorted(blob) == ['max_duration', 'max_pitch', 'phon2int', 'speaker2int']
    back = TextcoderEncodings()
    back.load(str(tmp_path / 'x.encodings'))
    assert back.phon2int == enc.phon2int and back.speaker2int == enc.speaker2int
    assert back.max_duration == int(enc.max_duration) and back.max_pitch == int(enc.max_pitch)


def test_dataset_needs_json_mgc_and_pitch_only(tmp_path):
    from ttscube_amd.io_utils.io_textcoder import TextcoderDataset
    for i, with_pitch in ((0, True), (1, False), (2, True)):
        meta = {'id': 'u%d' % i, 'phones': ['a', 'b'], 'speaker': 's', 'frame2phon': [0, 0, 1]}
        json.dump(meta, open(str(tmp_path / ('u%d.json' % i)), 'w'))
        np.save(open(str(tmp_path / ('u%d.mgc' % i)), 'wb'), np.zeros((3, 80), dtype=np.float32) + i)
        if with_pitch:
            np.save(open(str(tmp_path / ('u%d.pitch' % i)), 'wb'), np.full(3, 100.0 + i))
    ds = TextcoderDataset(str(tmp_path))
    assert len(ds) == 2                       # u1 has no .pitch; no .wav is needed by anyone
    ids = sorted(ds[k]['meta']['id'] for k in range(len(ds)))
    assert ids == ['u0', 'u2']
    it = ds[1]
    assert set(it) == {'meta', 'mgc', 'pitch'} and it['mgc'].shape == (3, 80) and float(it['pitch'][0]) == 102.0


def _script(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train_textcoder.py')] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=120)


def test_trainer_help_and_flags():
    r = _script(['--help'])
    assert r.returncode == 0, r.stderr
    for flag in ('--output-base', '--batch-size', '--train-folder', '--dev-folder', '--pframes', '--lr', '--resume', '--synthetic', '--epochs',
                 '--vocoder', '--epoch-generation', '--sample-rate', '--hop-size'):
        assert flag in r.stdout, flag
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import train_textcoder
    finally:
        sys.path.pop(0)
    a = train_textcoder.parser().parse_args(['--synthetic', '8', '--epochs', '2', '--resume', '--vocoder', 'g_1'])
    assert a.synthetic == 8 and a.epochs == 2 and a.resume and a.vocoder == 'g_1' and a.pframes == 3 and a.lr == 2e-4
    assert train_textcoder.parser().parse_args([]).vocoder is None


def test_trainer_refuses_more_than_one_process(tmp_path):
    r = _script(['--synthetic', '4', '--output-base', str(tmp_path / 'tc')], env={'WORLD_SIZE': '2'})
    assert r.returncode != 0
    assert 'WORLD_SIZE=2' in (r.stderr + r.stdout) and 'multi-GPU' in (r.stderr + r.stdout)
    assert not os.path.exists(str(tmp_path / 'tc.yaml'))
