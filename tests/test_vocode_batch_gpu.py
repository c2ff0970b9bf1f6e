"""GPU tests of batched WaveRNN vocoding: ``CubenetVocoder.synthesize_batch`` gives every utterance the bits of ``_inference`` on that
utterance alone (and, without sampling noise, of the oracle chain lr-oracle -> fold -> hr-oracle -> un-fold), whatever the launch size and
the order of the list; scripts/vocode.py writes the same bytes at every --batch; io_utils.vocoder.WaveRNNVocoder keeps the vocoder contract."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import wavernn_ref as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [40, 7, 23, 61, 20]   # T < 20 (nb = T), T no multiple of 20, T = 20 (one-frame chunks)
SEED = 0x5EED0000


@pytest.fixture(params=['tile', 'stream'])
def wr_kernel(request, monkeypatch):
    """both decode kernels: the tile kernel allowed (its default) / the streaming kernel forced (TTSC_WR_TILE=0)"""
    if request.param == 'tile':
        monkeypatch.delenv('TTSC_WR_TILE', raising=False)
    else:
        monkeypatch.setenv('TTSC_WR_TILE', '0')
    monkeypatch.delenv('TTSC_WR_BT', raising=False)
    return request.param


def _state_dicts(output):
    S = O.SAMPLE_SIZE[output]
    return (O.synthetic_state_dict(H=64, num_layers=1, use_lowres=True, seed=21, S=S),
            O.synthetic_state_dict(H=64, num_layers=1, use_lowres=False, seed=22, S=S))


def _vocoder(output):
    from ttscube_amd.networks.vocoder import CubenetVocoder
    voc = CubenetVocoder(num_layers_lr=1, layer_size_lr=64, num_layers_hr=1, layer_size_hr=64, upsample=240, upsample_low=10, output=output)
    sd_hr, sd_lr = _state_dicts(output)
    sd = {'_wavernn_hr.' + k: torch.from_numpy(v) for k, v in sd_hr.items()}
    sd.update({'_wavernn_lr.' + k: torch.from_numpy(v) for k, v in sd_lr.items()})
    voc.load_state_dict(sd, strict=True)
    return voc.cuda().eval()


def _mels():
    rng = np.random.RandomState(77)
    return [np.clip(rng.randn(T, 80) - 2.0, -5.0, 1.0).astype(np.float32) for T in TS]


_ORACLE = {}


def _oracle_chain(i):
    """argmax, mulaw: lr-oracle -> O.inference_batch -> hr-oracle -> O.compose_batched_inference (computed once per utterance)"""
    if i not in _ORACLE:
        sd_hr, sd_lr = _state_dicts('mulaw')
        mel = _mels()[i][None]
        _, r_lr, _ = O.decode(sd_lr, mel, None, num_layers=1, H=64, use_lowres=False, upsample=24, mode=O.MODE_ARGMAX)
        fo = O.inference_batch(mel, r_lr, num_batches=20)
        _, r_hr, _ = O.decode(sd_hr, fo['mel'], fo['x_low'], num_layers=1, H=64, mode=O.MODE_ARGMAX)
        _ORACLE[i] = (r_lr[0], O.compose_batched_inference(r_hr)[0])
    return _ORACLE[i]


@pytest.mark.parametrize('output', ['mulaw', 'mol'])
def test_batch_equals_the_loop(output, wr_kernel):
    voc = _vocoder(output)
    mels = _mels()
    want = 'tile' if wr_kernel == 'tile' else 'stream'
    for mode in ('philox', 'argmax'):
        loop = [voc._inference({'mel': torch.from_numpy(m[None])}, seed=SEED + i, mode=mode) for i, m in enumerate(mels)]
        loop = [(a[0, :, 0], b[0]) for a, b in loop]
        for i, T in enumerate(TS):
            assert loop[i][0].shape == (24 * T,)
        if mode == 'argmax' and output == 'mulaw':
            for i in range(len(TS)):
                r_lr, r_hr = _oracle_chain(i)
                assert np.array_equal(loop[i][0], r_lr) and np.array_equal(loop[i][1], r_hr)
        # one launch; several launches with one utterance's rows split across them (87 rows: 24 + 24 + 24 + 15)
        for max_rows in (None, 24):
            got = voc.synthesize_batch(mels, seed=SEED, mode=mode, max_rows=max_rows)
            assert voc._wavernn_hr.last_kernel == want and voc._wavernn_lr.last_kernel == want
            assert len(voc.last_plan.launches) == (1 if max_rows is None else 4)
            for i in range(len(TS)):
                assert got[i][0].shape == loop[i][0].shape and got[i][1].shape == loop[i][1].shape
                assert np.array_equal(got[i][0], loop[i][0]), (mode, max_rows, i, 'x_lr')
                assert np.array_equal(got[i][1], loop[i][1]), (mode, max_rows, i, 'x_hr')
        # the list permuted, the seeds permuted alike: every utterance keeps its bits
        perm = [3, 0, 4, 2, 1]
        got = voc.synthesize_batch([mels[p] for p in perm], seed=[SEED + p for p in perm], mode=mode)
        for k, p in enumerate(perm):
            assert np.array_equal(got[k][0], loop[p][0]) and np.array_equal(got[k][1], loop[p][1]), (mode, 'permuted', p)


def _save_model(prefix, output='mulaw'):
    import yaml
    voc = _vocoder(output)
    yaml.dump({'num_layers_lr': 1, 'layer_size_lr': 64, 'num_layers_hr': 1, 'layer_size_hr': 64, 'upsample': 240, 'sample_rate': 24000,
               'output': output, 'sample_rate_low': 2400, 'hop_size': 240}, open(prefix + '.yaml', 'w'))
    voc.save(prefix + '.last')
    return voc


def test_vocode_script_same_bytes_at_every_batch(tmp_path):
    prefix = str(tmp_path / 'voc')
    _save_model(prefix)
    feats = tmp_path / 'feats'
    feats.mkdir()
    rng = np.random.RandomState(5)
    for name, T in (('a', 3), ('b', 1), ('c', 2)):
        with open(str(feats / (name + '.mgc')), 'wb') as f:
            np.save(f, np.clip(rng.randn(T, 80) - 2.0, -5.0, 1.0).astype(np.float32))
    outs = {}
    for batch in (1, 3):
        out = tmp_path / ('out%d' % batch)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'vocode.py'), '--model', prefix, '--input', str(feats),
                            '--output-folder', str(out), '--batch', str(batch), '--seed', '11'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[batch] = {n: open(str(out / n), 'rb').read() for n in sorted(os.listdir(str(out)))}
    assert sorted(outs[1]) == ['a.wav', 'b.wav', 'c.wav'] and outs[1] == outs[3]
    import scipy.io.wavfile
    sr, a = scipy.io.wavfile.read(str(tmp_path / 'out3' / 'a.wav'))
    assert sr == 24000 and a.dtype == np.int16 and a.shape == (300,)   # T = 3: three chunks of min(2 * 240, 34 * 10) - 240 samples


def test_wavernn_vocoder_adapter():
    from ttscube_amd.io_utils.vocoder import WaveRNNVocoder
    voc = _vocoder('mulaw')
    mels = _mels()[:3]   # T = 40, 7, 23
    F = max(m.shape[0] for m in mels)
    mel = torch.zeros(3, 80, F)
    for b, m in enumerate(mels):
        mel[b, :, :m.shape[0]] = torch.from_numpy(m.T) * math.log(10.0)
    adapter = WaveRNNVocoder(voc, batch=2, seed=SEED)
    audio = adapter(mel.cuda(), frames=[m.shape[0] for m in mels])
    loop = [voc._inference({'mel': (mel[b, :, :m.shape[0]].t() * (1.0 / math.log(10.0)))[None]}, seed=SEED + b)[1][0]
            for b, m in enumerate(mels)]
    assert adapter.last_lengths == [x.shape[0] for x in loop]
    assert audio.is_cuda and tuple(audio.shape) == (3, 1, max(adapter.last_lengths))
    a = audio.cpu().numpy()
    for b, x in enumerate(loop):
        assert np.array_equal(a[b, 0, :x.shape[0]], np.clip(x, -1.0, 1.0)) and not a[b, 0, x.shape[0]:].any()
    assert tuple(adapter(mel[:1, :, :7].cuda()).shape) == (1, 1, loop[1].shape[0])
