"""CPU: the host side of the HiFi-GAN trainer (ttscube_amd/hifigan/train.py, io_utils/segment_feed.py) — sampler, corpus tables, file lists,
checkpoint scan and the public checkpoint layout.  No compute calls into the extension."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import hifigan_ref as R
from tests import segment_feed_reference as SR


def _frames(seed=0, U=23):
    return np.random.RandomState(seed).randint(1, 200, size=U)


def test_sampler_is_a_function_of_seed_and_epoch_alone():
    from ttscube_amd.io_utils.segment_feed import epoch_plan
    nf = _frames()
    p0, s0 = epoch_plan(1234, 3, nf, 50)
    np.random.seed(99)                    # the global generator plays no part
    np.random.rand(17)
    p1, s1 = epoch_plan(1234, 3, nf, 50)
    assert np.array_equal(p0, p1) and np.array_equal(s0, s1)
    assert sorted(p0.tolist()) == list(range(nf.shape[0]))
    p2, s2 = epoch_plan(1234, 4, nf, 50)
    p3, s3 = epoch_plan(1235, 3, nf, 50)
    assert not np.array_equal(p0, p2) and not np.array_equal(p0, p3)
    assert not np.array_equal(s0, s2) and not np.array_equal(s0, s3)


@pytest.mark.parametrize('frames', [1, 7, 50, 500])
def test_sampler_starts_stay_inside_the_utterance(frames):
    from ttscube_amd.io_utils.segment_feed import epoch_plan
    nf = np.concatenate([_frames(1, 400), [frames, frames + 1, frames - 1 if frames > 1 else 1]])
    seen_last = False
    for epoch in range(20):
        _, start = epoch_plan(7, epoch, nf, frames)
        room = np.maximum(nf - frames, 0)
        assert np.all(start >= 0) and np.all(start <= room)
        assert np.all(start[room == 0] == 0)
        seen_last |= bool(np.any((start == room - 1) & (room > 1)))
    assert seen_last or frames == 500      # the draw reaches the end of the range it is meant to cover


def test_resumed_epoch_draws_the_tail_of_the_uninterrupted_one():
    from ttscube_amd.io_utils.segment_feed import epoch_batches
    nf = _frames(2, 23)
    whole = list(epoch_batches(5, 2, nf, 50, 4))
    assert len(whole) == 23 // 4 and all(u.shape == (4,) and s.shape == (4,) for u, s in whole)
    for first in (0, 1, 3, 5):
        tail = list(epoch_batches(5, 2, nf, 50, 4, first=first))
        assert len(tail) == len(whole) - first
        for (u0, s0), (u1, s1) in zip(whole[first:], tail):
            assert np.array_equal(u0, u1) and np.array_equal(s0, s1)


def test_corpus_tables_and_gain():
    from ttscube_amd.io_utils.segment_feed import ALIGN, build_tables, utterance_gain
    rng = np.random.RandomState(3)
    audio = [rng.randint(-20000, 20000, size=n).astype(np.int16) for n in (1201, 960, 17)] + [np.zeros((300,), np.int16)]
    audio[1][5] = -32768
    mels = [rng.randn(n, 80).astype(np.float32) for n in (6, 4, 1, 2)]
    t = build_tables(list(zip(audio, mels)), hop=240, n_mels=80)
    assert np.all(t['wav_off'] % ALIGN == 0) and t['wav_off'][0] == 0 and t['mel_off'].tolist() == [0, 6, 10, 11, 13]
    assert t['n_frames'].tolist() == [6, 4, 1, 2] and t['length'].tolist() == [1201, 960, 17, 300]
    for u, a in enumerate(audio):
        got = t['wav'][t['wav_off'][u]:t['wav_off'][u + 1]]
        assert np.array_equal(got[:a.shape[0]], a) and not got[a.shape[0]:].any()
        assert np.array_equal(t['mel'][t['mel_off'][u]:t['mel_off'][u + 1]], mels[u])
    assert t['gain'].dtype == np.float32
    assert t['gain'][1] == np.float32(0.95 / 32768) and t['gain'][3] == 0 and utterance_gain(np.zeros((0,), np.int16)) == 0
    assert t['gain'][0] == np.float32(0.95 / np.abs(audio[0].astype(np.int32)).max())
    # without mels the frame count is L // hop
    t2 = build_tables([(a, None) for a in audio], hop=240)
    assert t2['mel'] is None and t2['n_frames'].tolist() == [5, 4, 0, 1]
    with pytest.raises(ValueError):
        build_tables([(audio[0], mels[0]), (audio[1], None)])
    # the restatement over these tables: the loudest sample lands on -0.95 exactly once rounded, tails are zero / mel_pad
    y, m = SR.gather(t['wav'], t['wav_off'], t['gain'], t['mel'], t['mel_off'], [1, 3], [0, 1], 5, 240, 1.0, -11.5)
    assert y.shape == (2, 1, 1200) and m.shape == (2, 80, 5)
    assert y[0, 0, 5] == np.float32(-32768) * np.float32(0.95 / 32768) and not y[0, 0, 960:].any() and not y[1].any()
    assert np.array_equal(m[0, :, :4], mels[1].T) and np.all(m[0, :, 4] == np.float32(-11.5))
    assert np.array_equal(m[1, :, 0], mels[3][1]) and np.all(m[1, :, 1:] == np.float32(-11.5))


def test_file_lists_and_processed_folder_discovery(tmp_path):
    from ttscube_amd.hifigan.train import discover_processed, parse_filelist
    lst = tmp_path / 'training.txt'
    lst.write_text('LJ001-0001|Printing, in the only sense|Printing\n\nLJ001-0002|with a | in the text\nplain_name\n', encoding='utf-8')
    assert parse_filelist(str(lst)) == ['LJ001-0001', 'LJ001-0002', 'plain_name']
    for part, ids in (('train', ['b', 'a', 'c']), ('dev', ['z'])):
        os.makedirs(tmp_path / 'processed' / part)
        for i in ids:
            (tmp_path / 'processed' / part / (i + '.wav')).write_bytes(b'')
    (tmp_path / 'processed' / 'train' / 'a.mgc').write_bytes(b'')
    (tmp_path / 'processed' / 'train' / 'notes.txt').write_bytes(b'')
    tr, dv = discover_processed(str(tmp_path / 'processed'))
    assert [i for i, _ in tr] == ['a', 'b', 'c'] and [i for i, _ in dv] == ['z']
    assert tr[0][1] == str(tmp_path / 'processed' / 'train' / 'a.wav')
    tr, dv = discover_processed(str(tmp_path / 'processed'), need_mgc=True)
    assert [i for i, _ in tr] == ['a'] and dv == []
    with pytest.raises(FileNotFoundError):
        discover_processed(str(tmp_path / 'nothing'))


def test_checkpoint_scan_picks_the_latest_complete_pair(tmp_path):
    from ttscube_amd.hifigan.train import scan_checkpoints
    assert scan_checkpoints(str(tmp_path)) is None
    for name in ('g_00000003', 'do_00000003', 'g_00000010', 'do_00000010', 'g_00000020', 'do_00000015', 'g_latest', 'config.json', 'g_0000001'):
        (tmp_path / name).write_bytes(b'')
    steps, g, do = scan_checkpoints(str(tmp_path))
    assert steps == 10 and g == str(tmp_path / 'g_00000010') and do == str(tmp_path / 'do_00000010')
    os.remove(tmp_path / 'do_00000010')
    assert scan_checkpoints(str(tmp_path))[0] == 3
    os.remove(tmp_path / 'do_00000003')
    assert scan_checkpoints(str(tmp_path)) is None          # generator files alone are no pair to resume from


def test_generator_file_loads_through_the_unchanged_loader(tmp_path):
    from ttscube_amd.hifigan.env import AttrDict
    from ttscube_amd.hifigan.models import Generator
    from ttscube_amd.hifigan.train import save_generator
    from ttscube_amd.io_utils.runtime import load_generator_checkpoint
    h = dict(R.CONFIG_V1, upsample_initial_channel=32)
    sd = R.synthetic_state_dict(h, seed=11)
    assert any(k.endswith('weight_g') for k in sd) and any(k.endswith('weight_v') for k in sd)
    g = Generator(AttrDict(h))
    g.load_state_dict(sd)
    json.dump(h, open(tmp_path / 'config.json', 'w'))
    save_generator(str(tmp_path / 'g_00000007'), g)
    raw = torch.load(str(tmp_path / 'g_00000007'), map_location='cpu')
    assert list(raw) == ['generator'] and set(raw['generator']) == set(sd)
    assert all(torch.equal(raw['generator'][k], sd[k]) for k in sd)
    v = load_generator_checkpoint(str(tmp_path / 'g_00000007'))
    assert not v.training and hasattr(v.conv_pre, 'weight') and not hasattr(v.conv_pre, 'weight_g')
    want = R.fold_state_dict(sd)['conv_pre.weight'] if 'conv_pre.weight' in R.fold_state_dict(sd) else None
    if want is not None:
        assert torch.allclose(v.conv_pre.weight.detach(), want, rtol=1e-6, atol=1e-7)


def test_learning_rate_is_a_function_of_the_epoch():
    from ttscube_amd.hifigan.train import epoch_lr, loss_fmax
    h = {'learning_rate': 2e-4, 'lr_decay': 0.999, 'sampling_rate': 24000, 'fmax_for_loss': None}
    assert epoch_lr(h, 0) == 2e-4 and epoch_lr(h, 3) == 2e-4 * 0.999 ** 3
    assert loss_fmax(h) == 12000 and loss_fmax(dict(h, fmax_for_loss=8000)) == 8000


def test_library_exports_the_gather():
    from ttscube_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_lib.lib(), 'ttsc_segment_gather') and 'ttsc_segment_gather' in _lib.SIGNATURES
