"""GPU: the segment gather (csrc/segment_feed.hip through io_utils/segment_feed.py) against its numpy restatement, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import segment_feed_reference as SR

pytestmark = pytest.mark.gpu

MEL_PAD = math.log(1e-5)
LN10 = math.log(10.0)


@functools.lru_cache(maxsize=None)
def _items(frames, hop, n_mels=80):
    """four utterances: 0 shorter than the segment, 1 with F = L // hop whose crop from frame 3 ends on its last sample, 2 with F = L // hop + 1,
    3 all zero"""
    rng = np.random.RandomState(1000 * frames + hop)
    L = [max(frames * hop // 2, 1), (frames + 3) * hop, (frames + 5) * hop + hop // 2 + 1, frames * hop + 3]
    F = [L[0] // hop, L[1] // hop, L[2] // hop + 1, L[3] // hop]
    audio = [rng.randint(-32768, 32768, size=n).astype(np.int16) for n in L]
    audio[3][:] = 0
    mels = [(rng.randn(f, n_mels) - 2).astype(np.float32) for f in F]
    return tuple(zip(audio, mels))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _batches(items, frames):
    F2 = items[2][1].shape[0]
    return [([0, 1, 2], [0, 3, 0]), ([3, 2, 1], [0, max(F2 - frames, 0), 1])]


@pytest.mark.parametrize('hop', [240, 5])
@pytest.mark.parametrize('frames', [1, 7, 50])
def test_gather_matches_the_restatement_bit_for_bit(frames, hop):
    from ttscube_amd.io_utils.segment_feed import SegmentCorpus, build_tables
    items = _items(frames, hop)
    t = build_tables(items, hop, 80)
    corpus = SegmentCorpus(items, hop, 80, 'cuda:0')
    assert corpus.n_frames.tolist() == [m.shape[0] for _, m in items]
    for utt, start in _batches(items, frames):
        for scale in (LN10, 1.0):
            y, mel = corpus.gather(utt, start, frames, mel_scale=scale)
            y0, mel0 = SR.gather(t['wav'], t['wav_off'], t['gain'], t['mel'], t['mel_off'], utt, start, frames, hop, scale, MEL_PAD)
            y, mel = y.cpu().numpy(), mel.cpu().numpy()
            assert _same(y, y0) and _same(mel, mel0)
            assert np.isfinite(y).all() and np.isfinite(mel).all()
        # the audio-only call
        ya, none = corpus.gather(utt, start, frames, with_mel=False)
        assert none is None and _same(ya.cpu().numpy(), y0)
        # every row alone has the bits it has inside the batch
        for b in range(len(utt)):
            y1, m1 = corpus.gather(utt[b:b + 1], start[b:b + 1], frames, mel_scale=1.0)
            assert _same(y1.cpu().numpy(), y0[b:b + 1]) and _same(m1.cpu().numpy(), mel0[b:b + 1])
    # the cases the corpus was built for
    y0, mel0 = SR.gather(t['wav'], t['wav_off'], t['gain'], t['mel'], t['mel_off'], [0, 1, 2, 3], [0, 3, 0, 0], frames, hop, 1.0, MEL_PAD)
    L0, F0 = items[0][0].shape[0], items[0][1].shape[0]
    assert not y0[0, 0, L0:].any() and np.all(mel0[0, :, F0:] == np.float32(MEL_PAD)) and F0 < frames
    assert y0[1, 0, -1] == np.float32(items[1][0][-1]) * t['gain'][1] and t['wav_off'][1] + 3 * hop + frames * hop == t['wav_off'][1] + t['length'][1]
    assert t['gain'][3] == 0 and not y0[3].any()


@pytest.mark.parametrize('frames,hop,n_mels', [(7, 240, 80), (50, 5, 80), (70, 5, 80), (9, 3, 5)])
def test_unaligned_arenas_take_the_narrow_paths_with_the_same_bits(frames, hop, n_mels):
    """packed tables (no utterance starts on a multiple of 8) in arenas that start one element behind a 16-byte boundary; frames = 70 needs a second mel
    tile, n_mels = 5 an odd tile pitch"""
    from ttscube_amd.io_utils.segment_feed import segment_gather
    items = _items(frames, hop, n_mels)
    length = np.array([a.shape[0] for a, _ in items], np.int64)
    wav_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    mel_off = np.concatenate([[0], np.cumsum([m.shape[0] for _, m in items])]).astype(np.int64)
    wav = np.concatenate([a for a, _ in items])
    mel = np.concatenate([m for _, m in items]).astype(np.float32)
    gain = np.array([0.95 / max(int(np.abs(a.astype(np.int32)).max()), 1) if a.any() else 0.0 for a, _ in items], np.float32)
    dev = 'cuda:0'
    wav_d = torch.zeros(wav.shape[0] + 1, dtype=torch.int16, device=dev)[1:]
    wav_d.copy_(torch.from_numpy(wav))
    mel_d = torch.zeros(mel.size + 1, dtype=torch.float32, device=dev)[1:].view(mel.shape)
    mel_d.copy_(torch.from_numpy(mel))
    assert wav_d.data_ptr() % 16 == 2 and mel_d.data_ptr() % 16 == 4
    up = lambda a: torch.from_numpy(a).to(dev)
    for utt, start in _batches(items, frames):
        idx = up(np.array([utt, start], np.int32))
        y, m = segment_gather(wav_d, up(wav_off), up(gain), mel_d, up(mel_off), idx[0], idx[1], frames, hop, n_mels, LN10, MEL_PAD)
        y0, m0 = SR.gather(wav, wav_off, gain, mel, mel_off, utt, start, frames, hop, LN10, MEL_PAD)
        assert _same(y.cpu().numpy(), y0) and _same(m.cpu().numpy(), m0)


def test_gather_refuses_what_it_cannot_run():
    from ttscube_amd._lib import TTSCError
    from ttscube_amd.io_utils.segment_feed import SegmentCorpus
    items = _items(7, 5)
    corpus = SegmentCorpus(items, 5, 80, 'cuda:0')
    with pytest.raises(TTSCError):
        corpus.gather([4], [0], 7)
    with pytest.raises(TTSCError):
        corpus.gather([0], [-1], 7)
    with pytest.raises(TTSCError):
        SegmentCorpus([(a, None) for a, _ in items], 5, 80, 'cuda:0').gather([0], [0], 7, with_mel=True)
    with pytest.raises(TTSCError):
        SegmentCorpus(items, 5, 80, 'cpu')
