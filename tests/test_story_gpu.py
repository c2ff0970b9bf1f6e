"""GPU: the timeline mixer (csrc/story.hip through io_utils/story_mix.py) against the restatement of the reference's loop (tests/story_reference.py,
bit for bit throughout), and StoryCube end to end against the single-sentence call.

The layout of the first case: the issue's five lengths 1, 7, 8, 9, 4099 plus one segment of length 0 (six segments: the list of five has no empty
one).  Segments 0 and 1 are adjacent (no gap), the empty segment shares its position with the start of the next one, the boundaries 3 | 4 | 11 fall
into the thread run 0..7 .. 8..15 and 21 | 22 into the run 16..23, the track (4143 samples) spans three workgroups and ends inside a run."""
import warnings

import numpy as np
import pytest
import torch

from tests import story_reference as SR

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LENGTHS = [1, 7, 0, 8, 9, 4099]
SEG_DST = [3, 4, 13, 13, 22, 37]
SEG_SRC = [4105, 4110, 4120, 4121, 4131, 2]        # not ascending; the gaps of the packed buffer hold NaN
PACKED = 4145
TOTAL = 4143


def _case(M, seed=7):
    rng = np.random.default_rng(seed)
    assert TOTAL % 8 != 0 and TOTAL == SEG_DST[-1] + LENGTHS[-1] + 7
    packed = np.full(PACKED, np.nan, dtype=np.float32)
    waves = []
    for s, n in zip(SEG_SRC, LENGTHS):
        w = rng.uniform(-0.69, 0.69, size=n).astype(np.float32)
        assert np.isnan(packed[s:s + n]).all()                     # segments do not share elements
        packed[s:s + n] = w
        waves.append(w)
    assert np.isnan(packed).sum() == PACKED - sum(LENGTHS) > 0
    music = rng.uniform(-1.0, 1.0, size=M).astype(np.float32)
    music[0] = 1.0
    music[-1] = -1.0 if M > 1 else 1.0
    return packed, [SR.speech_to_i16(w) for w in waves], music


def _mix(packed, music, total, seg=(SEG_SRC, LENGTHS, SEG_DST), **kw):
    from ttscube_amd.io_utils.story_mix import mix_timeline
    return mix_timeline(torch.from_numpy(packed).to(DEV), seg[0], seg[1], seg[2], torch.from_numpy(music).to(DEV), total, **kw)


@pytest.mark.parametrize('M', [1, 3, 8, 977, TOTAL + 5])
def test_bits_against_the_reference_formula(M):
    packed, segs, music = _case(M)
    want, want_clipped = SR.mix_vectorised(segs, SEG_DST, music, TOTAL)
    assert want_clipped == 0                                        # |w| <= 0.69, |music| <= 1: the reference itself stays inside int16
    out, clipped = _mix(packed, music, TOTAL, return_clipped=True)
    assert out.dtype == torch.int16 and out.shape == (TOTAL,) and out.is_cuda
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (M, bad[:8], got[bad[:8]], want[bad[:8]])
    assert int(clipped.item()) == 0
    # device tables go to the kernel as they are: same bytes
    tables = [torch.tensor(t, dtype=torch.int64, device=DEV) for t in (SEG_SRC, LENGTHS, SEG_DST)]
    assert np.array_equal(_mix(packed, music, TOTAL, seg=tables).cpu().numpy(), want)


def test_rounding_variants_are_told_apart():
    rng = np.random.default_rng(11)
    n, M, lead = 200000, 65537, 5
    w = rng.uniform(-0.69, 0.69, size=n).astype(np.float32)
    music = rng.uniform(-1.0, 1.0, size=M).astype(np.float32)
    segs, dst, total = [SR.speech_to_i16(w)], [lead], n + lead + 6
    want, c = SR.mix_vectorised(segs, dst, music, total)
    assert c == 0
    d64 = int(np.count_nonzero(SR.mix_float64(segs, dst, music, total) != want))
    dfma = int(np.count_nonzero(SR.mix_fused(segs, dst, music, total) != want))
    print('of %d samples: float64 evaluation differs on %d, fused second step on %d' % (total, d64, dfma))
    assert d64 > 0 and dfma > 0          # a kernel doing either cannot pass the next assertion
    got = _mix(w, music, total, seg=([0], [n], dst)).cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def test_chunked_ranges_and_64_bit_phase():
    packed, segs, music = _case(977)
    whole = _mix(packed, music, TOTAL).cpu().numpy()
    assert np.array_equal(whole, SR.mix_vectorised(segs, SEG_DST, music, TOTAL)[0])
    pieces = [_mix(packed, music, TOTAL, t0=a, n=b - a).cpu().numpy() for a, b in ((0, 13), (13, 14), (14, TOTAL))]
    assert [len(p) for p in pieces] == [13, 1, TOTAL - 14]
    assert np.array_equal(np.concatenate(pieces), whole)
    # an output that is not 16-byte aligned takes the kernel's sample-by-sample stores: same bytes, neighbours untouched
    buf = torch.full((TOTAL + 2,), 12345, dtype=torch.int16, device=DEV)
    assert buf[1:].data_ptr() % 16 != 0
    _mix(packed, music, TOTAL, out=buf[1:TOTAL + 1])
    host = buf.cpu().numpy()
    assert host[0] == 12345 and host[-1] == 12345 and np.array_equal(host[1:-1], whole)
    # the music phase and the segment offsets past 2^32: a music bed alone ...
    t0, n = 2 ** 33 + 5, 4099
    total = t0 + n + 3
    bed = _mix(np.zeros(1, np.float32), music, total, seg=([], [], []), t0=t0, n=n).cpu().numpy()
    phase = [(t0 + j) % 977 for j in range(n)]                      # Python integers
    want_bed = np.trunc((music[phase] * np.float32(0.30)) * np.float32(32700.0)).astype(np.int16)
    assert np.array_equal(bed, want_bed)
    assert np.array_equal(bed, SR.mix_vectorised([], [], music, total, t0=t0, n=n)[0])
    # ... and one segment placed at 2^33 + 100 in that range
    rng = np.random.default_rng(5)
    w = rng.uniform(-0.69, 0.69, size=3000).astype(np.float32)
    dst = [2 ** 33 + 100]
    got = _mix(w, music, total, seg=([0], [3000], dst), t0=t0, n=n).cpu().numpy()
    want, c = SR.mix_vectorised([SR.speech_to_i16(w)], dst, music, total, t0=t0, n=n)
    assert c == 0 and np.array_equal(got, want)
    assert np.array_equal(got[:95], bed[:95]) and np.array_equal(got[3095:], bed[3095:]) and not np.array_equal(got[95:3095], bed[95:3095])


def test_saturation_is_counted_and_accumulates():
    rng = np.random.default_rng(3)
    n, M = 5000, 977
    w = (np.float32(0.99997) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    music = rng.choice([-1.0, 1.0], size=M).astype(np.float32)
    segs, dst, total = [SR.speech_to_i16(w)], [17], n + 40
    want, count = SR.mix_vectorised(segs, dst, music, total)
    assert count > 0 and want.max() == 32767 and want.min() == -32768
    out, clipped = _mix(w, music, total, seg=([0], [n], dst), return_clipped=True)
    assert np.array_equal(out.cpu().numpy(), want)
    assert int(clipped.item()) == count
    out2, clipped2 = _mix(w, music, total, seg=([0], [n], dst), return_clipped=True, clipped=clipped)
    assert clipped2 is clipped and int(clipped.item()) == 2 * count and np.array_equal(out2.cpu().numpy(), want)


def test_bad_arguments_are_refused_before_any_launch():
    from ttscube_amd._lib import TTSCError
    packed, _, music = _case(8)
    out = torch.full((TOTAL,), 12345, dtype=torch.int16, device=DEV)
    with pytest.raises(TTSCError, match='M=0'):
        _mix(packed, np.zeros(0, np.float32), TOTAL, out=out)
    lens = list(LENGTHS)
    lens[1] = -1
    with pytest.raises(TTSCError, match='negative length'):
        _mix(packed, music, TOTAL, seg=(SEG_SRC, lens, SEG_DST), out=out)
    dst = list(SEG_DST)
    dst[4] = 20                                                     # inside segment 3 = [13, 21)
    with pytest.raises(TTSCError, match='non-overlapping'):
        _mix(packed, music, TOTAL, seg=(SEG_SRC, LENGTHS, dst), out=out)
    torch.cuda.synchronize()
    assert bool((out == 12345).all())


def test_mix_is_deterministic():
    packed, _, music = _case(977)
    a, ca = _mix(packed, music, TOTAL, return_clipped=True)
    b, cb = _mix(packed, music, TOTAL, return_clipped=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)


def test_storycube_end_to_end(tmp_path):
    from tests.test_api_gpu import _make_model_dir
    from ttscube_amd.api import TTSCube
    from ttscube_amd.io_utils.audio import load_wav, save_wav
    from ttscube_amd.story import StoryCube
    base, _, _ = _make_model_dir(tmp_path)
    tts = TTSCube(base, None)
    rng = np.random.default_rng(9)
    music = rng.uniform(-0.5, 0.5, size=5003).astype(np.float32)
    text = 'a b c | d e f g | h a\n\nk\n\ne f g h i j | a b | c d'
    parts = text.split('\n\n')
    assert len(parts) == 3 and len(parts[1].split()) == 1
    solo = [tts(part, speaker='s1') for part in parts]              # the existing single-sentence call
    lengths = [len(a) for a in solo]
    offsets, total, meta = SR.timeline_literal(lengths, parts)
    want, count = SR.mix_vectorised(solo, offsets, music, total)

    def same(result, want):
        assert set(result) == {'audio', 'meta'}
        assert result['audio'].dtype == np.int16 and result['audio'].shape == (total,)
        assert np.array_equal(result['audio'], want)
        assert result['meta'] == meta and all(type(m['start']) is float and type(m['end']) is float for m in result['meta'][2:])

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        story = StoryCube(None, cube=tts, music=music)
        first = story(text, speaker='s1')
        same(first, want)
        again = story(text, speaker='s1')
        assert again['audio'].tobytes() == first['audio'].tobytes() and again['meta'] == first['meta']
        # saturated samples are reported through a warning, never in meta
        assert (count > 0) == any('saturated' in str(w.message) for w in caught)
        # one paragraph per padded batch (the pipelined path): the same bytes
        same(StoryCube(None, cube=tts, music=music, max_batch=1)(text, speaker='s1'), want)
        # music from a 24 kHz file, given per call: no rate change involved
        path = str(tmp_path / 'bed.wav')
        save_wav(path, rng.uniform(-0.5, 0.5, size=3001).astype(np.float32), 24000)
        bed, rate = load_wav(path, 24000)
        assert rate == 24000 and bed.dtype == np.float32 and bed.shape == (3001,)
        want_bed, _ = SR.mix_vectorised(solo, offsets, bed, total)
        same(story(text, speaker='s1', background_music_path=path), want_bed)
        same(StoryCube(None, cube=tts, music=path)(text, speaker='s1'), want_bed)
