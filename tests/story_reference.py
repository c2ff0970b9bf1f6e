"""Restatements of cube/story.py for the StoryCube tests (not a test module): the timeline bookkeeping, the per-sample mixing loop as the
reference runs it, and the same formula as array operations.

    buffer[ii] = (music[ii % len(music)] * 0.30) * 32700 + buffer[ii];   np.array(buffer, dtype='int16')

with `music[ii]` an np.float32 scalar and `buffer[ii]` an np.int16 speech sample (or the int 0): two float32 products and a float32 sum, each
rounded on its own, then a cast that truncates toward zero."""
import numpy as np


def speech_to_i16(w):
    """what TTSCube.__call__ does with the generator's float32 output"""
    return np.asarray(np.asarray(w, dtype=np.float32) * 32767, dtype=np.int16)


def timeline_literal(lengths, texts=None):
    """cube/story.py:15-47 with the audio replaced by its length -> (first sample of each part, total samples, metadata)"""
    position = 24000 * 5
    metadata = [
        {
            'name': 'intro',
            'start': 0,
            'end:': 5,
            'text': ''
        }
    ]
    offsets = []
    start = 5
    for k, n in enumerate(lengths):
        offsets.append(position)
        position += n
        position += 24000
        metadata.append({
            'name': 'paragraph',
            'text': '' if texts is None else texts[k],
            'start': start,
            'end': start + (n / 24000) + 1
        })
        start += (n / 24000) + 1
    position += 24000 * 5
    return offsets, position, metadata


def mix_literal(segments_i16, seg_dst, music_f32, total, gain=0.30, scale=32700.0):
    """the reference's loop over every sample, np.float32 / np.int16 scalars and the final np.array(..., dtype='int16').  Only for inputs whose
    sums stay inside int16 (the cast is undefined otherwise)."""
    assert music_f32.dtype == np.float32
    buffer = [0 for _ in range(total)]
    for seg, d in zip(segments_i16, seg_dst):
        assert seg.dtype == np.int16
        for k, x in enumerate(seg):
            buffer[d + k] = x                                   # an np.int16 scalar, as `for x in audio: buffer.append(x)` leaves it
    music = music_f32
    g, s = np.float32(gain), np.float32(scale)
    for ii in range(len(buffer)):
        buffer[ii] = (music[ii % len(music)] * g) * s + buffer[ii]
        assert type(buffer[ii]) is np.float32
    return np.array(buffer, dtype='int16')


def _range(segments_i16, seg_dst, music_f32, total, t0, n):
    """-> (speech as int64 [n], music as float32 [n]) of timeline samples t0 .. t0 + n - 1; indices are Python integers / int64 throughout"""
    n = total - t0 if n is None else n
    assert music_f32.dtype == np.float32 and 0 <= t0 and t0 + n <= total
    speech = np.zeros(n, dtype=np.int64)
    for seg, d in zip(segments_i16, seg_dst):
        assert seg.dtype == np.int16
        lo, hi = max(d, t0), min(d + len(seg), t0 + n)
        if lo < hi:
            speech[lo - t0:hi - t0] = seg[lo - d:hi - d]
    M = len(music_f32)
    phase = (np.arange(n, dtype=np.int64) + np.int64(t0 % M)) % np.int64(M)
    return speech, music_f32[phase]


def mix_vectorised(segments_i16, seg_dst, music_f32, total, gain=0.30, scale=32700.0, t0=0, n=None):
    """three float32 array operations, trunc, saturation -> (int16 [n], number of saturated samples)"""
    speech, music = _range(segments_i16, seg_dst, music_f32, total, t0, n)
    a = music * np.float32(gain)
    b = a * np.float32(scale)
    v = b + speech.astype(np.float32)
    assert a.dtype == b.dtype == v.dtype == np.float32
    r = np.trunc(v)
    clipped = int(np.count_nonzero((r > 32767) | (r < -32768)))
    return np.clip(r, -32768, 32767).astype(np.int16), clipped


def mix_float64(segments_i16, seg_dst, music_f32, total, gain=0.30, scale=32700.0, t0=0, n=None):
    """the formula evaluated in float64 (what a kernel in double, or a host loop over Python floats, would give) -> int16, saturated"""
    speech, music = _range(segments_i16, seg_dst, music_f32, total, t0, n)
    v = music.astype(np.float64) * float(gain) * float(scale) + speech
    return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)


def mix_fused(segments_i16, seg_dst, music_f32, total, gain=0.30, scale=32700.0, t0=0, n=None):
    """the second product and the sum contracted into one fused multiply-add (one rounding instead of two) -> int16, saturated.  fl32(m gain) has
    24 significant bits and `scale` 15, so the float64 product is exact and the float64 sum with an integer below 2^15 is exact wherever the
    product is not tiny; one rounding to float32 follows."""
    speech, music = _range(segments_i16, seg_dst, music_f32, total, t0, n)
    a = music * np.float32(gain)
    v = (a.astype(np.float64) * float(np.float32(scale)) + speech).astype(np.float32)
    return np.clip(np.trunc(v), -32768, 32767).astype(np.int16)
