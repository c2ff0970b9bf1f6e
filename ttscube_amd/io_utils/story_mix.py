"""The timeline of StoryCube (cube/story.py:16-52): where each paragraph's audio goes (`plan_timeline`, pure Python) and the mix of speech and
looped background music into one int16 track (`mix_timeline`: one HIP launch, csrc/story.hip).  tests/story_reference.py restates both.

    s      = trunc(fl32(w 32767))                                               inside a segment (w: the generator's float32 sample), else 0
    out[t] = int16(trunc(fl32(fl32(fl32(music[t % M] gain) scale) + s)))

are the bits of the reference's per-sample loop.  One departure: where the sum leaves the int16 range the reference's `np.array(..., dtype='int16')`
is undefined; here the sample saturates to [-32768, 32767] and is counted (it cannot happen for |w| <= 0.69 with |music| <= 1 at the reference's
gain 0.30 and scale 32700).  Nothing here imports the extension until `mix_timeline` runs; there is no CPU path for the mix."""


def plan_timeline(lengths, sample_rate=24000, lead=5, gap=1, tail=5, texts=None):
    """lengths: samples of each paragraph's audio, in order -> (seg_dst, total, meta)

    seg_dst[p]: first timeline sample of paragraph p, behind `lead` seconds of music alone and `gap` seconds after each earlier paragraph;
    total = lead + sum(lengths[p] + gap) + tail, in samples; meta: the reference's list (cube/story.py:18-41) with its keys — the intro's is really
    spelled 'end:' — and its float arithmetic (`start` accumulates len / sample_rate + gap), `text` = texts[p] ('' without texts)."""
    lead_n, gap_n, tail_n = (_whole_samples(v, sample_rate, k) for v, k in ((lead, 'lead'), (gap, 'gap'), (tail, 'tail')))
    lengths = [int(v) for v in lengths]
    if any(v < 0 for v in lengths):
        raise ValueError('plan_timeline: negative length in %r' % (lengths,))
    if texts is not None and len(texts) != len(lengths):
        raise ValueError('plan_timeline: %d texts for %d lengths' % (len(texts), len(lengths)))
    meta = [{'name': 'intro', 'start': 0, 'end:': lead, 'text': ''}]
    seg_dst, pos, start = [], lead_n, lead
    for p, n in enumerate(lengths):
        seg_dst.append(pos)
        pos += n + gap_n
        meta.append({'name': 'paragraph', 'text': '' if texts is None else texts[p], 'start': start, 'end': start + (n / sample_rate) + gap})
        start += (n / sample_rate) + gap
    return seg_dst, pos + tail_n, meta


def _whole_samples(seconds, sample_rate, what):
    n = seconds * sample_rate
    if n < 0 or n != int(n):
        raise ValueError('plan_timeline: %s=%r s is not a whole, non-negative number of samples at %r Hz' % (what, seconds, sample_rate))
    return int(n)


def check_segments(seg_src, seg_len, seg_dst, speech_len, total):
    """the promises ttsc_story_mix cannot check on device tables, checked on host copies: lengths >= 0, every segment inside the speech buffer and
    inside the timeline, seg_dst ascending without overlap.  Raises _lib.TTSCError."""
    from .._lib import TTSCError
    if not (len(seg_src) == len(seg_len) == len(seg_dst)):
        raise TTSCError('mix_timeline: seg_src, seg_len and seg_dst hold %d, %d and %d entries' % (len(seg_src), len(seg_len), len(seg_dst)))
    end = 0
    for p, (s, n, d) in enumerate(zip(seg_src, seg_len, seg_dst)):
        if n < 0:
            raise TTSCError('mix_timeline: segment %d has the negative length %d' % (p, n))
        if s < 0 or s + n > speech_len:
            raise TTSCError('mix_timeline: segment %d reads speech[%d : %d], the buffer holds %d samples' % (p, s, s + n, speech_len))
        if d < end:
            raise TTSCError('mix_timeline: segment %d starts at timeline sample %d, before the end %d of the one before it (seg_dst must be '
                            'ascending and non-overlapping)' % (p, d, end))
        end = d + n
    if end > total:
        raise TTSCError('mix_timeline: the last segment ends at sample %d of a timeline of %d' % (end, total))


def mix_timeline(speech, seg_src, seg_len, seg_dst, music, total, gain=0.30, scale=32700.0, t0=0, n=None, return_clipped=False, out=None,
                 clipped=None):
    """speech: packed float32 waveforms on the device (only elements inside a segment are read); music: float32 [M >= 1] on the same device, looped;
    total: samples of the whole timeline -> int16 device tensor [n] holding timeline samples t0 .. t0 + n - 1 (n=None: up to `total`), written by
    one launch on the current stream.

    seg_src / seg_len / seg_dst, one entry per segment: first sample in `speech`, length, first sample on the timeline.  Given as host values
    (lists, numpy arrays, CPU tensors) they are checked here (`check_segments`) and uploaded in one copy; given as int64 device tensors they go to
    the kernel as they are, unchecked — reading them back would stall the stream — and the caller answers for them.
    return_clipped: also return the int64 [1] device count of saturated samples.  `clipped=` (int64 [1] on the device) is added to instead of a
    fresh zero; `out=` (int16 [n], contiguous) is written instead of a fresh tensor."""
    import ctypes as C

    import torch

    from .. import _lib
    _lib.require_gpu()
    assert speech.is_cuda and speech.dtype == torch.float32 and speech.dim() == 1 and speech.is_contiguous()
    assert music.dtype == torch.float32 and music.dim() == 1 and music.is_contiguous() and music.device == speech.device
    dev, total, t0 = speech.device, int(total), int(t0)
    n = total - t0 if n is None else int(n)
    if t0 < 0 or n < 0 or t0 + n > total:
        raise _lib.TTSCError('mix_timeline: the range t0=%d, n=%d does not lie inside a timeline of %d samples' % (t0, n, total))
    tables = (seg_src, seg_len, seg_dst)
    if all(torch.is_tensor(t) and t.is_cuda for t in tables):
        assert all(t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == dev for t in tables)
        assert seg_src.numel() == seg_len.numel() == seg_dst.numel()
        P = seg_src.numel()
    else:
        host = [[int(v) for v in (t.tolist() if hasattr(t, 'tolist') else t)] for t in tables]
        check_segments(host[0], host[1], host[2], speech.numel(), total)
        P = len(host[0])
        if P:
            both = torch.tensor(host, dtype=torch.int64).to(dev)            # [3, P]: one upload
            seg_src, seg_len, seg_dst = both[0], both[1], both[2]
    if out is None:
        out = torch.empty((n,), dtype=torch.int16, device=dev)
    assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.numel() == n and out.device == dev
    count = clipped
    if count is None and return_clipped:
        count = torch.zeros((1,), dtype=torch.int64, device=dev)
    if count is not None:
        assert count.is_cuda and count.dtype == torch.int64 and count.numel() == 1 and count.device == dev
    if P and speech.numel() == 0:                                            # only empty segments: the kernel reads nothing, the entry point wants a pointer
        speech = torch.zeros((1,), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ttsc_story_mix(ptr(speech if P else None), ptr(seg_src if P else None), ptr(seg_len if P else None),
                                             ptr(seg_dst if P else None), P, ptr(music), music.numel(), float(gain), float(scale), t0, n,
                                             ptr(out), ptr(count), _lib.current_stream()), 'ttsc_story_mix')
    return (out, count) if return_clipped else out
