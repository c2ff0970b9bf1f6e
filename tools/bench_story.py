"""StoryCube timeline mixer timings on one GPU (profiles/story_bench.log).  Seeded data, no model: 20 segments of 30 s, the reference's 5 s lead,
1 s behind each segment and 5 s tail (630 s of track at 24 kHz) over a 180 s music loop.  Only this size is measured.

Four sides in one process, the two GPU sides alternated round by round (device events, median of --rounds after warm-up):
  1. the one-launch mix (ttsc_story_mix through io_utils.story_mix.mix_timeline, device tables, device input to device output)
  2. the same formula as torch ops on the same GPU: arange % M, gather, 20 slice copies of trunc(w 32767), three float32 ops, trunc, clamp, cast
  3. the formula vectorised in numpy on the host (median of 3)
  4. the reference's literal per-sample Python loop on a 1 s slice, extrapolated to the track: NOT a measurement of the whole track
All three array results must equal each other bit for bit, or the tool fails.

    python tools/bench_story.py [--rounds 20] [--log profiles/story_bench.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE, SEGMENTS, SEG_SECONDS, MUSIC_SECONDS = 24000, 20, 30, 180
GAIN, SCALE = 0.30, 32700.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--log', default=None, help='also write the lines to this file (profiles/story_bench.log)')
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error('--rounds must be at least 20')
    from ttscube_amd import _lib
    from ttscube_amd.io_utils.story_mix import mix_timeline, plan_timeline
    _lib.require_gpu()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda:0')
    rng = np.random.default_rng(2024)
    lengths = [SEG_SECONDS * RATE] * SEGMENTS
    seg_dst, total, _ = plan_timeline(lengths, RATE)
    seg_src = [p * SEG_SECONDS * RATE for p in range(SEGMENTS)]
    speech_h = rng.uniform(-0.69, 0.69, size=sum(lengths)).astype(np.float32)
    music_h = rng.uniform(-1.0, 1.0, size=MUSIC_SECONDS * RATE).astype(np.float32)
    M = music_h.size
    speech, music = torch.from_numpy(speech_h).to(dev), torch.from_numpy(music_h).to(dev)
    tables = [torch.tensor(t, dtype=torch.int64, device=dev) for t in (seg_src, lengths, seg_dst)]
    out = torch.empty((total,), dtype=torch.int16, device=dev)
    g32, s32 = float(np.float32(GAIN)), float(np.float32(SCALE))

    def kernel():
        mix_timeline(speech, tables[0], tables[1], tables[2], music, total, gain=GAIN, scale=SCALE, out=out)

    def torch_ops():
        idx = torch.arange(total, device=dev) % M
        v = (music[idx] * g32) * s32
        s = torch.zeros((total,), dtype=torch.float32, device=dev)
        for a, n, d in zip(seg_src, lengths, seg_dst):
            s[d:d + n] = torch.trunc(speech[a:a + n] * 32767.0)
        return torch.trunc(v + s).clamp_(-32768.0, 32767.0).to(torch.int16)

    def numpy_ops():
        idx = np.arange(total, dtype=np.int64) % M
        v = (music_h[idx] * np.float32(GAIN)) * np.float32(SCALE)
        s = np.zeros(total, dtype=np.float32)
        for a, n, d in zip(seg_src, lengths, seg_dst):
            s[d:d + n] = np.trunc(speech_h[a:a + n] * np.float32(32767))
        return np.clip(np.trunc(v + s), -32768, 32767).astype(np.int16)

    say('workload: %d segments x %d s + %d s lead, 1 s gaps, %d s tail = %d samples (%.0f s at %d Hz), music loop %d s (%.1f MB float32); seeded '
        'data, no model; only this size was measured' % (SEGMENTS, SEG_SECONDS, 5, 5, total, total / RATE, RATE, MUSIC_SECONDS, M * 4 / 1e6))
    for _ in range(3):
        kernel()
        ref_t = torch_ops()
    torch.cuda.synchronize()
    t_k, t_t = [], []
    for _ in range(args.rounds):
        t_k.append(event_ms(kernel))
        t_t.append(event_ms(torch_ops))
    k_host, t_host = out.cpu().numpy(), ref_t.cpu().numpy()
    t_n = []
    for _ in range(3):
        t0 = time.perf_counter()
        n_host = numpy_ops()
        t_n.append((time.perf_counter() - t0) * 1e3)
    if not (np.array_equal(k_host, t_host) and np.array_equal(k_host, n_host)):
        raise SystemExit('bench_story: the three results differ (kernel vs torch ops: %d samples, kernel vs numpy: %d)'
                         % (np.count_nonzero(k_host != t_host), np.count_nonzero(k_host != n_host)))
    # the reference's loop (cube/story.py:50-52) on the first second that holds speech
    lo = seg_dst[0]
    buffer = [x for x in np.asarray(speech_h[:RATE] * 32767, dtype=np.int16)]
    t0 = time.perf_counter()
    for ii in range(len(buffer)):
        buffer[ii] = (music_h[(lo + ii) % len(music_h)] * 0.30) * 32700 + buffer[ii]
    literal = np.array(buffer, dtype='int16')
    t_l = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(literal, k_host[lo:lo + RATE]))
    moved = (total * 2 + total * 4 + sum(lengths) * 4) / 1e9
    mk, mt, mn = statistics.median(t_k), statistics.median(t_t), statistics.median(t_n)
    say('1. one-launch mix (ttsc_story_mix)   : %9.3f ms  median of %d (min %.3f, max %.3f); %.3f GB must move (2 B written + 4 B of music per '
        'sample, 4 B per speech sample) -> %.0f GB/s; %.0f x real time' % (mk, args.rounds, min(t_k), max(t_k), moved, moved / (mk * 1e-3),
                                                                           total / RATE / (mk * 1e-3)))
    say('2. torch ops on the same GPU         : %9.3f ms  median of %d (min %.3f, max %.3f), alternated with 1.; same bytes' % (
        mt, args.rounds, min(t_t), max(t_t)))
    say('3. numpy on the host, vectorised     : %9.1f ms  median of 3; same bytes' % mn)
    say('4. the reference\'s per-sample loop   : %9.1f ms for a 1 s slice (%s the kernel\'s bytes there) -> %.0f s for the track, extrapolated '
        'from 1 s, not measured' % (t_l, 'equal to' if same else 'DIFFERENT from', t_l * 1e-3 * total / RATE))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
