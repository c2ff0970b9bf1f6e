"""HIP resampler and vocoder feature cache timings on one GPU (profiles/resample_bench.log).

Kernel: 64 seeded rows x 8 s at 44.1 kHz and at 48 kHz, each to 24 kHz and to 2.4 kHz — one ttsc_resample_poly launch over the batch (device
input to device output, device events, median of --rounds launches after warm-up) beside scipy.signal.resample_poly over the same 64 float32 rows,
one after the other in this process (scipy runs it on one thread however many are free; median of 3).
Whole folder: 64 such files (32 at each rate, int16 wav) in a temporary folder — VocoderDataset.precompute(batch=32) against reading the same
fresh dataset item by item through the lazy path (scipy twice and one spectrogram call per file), three fresh cache directories each, alternated.
Only these sizes are measured.

    python tools/bench_resample.py [--rounds 20] [--log profiles/resample_bench.log]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import scipy.io.wavfile
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SECONDS = 64, 8.0
SOURCE_RATES, TARGET_RATES = (44100, 48000), (24000, 2400)


def rows(rate, seed):
    """B seeded rows: a few gliding partials and a little noise, peak below 1"""
    rng = np.random.default_rng(seed)
    L = int(SECONDS * rate)
    t = np.arange(L) / rate
    x = np.zeros((B, L), np.float32)
    for b in range(B):
        f = rng.uniform(90, 250) * (1.0 + 0.2 * np.sin(2 * np.pi * rng.uniform(0.2, 0.6) * t + rng.uniform(0, 6)))
        phase = 2 * np.pi * np.cumsum(f) / rate
        v = sum(np.sin(h * phase) / h for h in range(1, 9))
        x[b] = 0.6 * v / np.abs(v).max() + 1e-3 * rng.standard_normal(L)
    return x


def gpu_median_ms(fn, rounds, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'resample_bench.log'))
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error('--rounds must be at least 20')
    from ttscube_amd import _lib
    from ttscube_amd.io_utils import resample as RS
    from ttscube_amd.io_utils.io_vocoder import VocoderDataset
    from ttscube_amd.io_utils.vocoder import MelVocoder
    _lib.require_gpu()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda:0')
    resampler = RS.Resampler(dev)
    say('workload: %d rows x %.0f s, float32; kernel = one ttsc_resample_poly launch (median of %d by device events); scipy = '
        'scipy.signal.resample_poly row by row in one process, which runs it on one thread (median of 3); only these sizes were measured'
        % (B, SECONDS, args.rounds))
    host = {}
    for rate in SOURCE_RATES:
        host[rate] = rows(rate, rate)
        x = torch.from_numpy(host[rate]).to(dev)
        lengths = torch.full((B,), x.shape[1], dtype=torch.int32, device=dev)
        for sr in TARGET_RATES:
            up, down = RS.ratio(rate, sr)
            y, _, _ = resampler.resample_device(x, lengths, rate, sr)
            t_gpu = gpu_median_ms(lambda: resampler.resample_device(x, lengths, rate, sr), args.rounds)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = [scipy.signal.resample_poly(row, up, down) for row in host[rate]]
                times.append(time.perf_counter() - t0)
            t_cpu = statistics.median(times) * 1e3
            diff = float(np.abs(y.cpu().numpy() - np.stack(ref)).max())
            moved = (x.numel() + y.numel()) * 4 / 1e9
            say('%6d -> %5d Hz (up %3d, down %3d, %4d taps): kernel %8.3f ms (%6.1f GB/s of rows read + written, %7.0f x real time)   '
                'scipy %9.1f ms   max |kernel - scipy float32| %.2e' % (rate, sr, up, down, 20 * max(up, down) + 1, t_gpu, moved / (t_gpu * 1e-3),
                                                                        B * SECONDS / (t_gpu * 1e-3), t_cpu, diff))

    vocoder = MelVocoder(dev)
    with tempfile.TemporaryDirectory() as root:
        wavs = os.path.join(root, 'wavs')
        os.makedirs(wavs)
        n = 0
        for rate in SOURCE_RATES:
            for b in range(B // len(SOURCE_RATES)):
                scipy.io.wavfile.write(os.path.join(wavs, 'u%03d.wav' % n), rate, np.asarray(host[rate][b] * 32767, dtype=np.int16))
                n += 1
        t0 = time.perf_counter()
        for name in sorted(os.listdir(wavs)):
            scipy.io.wavfile.read(os.path.join(wavs, name))
        t_read = time.perf_counter() - t0
        t_pre, t_lazy = [], []
        for r in range(3):
            ds = VocoderDataset(wavs, cache_dir=os.path.join(root, 'cache_pre%d' % r), mel_vocoder=vocoder)
            t0 = time.perf_counter()
            written = ds.precompute(batch=32, device=dev, resampler=resampler)
            torch.cuda.synchronize()
            t_pre.append(time.perf_counter() - t0)
            assert written == n, written
            ds = VocoderDataset(wavs, cache_dir=os.path.join(root, 'cache_lazy%d' % r), mel_vocoder=vocoder)
            t0 = time.perf_counter()
            for i in range(len(ds)):
                ds[i]
            torch.cuda.synchronize()
            t_lazy.append(time.perf_counter() - t0)
        audio_s = n * SECONDS
        say('whole folder, %d files x %.0f s (%d at each of %s Hz, int16 wav), features to 24 kHz / 2.4 kHz / log-mel, cache files written, median '
            'of 3 fresh cache directories each, alternated:' % (n, SECONDS, B // len(SOURCE_RATES), ' and '.join(str(r) for r in SOURCE_RATES)))
        say('  VocoderDataset.precompute(batch=32) : %7.3f s  (%5.0f audio-seconds per second; runs %s)' % (
            statistics.median(t_pre), audio_s / statistics.median(t_pre), ' '.join('%.3f' % t for t in t_pre)))
        say('  lazy path, item by item             : %7.3f s  (%5.0f audio-seconds per second; runs %s)' % (
            statistics.median(t_lazy), audio_s / statistics.median(t_lazy), ' '.join('%.3f' % t for t in t_lazy)))
        say('  reading the %d wav files alone       : %7.3f s (one pass, files just written: from the page cache)' % (n, t_read))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
