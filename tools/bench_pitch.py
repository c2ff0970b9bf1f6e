"""Pitch tracker and corpus import timings on one GPU (profiles/pitch_bench.log).

Workload: 64 utterances x 8 s at 24 kHz, seeded harmonic signals (F0 glides with voiced and silent stretches), hop 240, 60-400 Hz.
Medians over rounds of
  * the tracker alone (both launches, device input to device output) and each launch on its own;
  * the whole import (text side, wav read, spectrogram, pitch, files written) in utterance-seconds per second;
and two comparators:
  * the NCCF stage as torch ops on the same GPU (`unfold` + batched products, no peak picking);
  * the tracking stage in the numpy restatement (tests/pitch_reference.py, float64, one utterance, scaled to the batch).
RAPT itself (pysptk) is not installed here and is not timed.

    python tools/bench_pitch.py [--rounds 7] [--no-import]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SECONDS, SR, HOP, FMIN, FMAX = 64, 8.0, 24000, 240, 60, 400


def signals(seed=7):
    rng = np.random.default_rng(seed)
    L = int(SECONDS * SR)
    t = np.arange(L) / SR
    x = np.zeros((B, L), np.float32)
    for b in range(B):
        f = rng.uniform(90, 250) * (1.0 + 0.2 * np.sin(2 * np.pi * rng.uniform(0.2, 0.6) * t + rng.uniform(0, 6)))
        phase = 2 * np.pi * np.cumsum(f) / SR
        v = sum(np.sin(h * phase) / h for h in range(1, 9))
        gate = (np.sin(2 * np.pi * rng.uniform(0.3, 0.8) * t + rng.uniform(0, 6)) > -0.6).astype(np.float64)     # silent stretches
        x[b] = 0.3 * v / np.abs(v).max() * gate + 1e-4 * rng.standard_normal(L)
    return x


def gpu_median_ms(fn, rounds, warmup=2):
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


def torch_nccf(x, n, kmin, kmax):
    """the NCCF stage as torch ops: frames by unfold, then per block of lags a batched product and two reductions"""
    span = n + kmax
    F = x.shape[1] // HOP
    xp = torch.nn.functional.pad(x, (0, span))
    fr = xp.unfold(1, span, HOP)[:, :F]
    s = fr - fr.mean(dim=2, keepdim=True)
    head = s[:, :, :n]
    e0 = (head * head).sum(dim=2)
    out = torch.empty((x.shape[0], F, kmax - kmin + 1), device=x.device)
    for k0 in range(kmin, kmax + 1, 32):
        k1 = min(k0 + 32, kmax + 1)
        seg = s[:, :, k0:k1 - 1 + n].unfold(2, n, 1)                      # [B, F, lags, n]
        num = (seg * head.unsqueeze(2)).sum(dim=3)
        ek = (seg * seg).sum(dim=3)
        out[:, :, k0 - kmin:k1 - kmin] = num / torch.sqrt(e0.unsqueeze(2) * ek + 10000.0 / 32768.0 ** 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-import', action='store_true')
    args = ap.parse_args()
    from ttscube_amd.io_utils import pitch
    from tests import pitch_reference as R
    dev = torch.device('cuda:0')
    x_host = signals()
    x = torch.from_numpy(x_host).to(dev)
    lengths = torch.full((B,), x.shape[1], dtype=torch.int32, device=dev)
    n, kmin, kmax = pitch.lag_range(SR, FMIN, FMAX)
    F = x.shape[1] // HOP
    nframes = torch.full((B,), F, dtype=torch.int32, device=dev)
    tracker = pitch.PitchTracker(dev)
    print('workload: %d x %.0f s at %d Hz, hop %d, %d-%d Hz: %d frames per utterance, %d lags, window %d' % (B, SECONDS, SR, HOP, FMIN, FMAX, F,
                                                                                                        kmax - kmin + 1, n))
    tab = pitch.nccf(x, lengths, SR, HOP, FMIN, FMAX)
    t_both = gpu_median_ms(lambda: tracker.f0_device(x, lengths, SR, HOP, FMIN, FMAX), args.rounds)
    t_nccf = gpu_median_ms(lambda: pitch.nccf(x, lengths, SR, HOP, FMIN, FMAX), args.rounds)
    t_track = gpu_median_ms(lambda: pitch.track(tab['cand_lag'], tab['cand_val'], tab['ncand'], tab['maxphi'], tab['rms'], nframes, kmax, SR),
                            args.rounds)
    audio_s = B * SECONDS
    print('tracker, both launches : %8.3f ms   (%.0f x real time)' % (t_both, audio_s / (t_both * 1e-3)))
    print('  ttsc_pitch_nccf      : %8.3f ms' % t_nccf)
    print('  ttsc_pitch_track     : %8.3f ms' % t_track)
    t_torch = gpu_median_ms(lambda: torch_nccf(x, n, kmin, kmax), max(3, args.rounds // 2), warmup=1)
    phi_k = pitch.nccf(x[:4], lengths[:4], SR, HOP, FMIN, FMAX, want_phi=True)['phi']
    phi_t = torch_nccf(x[:4], n, kmin, kmax)
    print('NCCF as torch ops      : %8.3f ms   (%.1f x ttsc_pitch_nccf; max |phi difference| on 4 utterances %.2e)' % (
        t_torch, t_torch / t_nccf, float((phi_k - phi_t).abs().max())))
    host = {k: v[0].cpu().numpy() for k, v in tab.items() if v is not None}
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        R.track(host['cand_lag'], host['cand_val'], host['ncand'], host['maxphi'], host['rms'], kmax, SR, np.float64)
        times.append(time.perf_counter() - t0)
    t_np = statistics.median(times) * 1e3
    print('tracking in numpy      : %8.3f ms per utterance, %.0f ms for the batch   (%.0f x ttsc_pitch_track)' % (t_np, t_np * B, t_np * B / t_track))
    if args.no_import:
        return
    import scipy.io.wavfile
    from ttscube_amd.io_utils.corpus_import import import_dataset
    from tests.test_import_textgrid_gpu import _textgrid
    with tempfile.TemporaryDirectory() as root:
        src = os.path.join(root, 'aligned')
        os.makedirs(src)
        words = [('', [''])] + [('word', ['W', 'ER1', 'D'])] * 12 + [('', [''])]
        for b in range(B):
            scipy.io.wavfile.write(os.path.join(src, 'u%03d.wav' % b), SR, np.asarray(x_host[b] * 32767, dtype=np.int16))
            with open(os.path.join(src, 'u%03d.TextGrid' % b), 'w') as f:
                f.write(_textgrid(SECONDS, words, ' '.join(['word'] * 12)))
        times = []
        for r in range(3):
            t0 = time.perf_counter()
            counts = import_dataset(src, os.path.join(root, 'out%d' % r), dev_ratio=0.1, sample_rate=SR, hop_size=HOP, batch=32, device='cuda:0')
            assert sum(counts) == B, counts
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t_imp = statistics.median(times)
        print('whole import           : %8.3f s for %d utterances (%d train, %d dev): %.0f utterance-seconds per second' % (
            t_imp, B, counts[0], counts[1], audio_s / t_imp))


if __name__ == '__main__':
    main()
