"""Griffin-Lim on the HIP FFT kernels, timings on one GPU (profiles/griffinlim_bench.log).

Workload: 64 seeded rows x 8 s at 24 kHz, n_fft 1024, hop 240 (801 frames per row), 100 iterations: io_utils.stft.griffinlim from a device magnitude
to device audio (host clock around the call, ended by a device synchronise; median of --rounds), one ttsc_stft_project launch and one
ttsc_stft_overlap_add launch over the same batch (device events, median of 20), each with the bytes it must move: the padded signal and the magnitude
read and the frames written for the projection, the frames read and the padded signal written for the overlap-add.  Beside it the same loop written
with torch.stft / torch.istft on the same GPU (if torch's FFT backend loads there; nothing is substituted if it does not), and the numpy restatement
(tests/griffinlim_reference.py, float64, one thread) on ONE row for --host-iters iterations — anything scaled up from that is labelled as
extrapolated.  Only this size is measured.

    python tools/bench_griffinlim.py [--rounds 5] [--log profiles/griffinlim_bench.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SECONDS, RATE, N_FFT, HOP, N_ITER = 64, 8.0, 24000, 1024, 240, 100


def rows(seed=0):
    """B seeded rows: a few gliding partials and a little noise, peak below 1"""
    rng = np.random.default_rng(seed)
    L = int(SECONDS * RATE)
    t = np.arange(L) / RATE
    x = np.zeros((B, L), np.float32)
    for b in range(B):
        f = rng.uniform(90, 250) * (1.0 + 0.2 * np.sin(2 * np.pi * rng.uniform(0.2, 0.6) * t + rng.uniform(0, 6)))
        phase = 2 * np.pi * np.cumsum(f) / RATE
        v = sum(np.sin(h * phase) / h for h in range(1, 9))
        x[b] = 0.6 * v / np.abs(v).max() + 1e-3 * rng.standard_normal(L)
    return x


def event_median_ms(fn, rounds, warmup=3):
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


def call_median_ms(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def torch_griffinlim(mag, angles, n_iter):
    """the same loop on torch.stft / torch.istft: [B, F, nb] in, audio out (window='hann' periodic, center, reflect)"""
    win = torch.hann_window(N_FFT, periodic=True, device=mag.device)
    m = mag.abs().permute(0, 2, 1)
    a = angles.permute(0, 2, 1)
    L = HOP * (mag.shape[1] - 1)
    for _ in range(n_iter):
        y = torch.istft(m * a, N_FFT, hop_length=HOP, window=win, center=True, length=L)
        r = torch.stft(y, N_FFT, hop_length=HOP, window=win, center=True, pad_mode='reflect', return_complex=True)
        a = torch.exp(1j * torch.angle(r))
    return torch.istft(m * a, N_FFT, hop_length=HOP, window=win, center=True, length=L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'griffinlim_bench.log'))
    args = ap.parse_args()
    from tests import griffinlim_reference as R
    from ttscube_amd import _lib
    from ttscube_amd.io_utils import stft as S
    _lib.require_gpu()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device('cuda:0')
    host = rows()
    y = torch.from_numpy(host).to(dev)
    L = y.shape[1]
    F = 1 + L // HOP
    nb = N_FFT // 2 + 1
    Lsig = HOP * (F - 1) + N_FFT
    mag = S.stft(y, n_fft=N_FFT, hop=HOP).abs().contiguous()
    angles = torch.from_numpy(np.stack([S.draw_angles(nb, F, np.random.RandomState(b)) for b in range(B)])).to(dev)
    say('workload: %d rows x %.0f s at %d Hz, n_fft %d, hop %d: %d frames per row, %d in all; %d iterations; only this size was measured'
        % (B, SECONDS, RATE, N_FFT, HOP, F, B * F, N_ITER))

    t_call, runs = call_median_ms(lambda: S.griffinlim(mag, n_iter=N_ITER, hop=HOP, angles=angles), args.rounds)
    say('io_utils.stft.griffinlim, %d iterations = %d launches: %.2f ms (median of %d, host clock to a device synchronise; runs %s) = %.3f ms per '
        'iteration, %.0f x real time' % (N_ITER, 2 * N_ITER + 2, t_call, args.rounds, ' '.join('%.2f' % t for t in runs), t_call / N_ITER,
                                         B * SECONDS / (t_call * 1e-3)))

    rows_all = S._Rows(None, B, F, dev, 'frames')
    fr = S._synthesize(torch.view_as_real((mag * angles).contiguous()), rows_all, N_FFT, HOP)
    sig = S._overlap_add(fr, rows_all, N_FFT, HOP, True)
    t_prj = event_median_ms(lambda: S._project(sig, mag, rows_all, N_FFT, HOP, fr), 20)
    t_ola = event_median_ms(lambda: S._overlap_add(fr, rows_all, N_FFT, HOP, True, out=sig), 20)
    b_prj = (B * Lsig + B * F * nb + B * F * N_FFT) * 4
    b_ola = (B * F * N_FFT + B * Lsig) * 4
    say('one ttsc_stft_project launch     : %.3f ms (median of 20, device events); must move %.1f MB (signal %.1f + magnitude %.1f read, frames %.1f '
        'written) -> %.0f GB/s' % (t_prj, b_prj / 1e6, B * Lsig * 4 / 1e6, B * F * nb * 4 / 1e6, B * F * N_FFT * 4 / 1e6, b_prj / (t_prj * 1e6)))
    say('one ttsc_stft_overlap_add launch : %.3f ms (median of 20, device events); must move %.1f MB (frames %.1f read, padded signal %.1f written) '
        '-> %.0f GB/s' % (t_ola, b_ola / 1e6, B * F * N_FFT * 4 / 1e6, B * Lsig * 4 / 1e6, b_ola / (t_ola * 1e6)))
    say('  (each frame is read by the projection as %d samples at hop %d, %.1fx the signal; counted once above — the repeats come from the caches)'
        % (N_FFT, HOP, N_FFT / HOP))

    try:
        ref = torch_griffinlim(mag, angles, 2)
        torch.cuda.synchronize()
    except Exception as e:                                          # noqa: BLE001 — whatever keeps torch's FFT backend from loading is reported as is
        say('torch.stft / torch.istft loop on the same GPU: NOT measured, torch\'s FFT backend did not run here (%s: %s)'
            % (type(e).__name__, str(e).splitlines()[0] if str(e) else ''))
    else:
        ours = S.griffinlim(mag, n_iter=2, hop=HOP, angles=angles)
        diff = float((ours - ref).abs().max() / ref.abs().max())
        t_torch, runs = call_median_ms(lambda: torch_griffinlim(mag, angles, N_ITER), args.rounds)
        say('the same loop on torch.stft / torch.istft, same GPU: %.2f ms (median of %d; runs %s) = %.3f ms per iteration; max |ours - torch| after 2 '
            'iterations %.2e of the peak' % (t_torch, args.rounds, ' '.join('%.2f' % t for t in runs), t_torch / N_ITER, diff))

    m1 = mag[0].cpu().numpy().astype(np.float64)
    a1 = angles[0].cpu().numpy()
    t0 = time.perf_counter()
    R.griffinlim(m1, a1, args.host_iters, HOP)
    t_host = time.perf_counter() - t0
    per_iter = t_host / (args.host_iters + 1)
    say('numpy restatement (float64, one thread), ONE row, %d iterations: %.2f s = %.3f s per inverse + forward pair' % (args.host_iters, t_host, per_iter))
    say('  EXTRAPOLATED, not measured: %d rows x %d iterations at that rate would take about %.0f s' % (B, N_ITER, per_iter * (N_ITER + 1) * B))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
