"""Loudness meter and gain stage timings on one GPU (profiles/loudness_bench.log).

64 seeded rows x 8 s at 24 kHz, on the device: ttsc_loudness_measure (its five kernels: tile states, row scan, energies, combine, peaks),
ttsc_loudness_finish and ttsc_loudness_apply, each call alone and the three in a row, by device events (median of --rounds after warm-up), beside
the same computation on the host over the same rows, one after the other in this process: scipy.signal.sosfilt for the K-weighting, numpy for
the sub-blocks, blocks and gates, scipy.signal.upfirdn with the same float32 filter for the 4x true peak, one float32 product for the gain
(median of 3).  The two are compared row by row.  Bytes that must be moved: the rows read once to measure, read and written once to scale
(3 x 4 bytes per sample).  Only this size is measured.

    python tools/bench_loudness.py [--rounds 20] [--log profiles/loudness_bench.log]"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SECONDS, RATE = 64, 8.0, 24000
TARGET, PEAK_DB = -23.0, -1.0


def rows(seed=11):
    """B seeded rows: a few gliding partials under a slow envelope and a little noise, levels spread over 20 dB"""
    rng = np.random.default_rng(seed)
    L = int(SECONDS * RATE)
    t = np.arange(L) / RATE
    x = np.zeros((B, L), np.float32)
    for b in range(B):
        f = rng.uniform(90, 250) * (1.0 + 0.2 * np.sin(2 * np.pi * rng.uniform(0.2, 0.6) * t + rng.uniform(0, 6)))
        phase = 2 * np.pi * np.cumsum(f) / RATE
        v = sum(np.sin(h * phase) / h for h in range(1, 9)) * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(0.3, 1.5) * t))
        x[b] = 10.0 ** (-rng.uniform(0, 20) / 20.0) * 0.9 * v / np.abs(v).max() + 1e-3 * rng.standard_normal(L)
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


def host_normalize(x, M):
    """the same computation with scipy and numpy -> (y float32 [B, L], lufs [B], gain float32 [B])"""
    sos = M.k_weighting(RATE)
    h = M.resample.design_filter(4, 1).astype(np.float32).astype(np.float64)
    S = RATE // 10
    y, lufs, gains = np.empty_like(x), np.empty(len(x)), np.empty(len(x), np.float32)
    for b, row in enumerate(x):
        k = scipy.signal.sosfilt(sos, row.astype(np.float64))
        sub = (k[:len(k) // S * S].reshape(-1, S) ** 2).sum(axis=1)
        z = (sub[:-3] + sub[1:-2] + sub[2:-1] + sub[3:]) / (4.0 * S)
        a = z > M.ABS_GATE
        m = a & (z > 0.1 * z[a].mean())
        zbar = z[m].mean()
        tp = np.abs(scipy.signal.upfirdn(h, row.astype(np.float64), up=4)[40:40 + 4 * len(row)]).max()
        g, _ = M.host_gain(zbar, max(float(np.abs(row).max()), tp), False, TARGET, PEAK_DB)
        y[b], lufs[b], gains[b] = g * row, float(M.lufs(zbar)), g
    return y, lufs, gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'loudness_bench.log'))
    args = ap.parse_args()
    if args.rounds < 1:
        ap.error('--rounds must be at least 1')
    import ctypes as C
    from ttscube_amd import _lib
    from ttscube_amd.io_utils import loudness as M
    _lib.require_gpu()
    L = _lib.lib()
    x = rows()
    n = x.shape[1]
    xd = torch.from_numpy(x).cuda()
    ld = torch.full((B,), n, dtype=torch.int32, device='cuda')
    meter = M.LoudnessMeter('cuda:0')
    p = lambda t: C.c_void_p(t.data_ptr())

    # the three calls on buffers made once
    nsub = -(-n // (RATE // 10))
    k, taps = M.kernel_constants(RATE), np.ascontiguousarray(M.true_peak_taps())
    sub = torch.empty((B, nsub), dtype=torch.float64, device='cuda')
    sp, tp = torch.empty(B, device='cuda'), torch.empty(B, device='cuda')
    nbytes = int(L.ttsc_loudness_workspace_bytes(B, n, RATE))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    te = torch.full((B,), float(M.target_energy(TARGET)), dtype=torch.float64, device='cuda')
    pl = torch.full((B,), 10.0 ** (PEAK_DB / 20.0), dtype=torch.float64, device='cuda')
    zbar = torch.empty(B, dtype=torch.float64, device='cuda')
    blocks, gated, silent, lim = (torch.empty(B, dtype=torch.int32, device='cuda') for _ in range(4))
    gain = torch.empty(B, device='cuda')
    yd = torch.empty_like(xd)

    def measure():
        _lib.check(L.ttsc_loudness_measure(p(xd), p(ld), B, n, RATE, k.ctypes.data_as(C.c_void_p), taps.ctypes.data_as(C.c_void_p), p(sub), nsub,
                                           p(sp), p(tp), p(ws), nbytes, _lib.current_stream()), 'measure')

    def finish():
        _lib.check(L.ttsc_loudness_finish(p(sub), p(ld), B, n, nsub, RATE, p(sp), p(tp), M.ABS_GATE, p(te), p(pl), 0.0, p(zbar), p(blocks),
                                          p(gated), p(silent), p(gain), p(lim), _lib.current_stream()), 'finish')

    def apply():
        _lib.check(L.ttsc_loudness_apply(p(xd), p(ld), p(gain), B, n, p(yd), _lib.current_stream()), 'apply')

    def all_three():
        measure()
        finish()
        apply()

    t_m, t_f, t_a, t_all = (gpu_median_ms(f, args.rounds) for f in (measure, finish, apply, all_three))
    t_api = gpu_median_ms(lambda: meter.normalize_device(xd, ld, RATE, TARGET, peak_db=PEAK_DB, inplace=False), args.rounds)

    host_times = []
    for _ in range(3):
        t0 = time.perf_counter()
        hy, hl, hg = host_normalize(x, M)
        host_times.append((time.perf_counter() - t0) * 1e3)
    t_host = statistics.median(host_times)
    gl = M.lufs(zbar.cpu().numpy())
    gy = yd.cpu().numpy()
    moved = 3 * 4 * B * n
    audio_s = B * SECONDS
    lines = [
        'workload: %d rows x %g s at %d Hz, float32 on the device, target %.1f LUFS under %.1f dB true peak; device events, median of %d; host = '
        'scipy.signal.sosfilt + numpy + scipy.signal.upfirdn row by row in one process (median of 3); only this size was measured'
        % (B, SECONDS, RATE, TARGET, PEAK_DB, args.rounds),
        '  ttsc_loudness_measure (tile states, row scan, energies, combine, peaks: 5 kernels) : %8.3f ms' % t_m,
        '  ttsc_loudness_finish  (blocks, gates, gain: one workgroup per row)                 : %8.3f ms' % t_f,
        '  ttsc_loudness_apply   (y = fl32(g x))                                              : %8.3f ms' % t_a,
        '  measure + finish + apply in a row                                                  : %8.3f ms  (%.1f GB/s of the %.1f MB that must be '
        'moved, %d x real time)' % (t_all, moved / t_all / 1e6, moved / 1e6, audio_s / (t_all * 1e-3)),
        '  LoudnessMeter.normalize_device (the same with its allocations and constant upload)  : %8.3f ms' % t_api,
        '  host, the same computation                                                          : %8.3f ms  (%d x real time; runs %s)'
        % (t_host, audio_s / (t_host * 1e-3), ' '.join('%.0f' % t for t in host_times)),
        '  agreement over the %d rows: max |LUFS kernel - host| %.2e, gains equal in %d rows (max relative difference %.2e), output samples '
        'equal in %.4f %% (max |difference| %.2e)' % (B, np.abs(gl - hl).max(), int((gain.cpu().numpy() == hg).sum()),
                                                      float(np.abs(gain.cpu().numpy() / hg - 1).max()), 100.0 * float((gy == hy).mean()),
                                                      float(np.abs(gy - hy).max())),
        '  rows read %.1f .. %.1f LUFS, %d of %d met the peak ceiling' % (gl.min(), gl.max(), int(lim.sum().item()), B),
    ]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(args.log, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
