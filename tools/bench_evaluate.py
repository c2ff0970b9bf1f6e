"""Dev-set evaluation timings on one GPU (profiles/evaluate_bench.log).

Workload: 64 pairs of seeded harmonic utterances at 24 kHz, hop 240; the reference side has 800 frames, the synthesized side is the same F0 and
gating contour rendered at 700 .. 900 frames (seeded), K = 24 cepstral coefficients.  Only this size is measured, plus one pair of 3000 x 3000
frames, timed once.  Medians over rounds of
  * the DTW launch alone (ttsc_dtw_align on the cepstra, device input to device output);
  * the whole Evaluator.evaluate_audio call (log-mel, F0, cepstra, DTW, scores; ends in the scores' copy to the host);
and two comparators for the DTW:
  * the same dynamic program as a loop of torch ops over anti-diagonals on the same GPU (costs only: it keeps no back-pointers and walks no path);
  * the float64 numpy restatement (tests/dtw_reference.py) on the host, timed on two pairs; its batch figure is that time scaled to 64 pairs — an
    extrapolation, not a measurement.

    python tools/bench_evaluate.py [--rounds 7]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, REF_FRAMES, SYN_LO, SYN_HI, SR, HOP, K = 64, 800, 700, 900, 24000, 240, 24


def render(rng_state, frames):
    """one utterance of `frames` frames from a contour drawn on normalised time (the same state gives the same contour at another length)"""
    rng = np.random.default_rng(rng_state)
    L = frames * HOP
    u = np.arange(L) / L
    f = rng.uniform(90, 250) * (1.0 + 0.2 * np.sin(2 * np.pi * rng.uniform(1.5, 5.0) * u + rng.uniform(0, 6)))
    gate = (np.sin(2 * np.pi * rng.uniform(2.0, 6.0) * u + rng.uniform(0, 6)) > -0.6).astype(np.float64)
    phase = 2 * np.pi * np.cumsum(f) / SR
    v = sum(np.sin(h * phase) / h for h in range(1, 9))
    return (0.3 * v / np.abs(v).max() * gate + 1e-4 * np.random.default_rng(rng_state + 1000003 * frames).standard_normal(L)).astype(np.float32)


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


def torch_dtw_cost(a, la, b, lb):
    """the same recurrence over anti-diagonals with torch ops: cost [P] only.  Local costs from the differences (cdist without the matrix-product
    form), skewed once so that anti-diagonal s is a contiguous row; then one small group of ops per anti-diagonal."""
    Pn, Na, _ = a.shape
    Nb = b.shape[1]
    d = torch.cdist(a, b, compute_mode='donot_use_mm_for_euclid_dist')                  # [P, Na, Nb]
    inf = torch.tensor(float('inf'), device=a.device)
    S = Na + Nb - 1
    i = torch.arange(Na, device=a.device)[None, :]
    j = torch.arange(S, device=a.device)[:, None] - i                                   # [S, Na]: column of row i on anti-diagonal s
    ok = (j >= 0) & (j < Nb)
    dsk = torch.where(ok[None], d.gather(2, j.clamp(0, Nb - 1).t()[None].expand(Pn, Na, S)).transpose(1, 2), inf)   # [P, S, Na]
    D = torch.full((Pn, S, Na), float('inf'), device=a.device)
    D[:, 0, 0] = dsk[:, 0, 0]
    pad = torch.full((Pn, 1), float('inf'), device=a.device)
    for s in range(1, S):
        p1 = D[:, s - 1]
        up = torch.cat([pad, p1[:, :-1]], dim=1)                                        # D(i-1, s-i)
        diag = torch.cat([pad, D[:, s - 2, :-1]], dim=1) if s > 1 else pad.expand(Pn, Na)
        D[:, s] = dsk[:, s] + torch.minimum(diag, torch.minimum(up, p1))
    return D[torch.arange(Pn, device=a.device), (la + lb - 2).long(), (la - 1).long()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from tests import dtw_reference as R
    from ttscube_amd.io_utils import evaluate as E
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)
    syn_frames = [int(v) for v in rng.integers(SYN_LO, SYN_HI + 1, P)]
    syn_frames[0], syn_frames[1] = SYN_HI, SYN_LO
    ref = np.stack([render(100 + p, REF_FRAMES) for p in range(P)])
    syn = np.zeros((P, SYN_HI * HOP), np.float32)
    for p in range(P):
        syn[p, :syn_frames[p] * HOP] = render(100 + p, syn_frames[p])
    ref_len, syn_len = [REF_FRAMES * HOP] * P, [n * HOP for n in syn_frames]
    X, Y = torch.from_numpy(ref).to(dev), torch.from_numpy(syn).to(dev)
    ev = E.Evaluator(dev)
    print('workload: %d pairs, reference %d frames, synthesized %d .. %d frames (seeded; mean %.0f), K = %d, hop %d at %d Hz; one MI355X, medians of %d'
          % (P, REF_FRAMES, min(syn_frames), max(syn_frames), float(np.mean(syn_frames)), K, HOP, SR, args.rounds))
    rm, rf, rn = ev.analyse(X, ref_len)
    sm, sf, sn = ev.analyse(Y, syn_len)
    a, b = E.mel_cepstra(rm, K), E.mel_cepstra(sm, K)
    res = ev.evaluate_audio(X, ref_len, Y, syn_len)
    c = res['corpus']
    print('scores of the workload : mcd_db %.3f  f0_rmse_hz %.2f  f0_rmse_cents %.1f  gpe %.4f  vde %.4f  dur_ratio %.4f  (path cells %d, both voiced %d)'
          % (c['mcd_db'], c['f0_rmse_hz'], c['f0_rmse_cents'], c['gpe'], c['vde'], c['dur_ratio'], c['n_path'], c['n_both_voiced']))
    t_dtw = gpu_median_ms(lambda: E.dtw_align(a, rn, b, sn), args.rounds)
    t_all = gpu_median_ms(lambda: ev.evaluate_audio(X, ref_len, Y, syn_len), args.rounds)
    audio_s = (sum(ref_len) + sum(syn_len)) / SR
    cells = sum(REF_FRAMES * n for n in syn_frames)
    blocks = -(-max(syn_frames) // 64)
    chain = blocks * (REF_FRAMES + 63)
    print('ttsc_dtw_align         : %8.3f ms   (%.2f G cells/s over %d cells; the longest pair walks %d column blocks x %d steps = %d dependent steps: '
          '%.0f ns per step)' % (t_dtw, cells / (t_dtw * 1e6), cells, blocks, REF_FRAMES + 63, chain, t_dtw * 1e6 / chain))
    print('evaluate_audio, whole  : %8.3f ms   (%.0f s of audio on both sides: %.0f x real time)' % (t_all, audio_s, audio_s / (t_all * 1e-3)))
    t_torch = gpu_median_ms(lambda: torch_dtw_cost(a, rn, b, sn), 3, warmup=1)
    out = E.dtw_align(a, rn, b, sn)
    rel = float(((torch_dtw_cost(a, rn, b, sn) - out['cost']).abs() / out['cost']).max())
    print('DP as torch ops        : %8.3f ms   (%.0f x ttsc_dtw_align; costs only, no path; max relative cost difference %.2e)' % (t_torch, t_torch / t_dtw, rel))
    ah, bh = a.cpu().numpy(), b.cpu().numpy()
    times = []
    for p in (0, 1):
        t0 = time.perf_counter()
        D, path = R.dtw(ah[p, :REF_FRAMES], bh[p, :syn_frames[p]], np.float64)
        times.append(time.perf_counter() - t0)
        same = np.array_equal(path[:, 0], out['path_a'][p, :len(path)].cpu().numpy()) and np.array_equal(path[:, 1], out['path_b'][p, :len(path)].cpu().numpy())
        print('  numpy float64, pair %d (%d x %d): %.2f s, cost %.4f (kernel %.4f), same path as the kernel: %s'
              % (p, REF_FRAMES, syn_frames[p], times[-1], D, float(out['cost'][p]), same))
    t_np = statistics.mean(times)
    print('DP in numpy, float64   : %8.0f ms per pair measured on 2 pairs; scaled to %d pairs (an extrapolation): %.0f s, %.0f x ttsc_dtw_align'
          % (t_np * 1e3, P, t_np * P, t_np * P * 1e3 / t_dtw))
    # one long pair, timed once
    N = 3000
    la_, lb_ = R.warp_pair(np.random.default_rng(3), N, N, K)
    A, B = torch.from_numpy(la_[None]).to(dev), torch.from_numpy(lb_[None]).to(dev)
    n1 = torch.tensor([N], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    big = E.dtw_align(A, n1, B, n1)
    e1.record()
    e1.synchronize()
    t_big = e0.elapsed_time(e1)
    chain = -(-N // 64) * (N + 63)
    print('one pair %d x %d, once: %8.3f ms   (%d dependent steps: %.0f ns per step; path length %d, cost %.3f)'
          % (N, N, t_big, chain, t_big * 1e6 / chain, int(big['plen'][0]), float(big['cost'][0])))


if __name__ == '__main__':
    main()
