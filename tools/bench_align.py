"""Forced-aligner timings on one GPU (profiles/align_bench.log).

Workload: 64 seeded utterances of the synthetic phones of tests/forced_align_signals.py at 24 kHz, about 8 s and about 100 phones each (words from
its lexicon until 100 phones are reached, 40 - 95 ms per phone, a 100 - 250 ms silence at both ends and behind every sixth word), hop 240,
3 sub-states per phone, 26 features.  Only this size is measured.  Medians over rounds of
  * the Viterbi launch alone (ttsc_fa_viterbi: all 64 utterances, device input to device output);
  * the accumulate call alone (ttsc_fa_accumulate: its two launches);
  * one whole iteration of ForcedAligner.fit as fit runs it (two batches of 32: search, statistics, the copies to the host, re-estimation);
and two comparators for the search:
  * the same recurrence as torch ops on the same GPU: batched emissions (three matrix products and a gather), then a per-frame loop of
    torch.maximum over the three predecessors (scores only: it keeps no back-pointers and walks no path);
  * the float32 numpy restatement (tests/forced_align_reference.py) on the host, timed on two utterances; its batch figure is that time scaled
    to 64 utterances — an extrapolation, not a measurement.

    python tools/bench_align.py [--rounds 7] [--log profiles/align_bench.log]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N_PHONES, N_SUB, SR, HOP = 64, 100, 3, 24000, 240


def utterance(rng, S):
    names = list(S.LEXICON)
    words, n = [], 0
    while n < N_PHONES:
        words.append(names[int(rng.integers(len(names)))])
        n += len(S.LEXICON[words[-1]])
    ms = SR // 1000
    sil = lambda: 0.002 * rng.standard_normal(int(rng.integers(100, 251)) * ms)
    parts = [sil()]
    for k, w in enumerate(words):
        parts += [S._phone(p, int(rng.integers(40, 96)) * ms, rng) for p in S.LEXICON[w]]
        if k % 6 == 5:
            parts.append(sil())
    parts.append(sil())
    x = np.concatenate(parts)
    return dict(audio=(x + 0.0005 * rng.standard_normal(len(x))).astype(np.float32), words=[w.lower() for w in words],
                prons=[S.LEXICON[w] for w in words], n_phones=n)


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


def torch_viterbi_scores(feat, nframes, lat, mean, ivar, cst):
    """the recurrence with torch ops: score [B] only (the best final position at every utterance's own last frame)"""
    Bn, T, D = feat.shape
    S_ = lat['state'].shape[1]
    quad = (feat * feat) @ ivar.t() - 2.0 * (feat @ (mean * ivar).t()) + ((mean * mean) * ivar).sum(1)           # [B, T, M]
    e_m = cst - 0.5 * quad
    valid = torch.arange(S_, device=feat.device)[None, :] < lat['npos'][:, None]
    st = lat['state'].clamp(min=0).long()
    e = torch.gather(e_m, 2, st[:, None, :].expand(Bn, T, S_))                                                     # [B, T, S]
    ninf = torch.tensor(float('-inf'), device=feat.device)
    e = torch.where(valid[:, None, :], e, ninf)
    sk = lat['skip'].clamp(min=0).long()
    has = (lat['skip'] >= 0) & valid
    pad = torch.full((Bn, 1), float('-inf'), device=feat.device)
    v = torch.where(lat['start'] != 0, e[:, 0], ninf)
    fin = (lat['final'] != 0) & valid
    score = torch.where(nframes == 1, torch.where(fin, v, ninf).max(1).values, torch.full((Bn,), float('-inf'), device=feat.device))
    for t in range(1, T):
        left = torch.cat([pad, v[:, :-1]], dim=1)
        jump = torch.where(has, torch.gather(v, 1, sk), ninf)
        v = e[:, t] + torch.maximum(v, torch.maximum(left, jump))
        score = torch.where(nframes == t + 1, torch.where(fin, v, ninf).max(1).values, score)
    return score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'align_bench.log'))
    args = ap.parse_args()
    from tests import forced_align_reference as R
    from tests import forced_align_signals as S
    from ttscube_amd.io_utils import forced_align as FA
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)
    items = [utterance(rng, S) for _ in range(B)]
    aligner = FA.ForcedAligner(S.PHONES, n_sub=N_SUB, device=dev)
    t0 = time.perf_counter()
    history = aligner.fit(items, iterations=2, batch=32)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    whole = next(aligner._batches(items, B))
    feat, nf, lat = whole['feat'], whole['nframes'], whole['lat']
    T, S_ = feat.shape[1], lat['state'].shape[1]
    frames, npos = nf.cpu().numpy(), lat['npos'].cpu().numpy()
    say('workload: %d utterances, %.2f .. %.2f s (mean %.2f), %d .. %d phones, %d .. %d frames, %d .. %d lattice positions, D = %d, M = %d; one MI355X, '
        'medians of %d' % (B, min(len(i['audio']) for i in items) / SR, max(len(i['audio']) for i in items) / SR,
                           float(np.mean([len(i['audio']) for i in items])) / SR, min(i['n_phones'] for i in items), max(i['n_phones'] for i in items),
                           frames.min(), frames.max(), npos.min(), npos.max(), aligner.D, aligner.M, args.rounds))
    say('fit, flat start + 2 iterations, first call (features, uploads and code loading included): %.0f ms; score per frame %s; infeasible %d'
        % (t_fit * 1e3, ' -> '.join('%.3f' % (h['score'] / h['frames']) for h in history), len(history[-1]['infeasible'])))
    mean, ivar, cst = aligner._model()
    out = FA.viterbi(feat, nf, lat, mean, ivar, cst)
    cells = int((frames.astype(np.int64) * npos).sum())
    t_vit = gpu_median_ms(lambda: FA.viterbi(feat, nf, lat, mean, ivar, cst), args.rounds)
    say('ttsc_fa_viterbi         : %8.3f ms   (%.2f G cells/s over %d cells; the longest utterance runs %d dependent frames: %.0f ns per frame, '
        'barrier, emissions of its tile and walk back included)' % (t_vit, cells / (t_vit * 1e6), cells, frames.max(), t_vit * 1e6 / frames.max()))
    tables = aligner._tables()
    t_acc = gpu_median_ms(lambda: FA.accumulate(feat, nf, out['align'], out['ok'], lat, *tables), args.rounds)
    say('ttsc_fa_accumulate      : %8.3f ms   (%d aligned frames into %d x %d float64 tables)' % (t_acc, int(frames[out['ok'].cpu().numpy() != 0].sum()),
                                                                                                  aligner.M, aligner.D))
    batches = list(aligner._batches(items, 32))

    def iteration():
        m = aligner._model()
        tb = aligner._tables()
        for bt in batches:
            o = FA.viterbi(bt['feat'], bt['nframes'], bt['lat'], *m)
            FA.accumulate(bt['feat'], bt['nframes'], o['align'], o['ok'], bt['lat'], *tb)
            o['ok'].cpu(), o['score'].cpu()
        FA.reestimate(tb[0].cpu().numpy(), tb[1].cpu().numpy(), tb[2].cpu().numpy(), aligner.mean, aligner.var, aligner.floor)

    times = []
    for k in range(args.rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iteration()
        torch.cuda.synchronize()
        if k >= 2:
            times.append((time.perf_counter() - t0) * 1e3)
    audio_s = sum(len(i['audio']) for i in items) / SR
    say('one fit iteration, whole: %8.3f ms   (host clock; two batches of 32, features kept on the device: %.0f s of audio, %.0f x real time)'
        % (statistics.median(times), audio_s, audio_s / (statistics.median(times) * 1e-3)))
    t_torch = gpu_median_ms(lambda: torch_viterbi_scores(feat, nf, lat, mean, ivar, cst), 3, warmup=1)
    ts = torch_viterbi_scores(feat, nf, lat, mean, ivar, cst)
    rel = float(((ts - out['score']).abs() / out['score'].abs()).max())
    say('recurrence as torch ops : %8.3f ms   (%.0f x ttsc_fa_viterbi; scores only, no path; max relative score difference %.2e)'
        % (t_torch, t_torch / t_vit, rel))
    fh, al = feat.cpu().numpy(), out['align'].cpu().numpy()
    km = [a.cpu().numpy() for a in (mean, ivar, cst)]
    times = []
    for b in (0, 1):
        l = {k: lat[k][b, :npos[b]].cpu().numpy() for k in ('state', 'skip', 'start', 'final')}
        t0 = time.perf_counter()
        a32, s32, ok = R.viterbi(fh[b, :frames[b]], l, *km, np.float32)
        times.append(time.perf_counter() - t0)
        say('  numpy float32, utterance %d (%d frames x %d positions): %.3f s, score %.3f (kernel %.3f), same path as the kernel: %s'
            % (b, frames[b], npos[b], times[-1], float(s32), float(out['score'][b]), bool(ok) and np.array_equal(a32, al[b, :frames[b]])))
    t_np = statistics.mean(times)
    say('search in numpy, float32: %8.0f ms per utterance measured on 2 utterances; scaled to %d utterances (an extrapolation): %.1f s, %.0f x '
        'ttsc_fa_viterbi' % (t_np * 1e3, B, t_np * B, t_np * B * 1e3 / t_vit))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
