"""HiFi-GAN trainer timings on one GPU (profiles/hifigan_train_bench.log).  Seeded synthetic data, no corpus; only these sizes are measured.

  (a) one `hifigan_training_step` (the trainer's loop body: gather launch + step) at b = 16 x 12 000 samples, full V1 generator, beside one
      `cubegan_training_step` at the same size (tools/bench_cubegan_step.py's batch): the two alternated round by round in this process, host clock
      around --iters steps that end in a device synchronise, median of the rounds
  (b) the gather launch alone (ttsc_segment_gather, index tensors already on the device) for b = 16 and b = 128, 50 frames, hop 240, with mel,
      against the same crops as torch slices + cat + permute + scale on the same GPU, alternated; device events around --launches back-to-back
      calls, so the figure is what one call costs in a stream of them — the host's enqueue through the Python wrapper (two torch.empty, one ctypes
      call) when that is longer than the kernel; the kernel's own time comes from a kernel trace in a run of its own.  Beside it the bytes the
      launch must move (2 B read + 4 B written per sample, 4 B + 4 B per mel element) as a rate, and that rate over the 8 TB/s HBM peak.
      The corpus (256 utterances of 4 s: 49 MB of audio, 33 MB of mel) fits the Infinity Cache, and a batch is 1.7 / 13 MB: the launch is a
      latency measurement more than a bandwidth one.  The two results must be equal bit for bit, or the tool fails.

    python tools/bench_hifigan_step.py [--rounds 5] [--iters 10] [--log profiles/hifigan_train_bench.log]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HOP, FRAMES, N_MELS, RATE = 240, 50, 80, 24000


def synthetic_items(n, seconds, seed):
    rng = np.random.RandomState(seed)
    L = int(seconds * RATE)
    out = []
    for _ in range(n):
        a = (9000 * np.sin(np.cumsum(rng.uniform(0.01, 0.3, size=L)))).astype(np.int16)
        out.append((a, np.clip(rng.randn(L // HOP + 1, N_MELS) - 2, -5, 1).astype(np.float32)))
    return out


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--log', default=None)
    args = ap.parse_args()
    from bench_cubegan_step import make_batch
    from ttscube_amd import _lib
    from ttscube_amd.hifigan.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from ttscube_amd.hifigan.env import AttrDict
    from ttscube_amd.hifigan.models import Generator
    from ttscube_amd.hifigan.train import hifigan_training_step
    from ttscube_amd.io_utils import segment_feed as SF
    from ttscube_amd.networks import training as T
    from ttscube_amd.networks.cubegan import Cubegan, _load_hifigan_config
    from ttscube_amd.optim import FlatAdamW
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    corpus = SF.SegmentCorpus(synthetic_items(256, 4.0, 7), HOP, N_MELS, dev)
    say('workload: seeded synthetic data, no corpus; corpus of %d utterances x 4 s (%.0f MB int16 audio, %.0f MB float32 mel); segments of %d frames '
        '= %d samples; only these sizes were measured' % (corpus.num, corpus.wav.numel() * 2 / 1e6, corpus.mel.numel() * 4 / 1e6, FRAMES, FRAMES * HOP))

    # ---- (a) ----
    B = 16
    batch, enc = make_batch(B, 40, np.random.RandomState(0))
    torch.manual_seed(0)
    model = Cubegan(enc, conditioning=None, train=True).cuda().train()
    opts = T.cubegan_configure_optimizers(model)
    r = random.Random(1)
    h = AttrDict(dict(_load_hifigan_config(), n_fft=1024, num_mels=80, sampling_rate=24000, hop_size=240, win_size=1024, fmin=0, fmax_for_loss=None))
    torch.manual_seed(0)
    gen, mpd, msd = Generator(h).cuda().train(), MultiPeriodDiscriminator().cuda().train(), MultiScaleDiscriminator().cuda().train()
    opt_g = FlatAdamW(list(gen.parameters()), 2e-4, betas=(0.8, 0.99))
    opt_d = FlatAdamW(list(msd.parameters()) + list(mpd.parameters()), 2e-4, betas=(0.8, 0.99))
    plan = list(SF.epoch_batches(1234, 0, corpus.n_frames, FRAMES, B))
    k = [0]

    def hifigan_step():
        utt, start = plan[k[0] % len(plan)]
        k[0] += 1
        y, mel = corpus.gather(utt, start, FRAMES, mel_scale=SF.LN10)
        return hifigan_training_step(gen, mpd, msd, opt_g, opt_d, y, mel, h)

    legs = [('cubegan_training_step', lambda: T.cubegan_training_step(model, batch, opts, rng=r)), ('gather + hifigan_training_step', hifigan_step)]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            t0 = time.perf_counter()
            for _ in range(args.iters):
                out = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.iters * 1e3)
            assert all(np.isfinite(v) for v in out.values()), out
    for name, _ in legs:
        say('(a) %-32s b=%d x %d samples: median %.1f ms/step over %d rounds of %d steps (rounds: %s)'
            % (name, B, FRAMES * HOP, statistics.median(times[name]), args.rounds, args.iters, ' '.join('%.1f' % t for t in times[name])))

    # ---- (b) ----
    wav_f = None
    for Bg in (16, 128):
        utt, start = next(SF.epoch_batches(99, 0, corpus.n_frames, FRAMES, Bg))
        idx = torch.from_numpy(np.stack([utt, start]).astype(np.int32)).to(dev)
        woff, moff = corpus.wav_off.tolist(), corpus.mel_off.tolist()
        gains = corpus.gain
        res = {}

        def kernel():
            res['k'] = SF.segment_gather(corpus.wav, corpus.wav_off, corpus.gain, corpus.mel, corpus.mel_off, idx[0], idx[1], FRAMES, HOP, N_MELS,
                                         SF.LN10, SF.MEL_PAD)

        def torch_ops():
            ys, ms = [], []
            for u, s in zip(utt.tolist(), start.tolist()):
                a = woff[u] + s * HOP
                ys.append((corpus.wav[a:a + FRAMES * HOP].float() * gains[u]).unsqueeze(0))
                ms.append(corpus.mel[moff[u] + s:moff[u] + s + FRAMES].unsqueeze(0))
            res['t'] = (torch.cat(ys, dim=0).unsqueeze(1), (torch.cat(ms, dim=0).permute(0, 2, 1) * np.float32(SF.LN10)).contiguous())

        for _ in range(3):
            kernel()
            torch_ops()
        torch.cuda.synchronize()
        if not (torch.equal(res['k'][0], res['t'][0]) and torch.equal(res['k'][1], res['t'][1])):
            raise SystemExit('bench_hifigan_step: the gather and the torch formulation differ at b=%d' % Bg)
        t_k, t_t = [], []
        for _ in range(args.rounds):
            t_k.append(event_ms(kernel, args.launches))
            t_t.append(event_ms(torch_ops, max(args.launches // 10, 1)))
        moved = Bg * (FRAMES * HOP * 6 + FRAMES * N_MELS * 8)
        mk, mt = statistics.median(t_k), statistics.median(t_t)
        say('(b) b=%-3d gather launch            : %8.4f ms median of %d rounds x %d launches (min %.4f, max %.4f); %.2f MB must move -> %.0f GB/s = '
            '%.1f %% of the 8 TB/s HBM peak' % (Bg, mk, args.rounds, args.launches, min(t_k), max(t_k), moved / 1e6, moved / (mk * 1e-3) / 1e9,
                                                 100.0 * moved / (mk * 1e-3) / 8e12))
        say('(b) b=%-3d torch slices + cat + permute + scale (%d launches of its own): %8.4f ms median (min %.4f, max %.4f), alternated; same bits; '
            '%.1f x the gather launch' % (Bg, 2 * Bg + 4, mt, min(t_t), max(t_t), mt / mk))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    json.dump({'step_ms': {n: statistics.median(t) for n, t in times.items()}}, sys.stdout)
    print()


if __name__ == '__main__':
    main()
