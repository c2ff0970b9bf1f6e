"""What prosody control costs: one sentence and the 64-sentence batch of `bench.py --mode e2e` (same seeded model, same sentences),
synthesised three ways that alternate in one process on one GPU:

    uncontrolled      no control in the batch dict: the launches of the parent path
    rate+pitch        rate = 1.25 (duration scale 0.8) and pitch = +2 semitones: both controlled launches, no range
    rate+pitch+range  pitch_range = 1.3 on top: every workgroup of a voiced frame also forms its row's voiced mean

Each figure is the median over `--rounds` rounds of a host clock around `--reps` calls that end in a device synchronise.  The controlled
variants speak faster (fewer frames): their times are NOT comparable with the uncontrolled one as a cost of the controls alone; the line
`identity controls` (scale 1, multiplier 1, range 1 as tensors: the controlled kernels on the uncontrolled frame counts) is.
ONLY THESE SIZES ARE MEASURED; the weights are random.

    python tools/bench_prosody.py [--rounds 7] [--reps 20] [--variants uncontrolled,...] [--package-root DIR]

--package-root imports ttscube_amd (and oracle) from another checkout — the uncontrolled variant then runs on a commit without this feature,
for an A/B on the same box."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

VARIANTS = ('uncontrolled', 'identity controls', 'rate+pitch', 'rate+pitch+range')


def controls(variant, B, N):
    if variant == 'uncontrolled':
        return {}
    if variant == 'identity controls':
        return {'x_dur_scale': torch.ones((B, N), dtype=torch.float64), 'x_pitch_mul': torch.ones((B, N)), 'x_pitch_range': torch.ones((B,))}
    c = {'x_dur_scale': torch.full((B, N), 1.0 / 1.25, dtype=torch.float64), 'x_pitch_mul': torch.full((B, N), float(np.float32(2.0 ** (2.0 / 12.0))))}
    if variant == 'rate+pitch+range':
        c['x_pitch_range'] = torch.full((B,), 1.3)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20, help='calls per timed window')
    ap.add_argument('--variants', default=','.join(VARIANTS))
    ap.add_argument('--package-root', dest='package_root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    variants = [v for v in a.variants.split(',') if v]
    assert all(v in VARIANTS for v in variants), variants
    sys.path.insert(0, a.package_root)
    from oracle import hifigan_ref as R          # synthetic weights only
    from oracle import meldecoder_ref as MO
    from ttscube_amd.io_utils.synthetic import synthetic_sentences
    from ttscube_amd.networks.cubegan import Cubegan
    if not torch.cuda.is_available():
        raise SystemExit('bench_prosody: needs a GPU (no CPU path)')
    dev = torch.device('cuda', 0)

    class _Enc:                                  # (bench.py::bench_e2e's model)
        phon2int = {'p%d' % i: i for i in range(50)}
        speaker2int = {'s0': 0}
        max_pitch = 300
        max_duration = 12

    torch.manual_seed(0)
    tts = Cubegan(_Enc(), conditioning=None, train=False)
    sd = tts.state_dict()
    sd.update({'_languasito.' + k: v for k, v in MO.fill_state_dict(MO.named_shapes(tts._languasito), 5).items()})
    sd.update({'_generator.' + k: v for k, v in R.synthetic_state_dict(dict(R.CONFIG_V1), seed=1234).items()})
    tts.load_state_dict(sd)
    tts = tts.to(dev).eval()
    xc, lens = synthetic_sentences(64, seed=1234)
    order = sorted(range(64), key=lambda i: int(lens[i]))
    cases = {'single_sentence': xc[:1, :lens[0]], '64_sentences': xc[order][:, :int(max(lens))]}
    res = {'rounds': a.rounds, 'reps': a.reps, 'package_root': os.path.basename(os.path.abspath(a.package_root))}

    def call(x, variant):
        X = {'x_char': torch.from_numpy(np.ascontiguousarray(x)), 'x_speaker': torch.ones((x.shape[0], 1), dtype=torch.long)}
        X.update(controls(variant, *x.shape))
        with torch.no_grad():
            wav, wl = tts.inference(X, return_lengths=True, check='deferred')
        tts._generator.finish_range_check()
        return wav, wl

    for name, x in cases.items():
        frames, times = {}, {v: [] for v in variants}
        for v in variants:                       # warm-up of every variant's shapes
            for _ in range(3):
                wav, wl = call(x, v)
            frames[v] = int(sum((int(n) - 64) // 240 for n in wl))
        base = call(x, 'uncontrolled') if 'identity controls' in variants and 'uncontrolled' in variants else None
        if base is not None:
            ident = call(x, 'identity controls')
            same = list(base[1]) == list(ident[1]) and all(bool(torch.equal(base[0][b, 0, :n], ident[0][b, 0, :n])) for b, n in enumerate(base[1]))
            print('%s: identity controls == uncontrolled, bit for bit: %s' % (name, same), flush=True)
            res[name + '_identity_bit_equal'] = bool(same)
        for _ in range(a.rounds):
            for v in variants:                   # the variants alternate inside every round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call(x, v)
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) / a.reps)
        for v in variants:
            med = statistics.median(times[v])
            print('%-16s %-18s median %8.3f ms  (min %8.3f, max %8.3f over %d rounds of %d calls)  %6d frames' % (
                name, v, med * 1e3, min(times[v]) * 1e3, max(times[v]) * 1e3, a.rounds, a.reps, frames[v]), flush=True)
            res['%s/%s' % (name, v)] = {'median_ms': round(med * 1e3, 4), 'min_ms': round(min(times[v]) * 1e3, 4), 'max_ms': round(max(times[v]) * 1e3, 4),
                                        'frames': frames[v]}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
