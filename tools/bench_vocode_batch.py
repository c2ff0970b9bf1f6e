"""Batched WaveRNN vocoding against the loop of single-utterance calls, on seeded synthetic weights.

16 ragged utterances of 2 ... 4 s (200 ... 400 mel frames) go through a CubenetVocoder with H = 512 in both nets, once with one and once with
two GRU layers: the loop of ``_inference`` calls (one utterance per call, as the reference offers the vocoder) and ONE
``synthesize_batch`` call are alternated in one process and their medians compared.  Next to the times it prints the sequential decode steps
either way takes — the sum over the utterances of 24 T_i + L_hr,i for the loop, the longest row of every launch for the batch — which is
where the ratio comes from.  ONLY THIS SIZE IS MEASURED: 16 utterances, H = 512, mulaw head; nothing here says how other sizes behave.

    python tools/bench_vocode_batch.py [--rounds 3] [--utterances 16] [--H 512]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wavernn_ref as O  # noqa: E402  (synthetic weights only)
from ttscube_amd.networks.vocoder import CubenetVocoder  # noqa: E402


def vocoder(H, layers, output='mulaw'):
    voc = CubenetVocoder(num_layers_lr=layers, layer_size_lr=H, num_layers_hr=layers, layer_size_hr=H, upsample=240, upsample_low=10,
                         output=output)
    S = O.SAMPLE_SIZE[output]
    sd = {'_wavernn_hr.' + k: torch.from_numpy(v) for k, v in O.synthetic_state_dict(H=H, num_layers=layers, use_lowres=True, seed=1, S=S).items()}
    sd.update({'_wavernn_lr.' + k: torch.from_numpy(v)
               for k, v in O.synthetic_state_dict(H=H, num_layers=layers, use_lowres=False, seed=2, S=S).items()})
    voc.load_state_dict(sd, strict=True)
    return voc.cuda().eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--utterances', type=int, default=16)
    ap.add_argument('--H', type=int, default=512)
    ap.add_argument('--min-frames', type=int, default=200)
    ap.add_argument('--max-frames', type=int, default=400)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vocode_batch: needs a GPU (no CPU path)')
    rng = np.random.RandomState(7)
    Ts = [int(t) for t in rng.randint(a.min_frames, a.max_frames + 1, size=a.utterances)]
    mels = [np.clip(rng.randn(T, 80) - 2.0, -5.0, 1.0).astype(np.float32) for T in Ts]
    print('only this size was measured: %d utterances of %d ... %d frames (%.1f s of audio), H = %d, mulaw head' % (
        len(Ts), min(Ts), max(Ts), sum(Ts) / 100.0, a.H), flush=True)
    for layers in (1, 2):
        voc = vocoder(a.H, layers)

        def loop():
            return [voc._inference({'mel': torch.from_numpy(m[None])}, seed=100 + i) for i, m in enumerate(mels)]

        def batch():
            return voc.synthesize_batch(mels, seed=100)

        ref = loop()      # warm-up of both paths, and the check that the batch computes what the loop computes
        got = batch()
        for i in range(len(mels)):
            assert np.array_equal(ref[i][0][0, :, 0], got[i][0]) and np.array_equal(ref[i][1][0], got[i][1]), 'utterance %d differs' % i
        t_loop, t_batch = [], []
        for _ in range(a.rounds):
            t_loop.append(timed(loop)[0])
            t_batch.append(timed(batch)[0])
        plan = voc.last_plan
        steps_batch, steps_loop = plan.steps()
        ml, mb = statistics.median(t_loop), statistics.median(t_batch)
        res = {'layers': layers, 'H': a.H, 'utterances': len(Ts), 'frames': Ts, 'audio_s': sum(Ts) / 100.0,
               'loop_s': [round(t, 4) for t in t_loop], 'batch_s': [round(t, 4) for t in t_batch], 'loop_median_s': round(ml, 4),
               'batch_median_s': round(mb, 4), 'ratio': round(ml / mb, 2), 'steps_loop': steps_loop, 'steps_batch': steps_batch,
               'steps_ratio': round(steps_loop / steps_batch, 2), 'hr_rows': len(plan.rows), 'hr_launches': [len(l) for l in plan.launches],
               'longest_row_per_launch': [max(plan.rows[k].out_len for k in l) for l in plan.launches],
               'kernel': {'lr': voc._wavernn_lr.last_kernel, 'hr': voc._wavernn_hr.last_kernel},
               'us_per_step_loop': round(ml / steps_loop * 1e6, 2), 'us_per_step_batch': round(mb / steps_batch * 1e6, 2)}
        print('%d layer(s): loop %.3f s, batch %.3f s, ratio %.2f  |  steps: loop %d, batch %d (ratio %.2f)  |  %d rows in launches of %s, %s kernel' % (
            layers, ml, mb, ml / mb, steps_loop, steps_batch, steps_loop / steps_batch, len(plan.rows), res['hr_launches'], res['kernel']['hr']),
            flush=True)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
