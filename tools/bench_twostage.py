"""Two-stage text-to-speech (api.TTSCubeTwoStage): ONE synthesize_batch call against the loop of single-sentence calls, on seeded weights.

32 seeded sentences of 20 ... 120 phones go through a full-size CubenetTextcoder (fill_state_dict weights, 60 phones, max_duration 12, pframes 3)
and a HiFi-GAN V1 generator (synthetic weights).  The loop of ``tts(text, seed=s + i)`` and one ``tts.synthesize_batch(texts, seed=s)`` are
alternated in one process and their medians compared; a second alternated pass times text -> mel (CubenetTextcoder.inference_batch) and
mel -> audio (the generator) separately for both; a last line runs the same list at members = 4, max_rows = 64 — what the default, which keeps
every sentence on the split it gets alone (and with it the solo call's bits), costs in throughput.  ONLY THIS SIZE IS MEASURED; the weights are
random, so the durations (and with them the AR steps per sentence) are those of random logits, not of a trained model.

    python tools/bench_twostage.py [--rounds 5] [--sentences 32]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import hifigan_ref as R  # noqa: E402  (synthetic weights only)
from oracle import meldecoder_ref as M  # noqa: E402  (seeded weights only)
from ttscube_amd.api import TTSCubeTwoStage  # noqa: E402
from ttscube_amd.io_utils.io_textcoder import TextcoderEncodings  # noqa: E402
from ttscube_amd.networks.textcoder import CubenetTextcoder  # noqa: E402

N_PHONES, MAX_DUR = 60, 12


def model_dir(tmp):
    enc = TextcoderEncodings()
    enc.phon2int = {'p%d' % i: i for i in range(N_PHONES)}
    enc.speaker2int = {'a': 0, 'b': 1}
    enc.max_pitch, enc.max_duration = 300, MAX_DUR
    base = os.path.join(tmp, 'textcoder')
    enc.save(base + '.encodings')
    yaml.dump({'sample_rate': 24000, 'pframes': 3, 'hop_size': 240}, open(base + '.yaml', 'w'))
    torch.save(M.fill_state_dict(M.named_shapes(CubenetTextcoder(enc, pframes=3)), 2024), base + '.best')
    os.makedirs(os.path.join(tmp, 'vocoder'))
    torch.save({'generator': R.synthetic_state_dict(dict(R.CONFIG_V1), seed=55)}, os.path.join(tmp, 'vocoder', 'g_00000001'))
    open(os.path.join(tmp, 'vocoder', 'config.json'), 'w').write(json.dumps(dict(R.CONFIG_V1)))
    return base, os.path.join(tmp, 'vocoder', 'g_00000001')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sentences', type=int, default=32)
    ap.add_argument('--seed', type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_twostage: needs a GPU (no CPU path)')
    rng = np.random.RandomState(11)
    lens = [int(n) for n in rng.randint(20, 121, size=a.sentences)]
    texts = [' '.join('p%d' % p for p in rng.randint(0, N_PHONES, size=n)) for n in lens]
    spk = ['a' if i % 2 == 0 else 'b' for i in range(len(texts))]
    with tempfile.TemporaryDirectory() as tmp:
        tts = TTSCubeTwoStage(*model_dir(tmp))
    S0 = a.seed

    def loop():
        return [tts(t, speaker=p, seed=S0 + i) for i, (t, p) in enumerate(zip(texts, spk))]

    def batch(**kw):
        return tts.synthesize_batch(texts, speaker=spk, seed=S0, max_batch=len(texts), **kw)

    ref, got = loop(), batch()          # warm-up of both paths; what the batch computes against what the loop computes
    same = [bool(np.array_equal(r, g)) for r, g in zip(ref, got)]
    worst = max(int(np.abs(r.astype(np.int32) - g.astype(np.int32)).max()) if len(r) == len(g) and len(r) else (0 if len(r) == len(g) else -1)
                for r, g in zip(ref, got))
    stats = dict(tts.last_stats)
    frames = [(len(g) - 64) // 240 for g in got]
    print('only this size was measured: %d sentences of %d ... %d phones -> %d ... %d frames (%.1f s of audio), full-size Textcoder + V1 generator, '
          'random weights' % (len(texts), min(lens), max(lens), min(frames), max(frames), sum(len(g) for g in got) / 24000.0), flush=True)
    print('batch == loop, bit for bit: %d of %d sentences (largest int16 difference %d; -1 = another length)' % (sum(same), len(same), worst), flush=True)
    members = tts._model.ar_members(1)
    t_loop, t_batch, t_wide = [], [], []
    batch(members=4, max_rows=64)        # (warm-up of the wide launch shape)
    wide_stats = dict(tts.last_stats)
    for _ in range(a.rounds):
        t_loop.append(timed(loop)[0])
        t_batch.append(timed(batch)[0])
        t_wide.append(timed(lambda: batch(members=4, max_rows=64))[0])

    # the two stages separately, alternated the same way (these calls wait for the GPU between the stages: their sums exceed the lines above)
    phones = [tts._phones(t) for t in texts]
    order = sorted(range(len(texts)), key=lambda i: len(phones[i]))
    Xb = tts._collate([phones[i] for i in order], [spk[i] for i in order])
    Xs = [tts._collate([phones[i]], [spk[i]]) for i in range(len(texts))]
    st = {'loop_mel': [], 'loop_audio': [], 'batch_mel': [], 'batch_audio': []}
    with torch.no_grad():
        for _ in range(a.rounds):
            tm = ta = 0.0
            for i, X in enumerate(Xs):
                d, (mel, fr) = timed(lambda: tts._model.inference_batch(X, seeds=[S0 + i], channel_major=True))
                tm += d
                ta += timed(lambda: tts._vocode(mel, fr, 'sync'))[0]
            st['loop_mel'].append(tm)
            st['loop_audio'].append(ta)
            d, (mel, fr) = timed(lambda: tts._model.inference_batch(Xb, seeds=[S0 + i for i in order], channel_major=True))
            st['batch_mel'].append(d)
            st['batch_audio'].append(timed(lambda: tts._vocode(mel, fr, 'sync'))[0])
    med = statistics.median
    ml, mb, mw = med(t_loop), med(t_batch), med(t_wide)
    res = {'sentences': len(texts), 'phones': lens, 'frames': frames, 'audio_s': round(sum(len(g) for g in got) / 24000.0, 2), 'rounds': a.rounds,
           'bit_equal_sentences': sum(same), 'members_default': members, 'ar_launches': stats['launches'], 'longest_row_steps': stats['max_steps'],
           'loop_s': [round(t, 4) for t in t_loop], 'batch_s': [round(t, 4) for t in t_batch], 'loop_median_s': round(ml, 4),
           'batch_median_s': round(mb, 4), 'ratio': round(ml / mb, 2),
           'text_to_mel_s': {'loop': round(med(st['loop_mel']), 4), 'batch': round(med(st['batch_mel']), 4)},
           'mel_to_audio_s': {'loop': round(med(st['loop_audio']), 4), 'batch': round(med(st['batch_audio']), 4)},
           'members4_max_rows64': {'batch_s': [round(t, 4) for t in t_wide], 'batch_median_s': round(mw, 4), 'ratio_to_loop': round(ml / mw, 2),
                                   'ratio_to_default_batch': round(mb / mw, 2), 'ar_launches': wide_stats['launches']}}
    print('loop %.4f s, batch %.4f s, ratio %.2f  |  text -> mel: loop %.4f, batch %.4f  |  mel -> audio: loop %.4f, batch %.4f  |  '
          '%d AR launch(es) at %d members, longest row %d steps' % (ml, mb, ml / mb, med(st['loop_mel']), med(st['batch_mel']), med(st['loop_audio']),
                                                                  med(st['batch_audio']), stats['launches'], members, stats['max_steps']), flush=True)
    print('members = 4, max_rows = 64: batch %.4f s (%d AR launch(es)), ratio to the loop %.2f, to the default batch %.2f' % (
        mw, wide_stats['launches'], ml / mw, mb / mw), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
