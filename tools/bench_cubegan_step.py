"""One full `Cubegan.training_step` (cubegan.py:85-189) per iteration on synthetic data at config C4's per-GPU size
(b utterances, 50-frame / 12 000-sample crops): discriminator step + generator step + text step, four optimizers.
    python tools/bench_cubegan_step.py [--batch 16] [--iters 5]
    python tools/bench_cubegan_step.py --lm fasttext:xx [--rounds 3]    the word-conditioned step (seeded synthetic vectors, 12 words per sentence + a
                                                                        left / right context) and the unconditioned one, alternated in ONE process"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


NWORDS = 12


def make_batch(B, nph, rng, lm=None):
    from ttscube_amd.io_utils.io_cubegan import CubeganCollate, CubeganEncodings
    enc = CubeganEncodings()
    enc.phon2int = {str(i): i for i in range(50)}
    enc.speaker2int = {'a': 0}
    enc.max_pitch, enc.max_duration = 300, 10
    ex = []
    for b in range(B):
        durs = rng.randint(3, 9, size=nph)
        f2p = [p for p, d in enumerate(durs) for _ in range(d)]
        F_ = len(f2p)
        ex.append({'meta': {'phones': [str(v) for v in rng.randint(0, 50, size=nph)], 'speaker': 'a', 'frame2phon': f2p,
                            'phon2word': [0] * nph},
                   'mgc': np.clip(rng.randn(F_, 80) - 2, -5, 1), 'pitch': rng.randint(0, 300, size=F_).astype(np.float64),
                   'audio': rng.uniform(-0.5, 0.5, size=F_ * 240)})
    if lm is None:
        return CubeganCollate(enc).collate_fn(ex), enc
    # the SAME examples with words: NWORDS words over equal runs of phonemes, one word of context on either side
    from ttscube_amd.io_utils.word_vectors import WordVectors
    vocab = ['w%d' % i for i in range(200)]
    wr = np.random.RandomState(1)
    for e in ex:
        e['meta'].update(words=[vocab[i] for i in wr.randint(0, 200, size=NWORDS)], words_left=[vocab[wr.randint(200)]], words_right=[vocab[wr.randint(200)]],
                         phon2word=[p * NWORDS // nph for p in range(nph)])
    return CubeganCollate(enc, conditioning_type=lm, word_vectors=WordVectors.synthetic(vocab, dim=300, seed=2)).collate_fn(ex), enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--ragged', action='store_true', help="bench.py's batch: synthetic_examples(b, 777, min_ph=30, max_ph=50) through the class surface")
    ap.add_argument('--lm', default=None, help='fasttext:<lang>: time the word-conditioned step and the unconditioned one, alternated in this process')
    ap.add_argument('--rounds', type=int, default=3, help='with --lm: alternations (each times --iters steps of either model)')
    a = ap.parse_args()
    from ttscube_amd.networks.cubegan import Cubegan
    from ttscube_amd.networks import training as T
    if a.lm:
        return alternate(a, Cubegan, T)
    rng = np.random.RandomState(0)
    if a.ragged:
        from ttscube_amd.io_utils.io_cubegan import CubeganCollate
        from ttscube_amd.io_utils.synthetic import synthetic_encodings, synthetic_examples
        enc = synthetic_encodings()
        batch = CubeganCollate(enc).collate_fn(list(synthetic_examples(a.batch, 777, min_ph=30, max_ph=50)))
    else:
        batch, enc = make_batch(a.batch, 40, rng)
    torch.manual_seed(0)
    model = Cubegan(enc, conditioning=None, train=True).cuda()
    model.train()
    opts = T.cubegan_configure_optimizers(model)
    r = random.Random(1)
    step = (lambda: model.training_step(batch, 0, rng=r)) if a.ragged else (lambda: T.cubegan_training_step(model, batch, opts, rng=r))
    if a.ragged:
        model._optimizers = opts
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.iters
    print('cubegan training step  b=%d x 12000 samples: %.1f ms/step  %.2f M samples/s  losses %s' %
          (a.batch, dt * 1e3, a.batch * 12000 / dt / 1e6, {k: round(v, 4) for k, v in out.items()}), flush=True)


def alternate(a, Cubegan, T):
    legs = []
    for lm in (None, a.lm):
        batch, enc = make_batch(a.batch, 40, np.random.RandomState(0), lm)
        torch.manual_seed(0)
        model = Cubegan(enc, conditioning=lm, train=True).cuda().train()
        legs.append((lm or 'none', model, batch, T.cubegan_configure_optimizers(model), random.Random(1)))
    for _, model, batch, opts, r in legs:
        for _ in range(3):
            T.cubegan_training_step(model, batch, opts, rng=r)
    torch.cuda.synchronize()
    times = {name: [] for name, *_ in legs}
    for _ in range(a.rounds):
        for name, model, batch, opts, r in legs:
            t0 = time.perf_counter()
            for _ in range(a.iters):
                out = T.cubegan_training_step(model, batch, opts, rng=r)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
            assert all(np.isfinite(v) for v in out.values()), out
    for name, *_ in legs:
        ts = sorted(times[name])
        print('cubegan training step  b=%d x 12000 samples  conditioning=%-12s median %.1f ms/step  (rounds: %s)' %
              (a.batch, name, ts[len(ts) // 2], ' '.join('%.1f' % t for t in times[name])), flush=True)


if __name__ == '__main__':
    main()
