#!/usr/bin/env python
"""Counterpart of the reference's scripts/train_phonemizer.py (flags, files written), without pytorch_lightning, single process.

It trains `CubenetPhonemizer`, the character tagger the runtime loads (io_utils.io_text.Text2FeatBlizzard) — the reference's script trains its
many-to-many variant, which nothing at run time reads — with one target per character (PhonemizerCollate(targets='aligned')).

Files: <base>.encodings, <base>.pacc.best / <base>.sacc.best (state_dicts selected on the dev set's phone / sentence accuracy), <base>.last.
Copy a checkpoint to <base>.model to use it: TTSCube(model_path, <base>) / Text2FeatBlizzard(<base>).
`--max-steps N` ends training after N steps (validation and the checkpoints still follow); `--epochs` bounds the epochs (the reference runs
until interrupted)."""
import os
import random
import sys
from argparse import ArgumentParser

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd import _lib  # noqa: E402
from ttscube_amd.io_utils.io_phonemizer import PhonemizerCollate, PhonemizerDataset, PhonemizerEncodings  # noqa: E402
from ttscube_amd.io_utils.loader import BatchLoader, equal_batches  # noqa: E402
from ttscube_amd.networks.phonemizer import CubenetPhonemizer, check_status  # noqa: E402


def _train(params):
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('train_phonemizer.py trains on one process; run it without torch.distributed.run')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    base = params.output_base
    trainset, devset = PhonemizerDataset(params.train_file), PhonemizerDataset(params.dev_file)
    sys.stdout.write('==================Data==================\nTraining examples: %d\nValidation examples: %d\n'
                     '========================================\n\n================Training================\n' % (len(trainset), len(devset)))
    enc = PhonemizerEncodings()
    enc.compute(trainset)
    enc.save(base + '.encodings')
    sys.stdout.write('Number of graphemes: %d\nNumber of phones: %d\n' % (len(enc.graphemes), len(enc.phonemes)))
    collate = PhonemizerCollate(enc, targets='aligned')
    model = CubenetPhonemizer(enc, lr=params.lr).to(dev)
    best_pacc = best_sacc = 0.0
    steps, epoch = 0, 0
    done = lambda: params.max_steps is not None and steps >= params.max_steps
    while not done() and (params.epochs is None or epoch < params.epochs):
        model.train()
        order = list(range(len(trainset)))
        random.Random(1000 * epoch).shuffle(order)
        losses = []
        for batch in BatchLoader(trainset, equal_batches(order, params.batch_size), collate.collate_fn, params.num_workers):
            losses.append(model.training_step(batch, steps))
            steps += 1
            if done():
                break
        train_loss = float(torch.stack(losses).mean()) if losses else 0.0      # ONE read-back per epoch
        check_status('train_phonemizer')
        _lib.check_split_status('train_phonemizer')
        model.eval()
        outs = [model.validation_step(b, i) for i, b in
                enumerate(BatchLoader(devset, equal_batches(list(range(len(devset))), params.batch_size), collate.collate_fn, params.num_workers))]
        model.validation_epoch_end(outs)
        sys.stdout.write('\n\n\tepoch %d  steps %d  train loss %.4f  val loss %.4f\n\tVal PACC: %s\n\tVal SACC: %s\n'
                         % (epoch, steps, train_loss, model._val_loss, model._val_pacc, model._val_sacc))
        if model._val_pacc > best_pacc:
            best_pacc = model._val_pacc
            sys.stdout.write('\tStoring %s.pacc.best\n' % base)
            model.save(base + '.pacc.best')
        if model._val_sacc > best_sacc:
            best_sacc = model._val_sacc
            sys.stdout.write('\tStoring %s.sacc.best\n' % base)
            model.save(base + '.sacc.best')
        sys.stdout.write('\tStoring %s.last\n' % base)
        model.save(base + '.last')
        sys.stdout.flush()
        epoch += 1


def parser():
    p = ArgumentParser(description='CubenetPhonemizer trainer (reference flags)')
    p.add_argument('--output-base', dest='output_base', default='data/phonemizer', help='Where to store the model (default=data/phonemizer)')
    p.add_argument('--batch-size', dest='batch_size', default=16, type=int)
    p.add_argument('--num-workers', dest='num_workers', default=4, type=int)
    p.add_argument('--accelerator', dest='accelerator', default='gpu', help='(accepted for compatibility; training runs on the HIP device)')
    p.add_argument('--devices', dest='devices', default=1, type=int)
    p.add_argument('--train-file', dest='train_file', default='data/blizzard-g2p.train')
    p.add_argument('--dev-file', dest='dev_file', default='data/blizzard-g2p.dev')
    p.add_argument('--lr', dest='lr', default=2e-4, type=float)
    p.add_argument('--epochs', type=int, default=None, help='stop after this many epochs (default: run until --max-steps or interrupted)')
    p.add_argument('--max-steps', dest='max_steps', type=int, default=None, help='stop after this many training steps')
    return p


if __name__ == '__main__':
    _train(parser().parse_args())
