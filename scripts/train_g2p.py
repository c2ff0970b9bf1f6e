#!/usr/bin/env python
"""Counterpart of the training mode of the reference's cube/networks/g2p.py (its flags, its files, its patience loop) on the HIP training path
(ttscube_amd/networks/g2p_train.py).

    python scripts/train_g2p.py --train-file TRAIN --dev-file DEV --store BASE [--batch-size 32] [--lr 1e-3] [--patience 20] [--load BASE]

Files: BASE.encodings at start, BASE.last after every epoch, BASE.best whenever the dev set's word accuracy improves.  `--load BASE` continues from
BASE.last with that model's accuracy as the baseline.  Text2Feat / G2P.load read BASE.best.

Deviation from the reference: batches include the last partial one and are never empty — the reference's _get_batches drops everything below one
batch and appends an empty batch on exact multiples of the batch size (G2P.evaluate documents the same deviation).  A run from scratch stores its
first epoch as BASE.best whatever its accuracy: its baseline is -1 where the reference's is 0.  With the reference's baseline a model that scores 0 on
the dev set (the usual state of the first epochs) is never stored, G2P.load finds no BASE.best, and the patience counter runs down before anything
loadable exists — under `--patience 1` the run ends after one epoch with nothing but BASE.last.  From the second epoch on the loop is the reference's.
Additions: --seed (shuffling and dropout masks; a run is repeatable), --max-epochs / --max-steps (bounded runs; the files are still written)."""
import os
import random
import sys
from argparse import ArgumentParser

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd.networks.g2p import G2P, G2PDataset  # noqa: E402
from ttscube_amd.networks.g2p_train import g2p_configure_optimizer, g2p_training_step  # noqa: E402
from ttscube_amd.networks.seq2seq import check_status  # noqa: E402

# (flag, dest, default, type or None for a switch, help): the reference's options for this mode, under its names
REFERENCE_FLAGS = [
    ('--patience', 'patience', 20, int, 'Num epochs without improvement (default=20)'),
    ('--train-file', 'train_file', None, str, 'Training file for g2p'),
    ('--dev-file', 'dev_file', None, str, 'Validation file for g2p'),
    ('--store', 'output_path', None, str, 'Base path for storing output model'),
    ('--batch-size', 'batch_size', 32, int, 'number of samples in a single batch (default=32)'),
    ('--resume', 'resume', False, None, 'Resume from previous checkpoint'),
    ('--device', 'device', 'cuda:0', str, None),
    ('--lr', 'lr', 1e-3, float, None),
    ('--load', 'model_path', None, str, None),
]
EXTRA_FLAGS = [
    ('--seed', 'seed', 1234, int, 'seed of the shuffling and of the dropout masks'),
    ('--max-epochs', 'max_epochs', None, int, 'stop after this many epochs'),
    ('--max-steps', 'max_steps', None, int, 'stop after this many training steps'),
]


def get_batches(examples, batch_size):
    return [examples[s:s + batch_size] for s in range(0, len(examples), batch_size)]


def _train(params):
    train, dev = G2PDataset(params.train_file), G2PDataset(params.dev_file)
    g2p = G2P()
    rng = random.Random(params.seed)
    torch.manual_seed(params.seed)
    if not params.model_path:
        g2p.update_encodings(train)
        g2p.initialize_network()
        g2p.save(params.output_path)
        g2p.to(params.device)
        best_acc = -1.0          # (the reference starts at 0: a model that scores 0 on the dev set would never be stored and BASE.best never exist)
    else:
        g2p.load(params.model_path, load_last=True)
        g2p.save(params.output_path)
        g2p.to(params.device)
        g2p.eval()
        best_acc = g2p.evaluate(dev)
        sys.stdout.write('Setting baseline accuracy to {0:.4f}\n'.format(best_acc))
    opt = g2p_configure_optimizer(g2p, lr=params.lr)
    patience_left = params.patience
    epoch, steps = 1, 0
    g2p.seq2seq.save('{0}.last'.format(params.output_path))
    done = lambda: params.max_steps is not None and steps >= params.max_steps
    while patience_left > 0 and not done() and (params.max_epochs is None or epoch <= params.max_epochs):
        g2p.train()
        patience_left -= 1
        sys.stdout.write('\n\nStarting epoch {0}\n'.format(epoch))
        rng.shuffle(train.examples)
        losses = []
        for batch in get_batches(train.examples, params.batch_size):
            losses.append(g2p_training_step(g2p, batch, opt))
            steps += 1
            if done():
                break
        total_loss = sum(l['loss'] for l in losses) / len(losses)          # read back once per epoch
        check_status('train_g2p')
        sys.stdout.write('\tAvg loss: {0}\n'.format(total_loss))
        g2p.eval()
        acc = g2p.evaluate(dev)
        sys.stdout.write('\tDevset accuracy: {0}\n'.format(acc))
        if acc > best_acc:
            best_acc = acc
            sys.stdout.write('\tStoring {0}.best\n'.format(params.output_path))
            g2p.seq2seq.save('{0}.best'.format(params.output_path))
            patience_left = params.patience
        sys.stdout.write('\tStoring {0}.last\n'.format(params.output_path))
        g2p.seq2seq.save('{0}.last'.format(params.output_path))
        sys.stdout.flush()
        epoch += 1


def parser():
    p = ArgumentParser(description='G2P trainer (reference flags)')
    for flag, dest, default, typ, hlp in REFERENCE_FLAGS + EXTRA_FLAGS:
        if typ is None:
            p.add_argument(flag, dest=dest, action='store_true', help=hlp)
        else:
            p.add_argument(flag, dest=dest, default=default, type=typ, help=hlp)
    return p


if __name__ == '__main__':
    args = parser().parse_args()
    if not (args.train_file and args.dev_file and args.output_path):
        parser().error('--train-file, --dev-file and --store are required')
    _train(args)
