#!/usr/bin/env python
"""Counterpart of the reference's scripts/train_textcoder.py (flags, files written), without pytorch_lightning, single process.

Files: <base>.yaml {sample_rate, pframes, hop_size}, <base>.encodings, <base>.best (CubenetTextcoder state_dict, selected on the DEV-set mel loss,
as the reference's callback does), <base>.last, <base>.opt.last (the optimizer's state_dict, torch.optim.Adam's layout).  --resume restores the
model AND the optimizer.  The reference synthesises the dev set with a hard-coded vocoder path; here that is the opt-in `--vocoder <g_ckpt>`
(every --epoch-generation epochs, through io_utils.runtime.synthesize_devset).

Data: `--train-folder` / `--dev-folder` hold the reference's processed corpus (<id>.json / .mgc / .pitch, io_utils.io_textcoder.TextcoderDataset).
With `--synthetic N` the folders are ignored and N seeded synthetic examples (+ N/4 for the dev set) are used instead — that must be asked for
explicitly: a missing or empty folder is an error.  Multi-GPU training is not built: WORLD_SIZE > 1 is refused."""
import os
import random
import sys
from argparse import ArgumentParser

import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd.io_utils.io_textcoder import TextcoderCollate, TextcoderDataset, TextcoderEncodings  # noqa: E402
from ttscube_amd.io_utils.loader import BatchLoader, equal_batches  # noqa: E402
from ttscube_amd.io_utils.synthetic import synthetic_examples  # noqa: E402
from ttscube_amd.networks.textcoder import CubenetTextcoder  # noqa: E402


def _check_world():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise SystemExit('train_textcoder.py trains on one process (WORLD_SIZE=%d): multi-GPU Textcoder training is not built; '
                         'run it without torch.distributed.run' % world)


def _data(params):
    if params.synthetic:
        return list(synthetic_examples(params.synthetic, 1234)), list(synthetic_examples(max(2, params.synthetic // 4), 4321))
    for folder in (params.train_folder, params.dev_folder):
        if not os.path.isdir(folder):
            raise SystemExit('%s does not exist (pass --synthetic N to train on synthetic examples)' % folder)
    trainset, devset = TextcoderDataset(params.train_folder), TextcoderDataset(params.dev_folder)
    if len(trainset) == 0 or len(devset) == 0:
        raise SystemExit('no <id>.json/.mgc/.pitch items under %s / %s' % (params.train_folder, params.dev_folder))
    return trainset, devset


def _train(params):
    _check_world()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    base = params.output_base
    yaml.dump({'sample_rate': params.sample_rate, 'pframes': params.pframes, 'hop_size': params.hop_size}, open(base + '.yaml', 'w'))
    trainset, devset = _data(params)
    sys.stdout.write('Training files: %d\nValidation files: %d\n' % (len(trainset), len(devset)))
    enc = TextcoderEncodings()
    if params.resume:
        enc.load(base + '.encodings')
    else:
        enc.compute(trainset)
        enc.save(base + '.encodings')
    sys.stdout.write('Number of speakers: %d\nNumber of phones: %d\nMaximum F0: %s\nMaximum duration: %s\n'
                     % (len(enc.speaker2int), len(enc.phon2int), enc.max_pitch, enc.max_duration))
    collate = TextcoderCollate(enc)
    model = CubenetTextcoder(enc, pframes=params.pframes, lr=params.lr)
    if params.resume:
        sys.stdout.write('Resuming from previous checkpoint\n')
        model.load(base + '.last')
        model._loaded_optimizer_state = torch.load(base + '.opt.last', map_location='cpu')
    model = model.to(dev)
    opt = model.optimizers()
    best = 99999.0
    for epoch in range(params.epochs):
        model.train()
        order = list(range(len(trainset)))
        random.Random(1000 * epoch).shuffle(order)
        loss_sum, nb, prev = 0.0, 0, None
        for batch in BatchLoader(trainset, equal_batches(order, params.batch_size), collate.collate_fn, params.num_workers):
            out = model.training_step(batch, nb)
            # the losses are read back when first looked at: look at the PREVIOUS step's after queueing this one
            if prev is not None:
                loss_sum += prev['loss']
            prev = out
            nb += 1
        if prev is not None:
            loss_sum += prev['loss']
        model.eval()
        outs = [model.validation_step(b, i) for i, b in
                enumerate(BatchLoader(devset, equal_batches(list(range(len(devset))), params.batch_size), collate.collate_fn, params.num_workers))]
        model.validation_epoch_end(outs)
        sys.stdout.write('\n\tepoch %d  train loss %.4f\n\tVal loss mel: %s\n\tVal loss pitch: %s\n\tVal loss dur: %s\n'
                         % (epoch, loss_sum / max(nb, 1), model._val_loss_mel, model._val_loss_pitch, model._val_loss_durs))
        if model._val_loss_mel < best:
            best = model._val_loss_mel
            sys.stdout.write('\tStoring %s.best\n' % base)
            model.save(base + '.best')
        model.save(base + '.last')
        torch.save(opt.state_dict(), base + '.opt.last')
        sys.stdout.write('\tStoring %s.last / %s.opt.last\n' % (base, base))
        sys.stdout.flush()
        if params.vocoder and epoch % params.epoch_generation == 0:
            from ttscube_amd.io_utils.runtime import load_generator_checkpoint, synthesize_devset
            sys.stdout.write('\tGenerating validation set\n')
            vocoder = load_generator_checkpoint(params.vocoder).to(dev)
            synthesize_devset(model, collate, devset, vocoder, output_path='generated_files/free/', forced_synthesis=False, limit=10)


def parser():
    p = ArgumentParser(description='CubenetTextcoder trainer (reference flags)')
    p.add_argument('--output-base', dest='output_base', default='data/textcoder')
    p.add_argument('--batch-size', dest='batch_size', default=16, type=int)
    p.add_argument('--num-workers', dest='num_workers', default=4, type=int)
    p.add_argument('--maximum-segment-size', dest='maximum_segment_size', type=int, default=24000, help='(accepted for compatibility; unused, as in the reference)')
    p.add_argument('--accelerator', dest='accelerator', default='gpu')
    p.add_argument('--devices', dest='devices', default=1, type=int)
    p.add_argument('--train-folder', dest='train_folder', default='data/processed/train')
    p.add_argument('--dev-folder', dest='dev_folder', default='data/processed/dev')
    p.add_argument('--sample-rate', dest='sample_rate', type=int, default=24000)
    p.add_argument('--hop-size', dest='hop_size', type=int, default=240)
    p.add_argument('--lr', dest='lr', default=2e-4, type=float)
    p.add_argument('--pframes', dest='pframes', type=int, default=3)
    p.add_argument('--epoch-generation', dest='epoch_generation', type=int, default=10,
                   help='synthesise the dev set every n-th epoch with --vocoder (files under generated_files/free)')
    p.add_argument('--vocoder', dest='vocoder', default=None, help='HiFi-GAN generator checkpoint (config.json beside it) for the dev-set synthesis; off by default')
    p.add_argument('--resume', dest='resume', action='store_true')
    p.add_argument('--epochs', type=int, default=1)
    p.add_argument('--synthetic', type=int, default=0, help='ignore the folders and train on N seeded synthetic examples')
    return p


if __name__ == '__main__':
    _train(parser().parse_args())
