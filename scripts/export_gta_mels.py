#!/usr/bin/env python
"""Write the ground-truth-aligned mels of a processed folder for vocoder fine-tuning (ttscube_amd/io_utils/gta.py): the trained Textcoder's
teacher-forced mel of every `<id>.json / .mgc / .pitch` item, as `<output-folder>/<id>.npy` (float32 [80, F], mel * ln 10: the generator's domain).

    python scripts/export_gta_mels.py --model data/textcoder --input-folder data/processed/train --output-folder gta/
    python scripts/train_hifigan.py --fine_tuning --input_mels_dir gta/ --processed-folder data/processed --config config.json ...

`--model` is the prefix scripts/train_textcoder.py writes (<prefix>.yaml, .encodings, .best; .last when there is no .best).  The files do not
depend on --batch; --seed fixes the PreNet's dropout masks."""
import os
import sys
from argparse import ArgumentParser

import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd.io_utils.gta import export_gta_mels  # noqa: E402
from ttscube_amd.io_utils.io_textcoder import TextcoderCollate, TextcoderDataset, TextcoderEncodings  # noqa: E402
from ttscube_amd.networks.textcoder import CubenetTextcoder  # noqa: E402


def parser():
    p = ArgumentParser(description='GTA mel export for HiFi-GAN fine-tuning')
    p.add_argument('--model', required=True, help='Textcoder prefix (train_textcoder.py --output-base)')
    p.add_argument('--input-folder', dest='input_folder', default='data/processed/train')
    p.add_argument('--output-folder', dest='output_folder', required=True)
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--seed', type=int, default=0)
    return p


def main(a):
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    conf = yaml.safe_load(open(a.model + '.yaml'))
    enc = TextcoderEncodings()
    enc.load(a.model + '.encodings')
    model = CubenetTextcoder(enc, pframes=int(conf.get('pframes', 3)))
    model.load(a.model + ('.best' if os.path.exists(a.model + '.best') else '.last'))
    model = model.to(dev)
    dataset = TextcoderDataset(a.input_folder)
    if len(dataset) == 0:
        raise SystemExit('no <id>.json/.mgc/.pitch items under %s' % a.input_folder)
    n = export_gta_mels(model, TextcoderCollate(enc), dataset, a.output_folder, batch=a.batch, seed=a.seed)
    sys.stdout.write('wrote %d files to %s\n' % (n, a.output_folder))


if __name__ == '__main__':
    main(parser().parse_args())
