#!/usr/bin/env python
"""HiFi-GAN vocoder trainer with the public trainer's flags and files (ttscube_amd/hifigan/train.py), single GPU.

Files: `<checkpoint_path>/config.json` (a copy of --config: io_utils.runtime.load_generator_checkpoint looks for it beside the generator file),
`g_%08d` = {'generator': state_dict with weight_g / weight_v}, `do_%08d` = {'mpd', 'msd', 'optim_g', 'optim_d', 'steps', 'epoch'} and
`validation.log`.  Start-up resumes from the latest `g_` / `do_` pair in the folder; a run resumed in the middle of an epoch draws the crops the
uninterrupted run would have drawn.

Data: `--input_training_file` / `--input_validation_file` (`name|text` lines, wavs under --input_wavs_dir) or `--processed-folder data/processed`
(its train/ and dev/ folders).  `--input-features audio` (default) trains on the generator's own mel of each crop, `mgc` on the corpus's
`<id>.mgc` rows, `gta` — implied by `--fine_tuning` — on `<input_mels_dir>/<id>.npy` written by scripts/export_gta_mels.py."""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd.hifigan.train import train  # noqa: E402


def parser():
    p = ArgumentParser(description='HiFi-GAN trainer (public flags)')
    p.add_argument('--group_name', default=None, help='(accepted for compatibility; unused)')
    p.add_argument('--input_wavs_dir', default='LJSpeech-1.1/wavs')
    p.add_argument('--input_mels_dir', default='ft_dataset')
    p.add_argument('--input_training_file', default=None)
    p.add_argument('--input_validation_file', default=None)
    p.add_argument('--processed-folder', dest='processed_folder', default=None, help='data/processed: train/ and dev/ replace the two file lists')
    p.add_argument('--checkpoint_path', default='cp_hifigan')
    p.add_argument('--config', default='')
    p.add_argument('--training_epochs', default=3100, type=int)
    p.add_argument('--stdout_interval', default=5, type=int)
    p.add_argument('--checkpoint_interval', default=5000, type=int)
    p.add_argument('--summary_interval', default=100, type=int, help='(accepted for compatibility; unused: no tensorboard writer)')
    p.add_argument('--validation_interval', default=1000, type=int)
    p.add_argument('--fine_tuning', default=False, type=lambda v: str(v).lower() in ('1', 'true', 'yes'), nargs='?', const=True)
    p.add_argument('--input-features', dest='input_features', default='audio', choices=('audio', 'mgc', 'gta'))
    return p


if __name__ == '__main__':
    train(parser().parse_args())
