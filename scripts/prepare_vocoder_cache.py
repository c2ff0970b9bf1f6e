#!/usr/bin/env python
"""Fill the vocoder trainer's feature cache ahead of training: for every .wav of --train-folder and --dev-folder the files
`<cache-dir>/<path>.{mgc,audio,audio_low}.npy` that io_utils.io_vocoder.VocoderDataset would otherwise compute file by file inside the first epoch.
Both rate changes run on the HIP resampler and the spectrograms in one call per --batch files (VocoderDataset.precompute).

    python scripts/prepare_vocoder_cache.py --train-folder wavs/train --dev-folder wavs/dev
    python scripts/train_vocoder.py --train-folder wavs/train --dev-folder wavs/dev ..."""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = ArgumentParser(description='Precompute the vocoder feature cache on the GPU')
    p.add_argument('--train-folder', dest='train_folder', required=True)
    p.add_argument('--dev-folder', dest='dev_folder', required=True)
    p.add_argument('--batch', type=int, default=32, help='files per GPU call (default=32)')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--cache-dir', dest='cache_dir', default='data/cache')
    p.add_argument('--sample-rate', dest='sample_rate', type=int, default=24000)
    p.add_argument('--sample-rate-low', dest='sample_rate_low', type=int, default=2400)
    p.add_argument('--hop-size', dest='hop_size', type=int, default=240)
    params = p.parse_args(argv)
    if params.batch < 1:
        p.error('--batch must be at least 1')
    from ttscube_amd.io_utils.io_vocoder import VocoderDataset
    from ttscube_amd.io_utils.resample import Resampler
    from ttscube_amd.io_utils.vocoder import MelVocoder
    resampler, vocoder = Resampler(params.device), MelVocoder(params.device)
    for folder in (params.train_folder, params.dev_folder):
        if not os.path.isdir(folder):
            raise SystemExit('%s does not exist' % folder)
        ds = VocoderDataset(folder, target_sample_rate=params.sample_rate, lowres_sample_rate=params.sample_rate_low, hop_size=params.hop_size,
                            cache_dir=params.cache_dir)
        n = ds.precompute(batch=params.batch, device=params.device, resampler=resampler, mel_vocoder=vocoder)
        print('{0}: {1} files, {2} written to {3}'.format(folder, len(ds), n, params.cache_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
