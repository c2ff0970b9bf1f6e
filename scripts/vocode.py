"""Mel features to audio through a trained CubenetVocoder (low- and high-resolution WaveRNN): every `<name>.mgc` (a bare np.save stream of
log10-mel [frames, 80], as the corpus importer and the Textcoder write them) becomes `<output-folder>/<name>.wav`, int16 at 24 kHz.

`--model <prefix>` names what scripts/train_vocoder.py wrote: `<prefix>.yaml` and `<prefix>.last` (or `<prefix>.lr.best` + `<prefix>.hr.best`).
`--batch N` sends N files at a time through CubenetVocoder.synthesize_batch (both nets as ragged rows of one launch).  File number i of the
sorted input is seeded with `--seed` + i, so the bytes written are the same at every `--batch`.

    python scripts/vocode.py --model data/models/vocoder --input data/processed/dev --output-folder generated_files/ --batch 16"""
import optparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def feature_files(inputs):
    out = []
    for p in inputs:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.endswith('.mgc')]
        else:
            out.append(p)
    return out


def load_vocoder(prefix, device):
    import torch
    import yaml

    from ttscube_amd.networks.vocoder import CubenetVocoder
    conf = yaml.safe_load(open(prefix + '.yaml'))
    model = CubenetVocoder(num_layers_lr=conf['num_layers_lr'], layer_size_lr=conf['layer_size_lr'], num_layers_hr=conf['num_layers_hr'],
                           layer_size_hr=conf['layer_size_hr'], upsample=conf['upsample'],
                           upsample_low=conf['sample_rate'] // conf['sample_rate_low'], output=conf['output'])
    if os.path.exists(prefix + '.last'):
        model.load(prefix + '.last')
    else:
        model._wavernn_lr.load(prefix + '.lr.best')
        model._wavernn_hr.load(prefix + '.hr.best')
    return model.to(torch.device(device)).eval()


def main(argv=None):
    parser = optparse.OptionParser()
    parser.add_option('--model', action='store', dest='model', help='CubenetVocoder prefix: <prefix>.yaml and <prefix>.last (or .lr.best / .hr.best)')
    parser.add_option('--input', action='append', dest='input', default=[], help='A .mgc file or a folder of them (may be given more than once)')
    parser.add_option('--output-folder', action='store', dest='output_folder', default='generated_files', help='Where the .wav files go')
    parser.add_option('--batch', type='int', dest='batch', default=16, help='Files per synthesize_batch call (default=16)')
    parser.add_option('--seed', type='int', dest='seed', default=0, help='Sampler seed; file i uses seed + i (default=0)')
    parser.add_option('--argmax', action='store_true', dest='argmax', default=False, help='No sampling noise: the mode of the output distribution')
    parser.add_option('--device', dest='device', default='cuda:0', help='HIP device (default=cuda:0)')
    params, rest = parser.parse_args(sys.argv[1:] if argv is None else argv)
    files = feature_files(params.input + rest)
    if not files or not params.model:
        parser.print_help()
        return 1
    if params.batch < 1:
        parser.error('--batch must be at least 1')
    import numpy as np

    from ttscube_amd.io_utils.audio import save_wav
    model = load_vocoder(params.model, params.device)
    os.makedirs(params.output_folder, exist_ok=True)
    for k in range(0, len(files), params.batch):
        group = files[k:k + params.batch]
        mels = [np.load(open(path, 'rb')).astype(np.float32) for path in group]   # [frames, num_mels] each
        pairs = model.synthesize_batch(mels, seed=[params.seed + k + i for i in range(len(group))], mode='argmax' if params.argmax else 'philox')
        for path, (_, x_hr) in zip(group, pairs):
            out = os.path.join(params.output_folder, os.path.splitext(os.path.basename(path))[0] + '.wav')
            save_wav(out, x_hr, 24000)
            print('%s -> %s (%d samples)' % (path, out, x_hr.shape[0]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
