#!/usr/bin/env python
"""Text in, wav out over the two-stage path (NOT in the reference): one sentence per line of --input -> <output-folder>/00001.wav, 00002.wav, ...
(int16 at the Textcoder yaml's sample rate) through ttscube_amd.api.TTSCubeTwoStage.

  --textcoder BASE   what scripts/train_textcoder.py writes: BASE.yaml / BASE.encodings / BASE.best (else BASE.last)
  --vocoder CKPT     a HiFi-GAN generator checkpoint (config.json beside it: scripts/train_hifigan.py), or the word `griffinlim` (no training needed)
  --phonemizer BASE  the front end's files (sentence phonemizer or word-level G2P); without it a line is read as phone symbols, `|` between words

Line i (from 0) is decoded with PreNet-dropout key --seed + i, so the files hold the same bytes at every --batch."""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parser():
    p = ArgumentParser(description='two-stage text-to-speech: Textcoder -> mel -> vocoder')
    p.add_argument('--textcoder', required=True, help='base path of the Textcoder files (.yaml / .encodings / .best or .last)')
    p.add_argument('--vocoder', required=True, help="HiFi-GAN generator checkpoint, or 'griffinlim'")
    p.add_argument('--phonemizer', default=None, help='base path of the phonemizer / G2P files (default: lines are phone strings)')
    p.add_argument('--input', required=True, help='text file, one sentence per line (empty lines are skipped)')
    p.add_argument('--output-folder', dest='output_folder', required=True)
    p.add_argument('--speaker', default='none')
    p.add_argument('--batch', type=int, default=32, help='sentences per padded batch')
    p.add_argument('--seed', type=int, default=0, help='line i is decoded with key seed + i')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--rate', type=float, default=1.0, help='speaking rate, > 1 is faster (duration scale 1 / rate, limited to [0.25, 4])')
    p.add_argument('--loudness', type=float, default=None, help='bring every sentence to this integrated loudness in LUFS (BS.1770-4; default: the '
                   'level the vocoder gives)')
    p.add_argument('--peak', type=float, default=-1.0, help='true-peak ceiling in dB for --loudness')
    p.add_argument('--markup', action='store_true', help='lines carry <prosody rate=..> / <break time=..> tags (ttscube_amd/io_utils/prosody.py)')
    return p


def read_sentences(path):
    with open(path, encoding='utf-8') as f:
        return [ln.strip() for ln in f if ln.strip()]


def check(params):
    if params.batch < 1:
        raise SystemExit('--batch must be at least 1 (got %d)' % params.batch)
    if not 0 <= params.seed < 2 ** 62:
        raise SystemExit('--seed must lie in [0, 2**62) (got %d)' % params.seed)
    return params


def main(argv=None):
    params = check(parser().parse_args(argv))
    texts = read_sentences(params.input)
    if not texts:
        raise SystemExit('%s holds no sentence' % params.input)
    from ttscube_amd.api import TTSCubeTwoStage
    from ttscube_amd.io_utils.audio import save_wav
    vocoder = params.vocoder
    if vocoder == 'griffinlim':
        import yaml
        from ttscube_amd.io_utils.vocoder import GriffinLimVocoder
        conf = yaml.load(open(params.textcoder + '.yaml'), yaml.Loader) or {}
        vocoder = GriffinLimVocoder(sample_rate=int(conf.get('sample_rate', 24000)), hop_size=int(conf.get('hop_size', 240)), device=params.device)
    tts = TTSCubeTwoStage(params.textcoder, vocoder, phonemizer_path=params.phonemizer, device=params.device)
    os.makedirs(params.output_folder, exist_ok=True)
    wavs = tts.synthesize_batch(texts, speaker=params.speaker, max_batch=params.batch, seed=params.seed, rate=params.rate, markup=params.markup,
                                loudness=params.loudness, peak_db=params.peak)
    for i, w in enumerate(wavs):
        save_wav(os.path.join(params.output_folder, '%05d.wav' % (i + 1)), w, tts.sample_rate)
    sys.stdout.write('%d files -> %s\n' % (len(wavs), params.output_folder))
    return 0


if __name__ == '__main__':
    sys.exit(main())
