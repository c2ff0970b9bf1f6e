#!/usr/bin/env python
"""Narrate a text file with ttscube_amd.story.StoryCube: paragraphs separated by a blank line in, one 24 kHz int16 wav with looped background
music and a JSON list of per-paragraph timestamps out.  The reference has no command line for cube/story.py; this is a thin wrapper around the
class (save_wav + json.dump).

    python scripts/story.py --model en-neural --text-file story.txt --output story.wav --meta story.json
    python scripts/story.py --model-path models/cubegan --phonemizer-path models/phonemizer --music bed.wav --text-file story.txt --output story.wav"""
import json
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = ArgumentParser(description='Several paragraphs -> one narrated track with background music (StoryCube)')
    p.add_argument('--model', help='a model under ~/.ttscube/models/NAME (its music.wav is the default background)')
    p.add_argument('--model-path', dest='model_path', help='BASE of BASE.{model,yaml,encodings} instead of --model')
    p.add_argument('--phonemizer-path', dest='phonemizer_path', help='BASE of the phonemizer files (with --model-path)')
    p.add_argument('--text-file', dest='text_file', required=True, help='UTF-8 text, paragraphs separated by a blank line')
    p.add_argument('--speaker', default=None)
    p.add_argument('--music', help='background music wav (required with --model-path; with --model it replaces music.wav)')
    p.add_argument('--output', required=True, help='out.wav (int16, 24 kHz)')
    p.add_argument('--meta', help='out.json: the timestamp list')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--rate', type=float, default=1.0, help='speaking rate, > 1 is faster (duration scale 1 / rate, limited to [0.25, 4])')
    p.add_argument('--pitch', type=float, default=0.0, help='pitch shift in semitones (moves the pitch input of the conditioning recurrence)')
    p.add_argument('--pitch-range', dest='pitch_range', type=float, default=1.0, help="factor on the spread of the pitch around each paragraph's voiced mean")
    p.add_argument('--loudness', type=float, default=None, help='bring every paragraph to this integrated loudness in LUFS before the mix (BS.1770-4; '
                   'default: the level the generator gives)')
    p.add_argument('--markup', action='store_true', help='paragraphs carry <prosody ..> / <break time=..> tags (ttscube_amd/io_utils/prosody.py)')
    p.add_argument('--max-batch', dest='max_batch', type=int, default=16, help='paragraphs per padded batch (default=16)')
    params = p.parse_args(argv)
    if (params.model is None) == (params.model_path is None):
        p.error('give either --model NAME or --model-path BASE')
    if params.model_path is not None and params.music is None:
        p.error('--model-path needs --music (only a model under ~/.ttscube/models brings its own music.wav)')
    if params.max_batch < 1:
        p.error('--max-batch must be at least 1')
    from ttscube_amd.io_utils.audio import save_wav
    from ttscube_amd.story import StoryCube
    cube = None
    if params.model_path is not None:
        from ttscube_amd.api import TTSCube
        cube = TTSCube(params.model_path, params.phonemizer_path, device=params.device)
    story = StoryCube(params.model, cube=cube, music=params.music, device=params.device, max_batch=params.max_batch)
    with open(params.text_file, encoding='utf-8') as f:
        text = f.read()
    result = story(text, speaker=params.speaker, rate=params.rate, pitch=params.pitch, pitch_range=params.pitch_range, markup=params.markup,
                   loudness=params.loudness)
    save_wav(params.output, result['audio'], 24000)
    if params.meta:
        with open(params.meta, 'w') as f:
            json.dump(result['meta'], f, indent=1)
    print('{0}: {1:.1f} s, {2} paragraphs'.format(params.output, len(result['audio']) / 24000, len(result['meta']) - 1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
