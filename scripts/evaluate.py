"""Score a synthesized dev set against its recordings (io_utils/evaluate.py): DTW over mel cepstra on the GPU, then a mel-cepstral distortion and
F0 / voicing figures per item and pooled over the corpus.  The synthesized side is a folder of <id>.wav files, or a Cubegan checkpoint that is run
here (the audio then stays on the device).  The MCD is over this project's 80-bin log-mel: comparable between runs of this tool, not with papers.

    python scripts/evaluate.py --devset data/processed/dev --generated generated_files/free --output metrics.json
    python scripts/evaluate.py --devset data/processed/dev --model data/models/cubegan --batch 32 --output metrics.json"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def build_parser():
    p = argparse.ArgumentParser(description='Objective dev-set evaluation: DTW-aligned mel-cepstral distortion and F0 / voicing errors')
    p.add_argument('--devset', required=True, help='Processed dev folder (<id>.json / .mgc / .pitch / .wav)')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--generated', help='Folder of synthesized <id>.wav files')
    src.add_argument('--model', help='Cubegan checkpoint prefix: <prefix>.encodings and <prefix>.best / .model / .last; the dev set is synthesized here')
    p.add_argument('--conditioning', default=None, help="With --model: the conditioning it was trained with (none, or fasttext:<lang>)")
    p.add_argument('--word-vectors', dest='word_vectors', default=None, help='With --model and fasttext conditioning: the .vec / .npz word-vector table')
    p.add_argument('--forced', action='store_true', help='With --model: forced alignment (the recordings\' durations and pitch) instead of free running')
    p.add_argument('--batch', type=int, default=32, help='Utterances per padded batch (default=32)')
    p.add_argument('--limit', type=int, default=-1, help='Score only the first N items (default: all)')
    p.add_argument('--device', default='cuda:0', help='HIP device (default=cuda:0)')
    p.add_argument('--output', default=None, help='Write the metrics as JSON here')
    return p


def parse_args(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if a.generated is not None and (a.conditioning or a.word_vectors or a.forced):
        p.error('--conditioning, --word-vectors and --forced go with --model')
    if a.batch < 1:
        p.error('--batch must be at least 1')
    return a


def load_model(prefix, conditioning, device):
    from ttscube_amd.io_utils.io_cubegan import CubeganEncodings
    from ttscube_amd.networks.cubegan import Cubegan
    path = next((prefix + ext for ext in ('.best', '.model', '.last') if os.path.exists(prefix + ext)), None)
    if path is None:
        raise FileNotFoundError('%s.best / .model / .last: no checkpoint' % prefix)
    model = Cubegan(CubeganEncodings(prefix + '.encodings'), conditioning=conditioning, train=False)
    model.load(path)
    return model.to(device).eval()


def main(argv=None, evaluator=None, out=None):
    """evaluator (tests): an Evaluator built elsewhere, e.g. around an injected aligner"""
    a = parse_args(argv)
    out = out if out is not None else sys.stdout
    from ttscube_amd.io_utils import evaluate as E
    conditioning = None if a.conditioning in (None, 'none') else a.conditioning
    if evaluator is None:
        evaluator = E.Evaluator(a.device)
    generated = a.generated if a.generated is not None else load_model(a.model, conditioning, a.device)
    res = evaluator.evaluate_devset(a.devset, generated, batch=a.batch, limit=a.limit, free=not a.forced, conditioning=conditioning,
                                    word_vectors=a.word_vectors, log=lambda line: out.write(line + '\n'))
    if a.output:
        E.write_json(res, a.output)
    return 0


if __name__ == '__main__':
    sys.exit(main())
