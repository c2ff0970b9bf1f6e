#!/usr/bin/env python
"""Bring a folder of wav files to one integrated loudness (ITU-R BS.1770-4 / EBU R 128) under a true-peak ceiling, on the GPU
(ttscube_amd/io_utils/loudness.py): one static gain per file.  Files of any rate are read, grouped by rate, and every group of up to --batch files
is measured and scaled in one padded batch; the results are written as int16 wav files at the file's own rate, with a report.json beside them.
Silent files (no block above the gates) are listed and copied unscaled.

    python scripts/normalize_loudness.py --input-folder wavs --output-folder wavs_r128 --target -23 --peak -1"""
import json
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None, meter=None):
    """meter: an object with LoudnessMeter's `normalize(rows, sr, target, peak_db)` (default: LoudnessMeter(--device))"""
    p = ArgumentParser(description='Loudness-normalise a folder of wav files (BS.1770-4 integrated loudness, true-peak ceiling)')
    p.add_argument('--input-folder', dest='input_folder', required=True)
    p.add_argument('--output-folder', dest='output_folder', required=True)
    p.add_argument('--target', type=float, default=-23.0, help='integrated loudness in LUFS')
    p.add_argument('--peak', type=float, default=-1.0, help='true-peak ceiling in dB')
    p.add_argument('--batch', type=int, default=32, help='files per padded batch')
    p.add_argument('--device', default='cuda:0')
    params = p.parse_args(argv)
    if params.batch < 1:
        p.error('--batch must be at least 1')

    from ttscube_amd.io_utils.audio import read_wav, save_wav
    from ttscube_amd.io_utils.loudness import check_rate
    names = sorted(f for f in os.listdir(params.input_folder) if f.lower().endswith('.wav'))
    if not names:
        p.error('no .wav files in %s' % params.input_folder)
    by_rate = {}
    for name in names:
        x, rate = read_wav(os.path.join(params.input_folder, name))
        by_rate.setdefault(int(rate), []).append((name, x))
    for rate in by_rate:
        check_rate(rate)                                        # a rate the meter refuses stops the run before anything is written
    if meter is None:
        from ttscube_amd.io_utils.loudness import LoudnessMeter
        meter = LoudnessMeter(params.device)
    os.makedirs(params.output_folder, exist_ok=True)
    report = {'target': params.target, 'peak': params.peak, 'files': {}, 'silent': []}
    for rate in sorted(by_rate):
        items = sorted(by_rate[rate], key=lambda it: it[1].size)      # (neighbours in length share a padded batch)
        for s in range(0, len(items), params.batch):
            group = items[s:s + params.batch]
            rows, reps = meter.normalize([x for _, x in group], rate, target=params.target, peak_db=params.peak)
            for (name, _), y, rep in zip(group, rows, reps):
                save_wav(os.path.join(params.output_folder, name), y, rate)
                report['files'][name] = dict(rep, sample_rate=rate, lufs_in=_num(rep['lufs_in']), lufs_out=_num(rep['lufs_out']))
                if rep['silent']:
                    report['silent'].append(name)
    report['silent'].sort()
    with open(os.path.join(params.output_folder, 'report.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print('%d files -> %s at %.1f LUFS (ceiling %.1f dB)%s' % (len(names), params.output_folder, params.target, params.peak,
                                                          '; silent, left unscaled: ' + ', '.join(report['silent']) if report['silent'] else ''))
    return report


def _num(v):
    """JSON has no -inf: a silent file's loudness is null"""
    return None if v == float('-inf') else v


if __name__ == '__main__':
    main()
