"""CPU: the StoryCube restatements agree with each other (tests/story_reference.py), plan_timeline gives the reference's bookkeeping, and the command
line parses without loading any GPU code."""
import os
import subprocess
import sys

import numpy as np

from tests import story_reference as SR
from tests.conftest import ROOT


def _seeded_case():
    """3 segments, 36 300 timeline samples, music of 977 samples; |speech| <= 22 600 and |music| <= 1, so |sum| <= 32 410: no saturation"""
    rng = np.random.default_rng(20240607)
    lengths = [5003, 1, 12007]
    segments = [rng.integers(-22600, 22601, size=n).astype(np.int16) for n in lengths]
    seg_dst = [4801, 9804, 14000]          # the second starts where the first ends
    total = 36300
    music = rng.uniform(-1.0, 1.0, size=977).astype(np.float32)
    music[:2] = (1.0, -1.0)
    return segments, seg_dst, music, total


def test_vectorised_restatement_equals_the_literal_loop_bit_for_bit():
    segments, seg_dst, music, total = _seeded_case()
    assert total <= 40000 and seg_dst[0] + len(segments[0]) == seg_dst[1]
    literal = SR.mix_literal(segments, seg_dst, music, total)
    vec, clipped = SR.mix_vectorised(segments, seg_dst, music, total)
    assert clipped == 0
    assert literal.dtype == vec.dtype == np.int16 and literal.shape == vec.shape == (total,)
    assert np.array_equal(literal, vec)
    # a range of the timeline is that slice of the whole
    part, c = SR.mix_vectorised(segments, seg_dst, music, total, t0=4790, n=5100)
    assert c == 0 and np.array_equal(part, vec[4790:4790 + 5100])


def test_plan_timeline_is_the_reference_bookkeeping():
    from ttscube_amd.io_utils.story_mix import plan_timeline
    for lengths in ([0], [1], [31337, 0, 120001]):
        texts = ['part %d' % k for k in range(len(lengths))]
        offsets, total, meta = SR.timeline_literal(lengths, texts)
        got = plan_timeline(lengths, texts=texts)
        assert got == (offsets, total, meta), lengths
        assert got[2][0] == {'name': 'intro', 'start': 0, 'end:': 5, 'text': ''}
        assert list(got[2][1]) == ['name', 'text', 'start', 'end']          # the reference's key order too (json.dump keeps it)
        assert all(type(m['end']) is float for m in got[2][1:])
        assert total == 240000 + sum(lengths) + 24000 * len(lengths)
        # without texts: the same skeleton with empty texts
        assert plan_timeline(lengths) == SR.timeline_literal(lengths)
    # the accumulated float `start` is the reference's running sum, not a product
    _, _, meta = plan_timeline([31337, 0, 120001])
    assert meta[3]['start'] == 5 + (31337 / 24000 + 1) + (0 / 24000 + 1)
    assert meta[3]['end'] == meta[3]['start'] + (120001 / 24000) + 1


def test_story_mix_module_needs_no_extension_for_planning():
    code = ('import sys; sys.path.insert(0, %r); from ttscube_amd.io_utils.story_mix import plan_timeline; plan_timeline([3]); '
            'bad = [m for m in ("torch", "ttscube_amd._lib") if m in sys.modules]; assert not bad, bad' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_story_script_help_imports_no_gpu_code():
    script = os.path.join(ROOT, 'scripts', 'story.py')
    code = ('import runpy, sys\n'
            'sys.argv = [%r, "--help"]\n'
            'try:\n'
            '    runpy.run_path(%r, run_name="__main__")\n'
            'except SystemExit as e:\n'
            '    assert e.code in (0, None), e.code\n'
            'else:\n'
            '    raise AssertionError("--help did not exit")\n'
            'bad = [m for m in ("torch", "ttscube_amd._lib", "ttscube_amd.story", "ttscube_amd.api") if m in sys.modules]\n'
            'assert not bad, bad\n' % (script, script))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ('--model', '--model-path', '--phonemizer-path', '--text-file', '--speaker', '--music', '--output', '--meta'):
        assert flag in r.stdout, flag
