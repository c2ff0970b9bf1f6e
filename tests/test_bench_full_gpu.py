"""GPU: what a plain `bench.py` run does and what only `--full` adds.  A plain run sets up, warms up, times the steps and prints the headline line:
no oracle check, no sustained-MFMA probe, no secondary legs, no CPU baseline, and at most 30 s of its whole run (process start to exit) outside the
warm-up and timed steps (checked on the headline workload, 64 x 8 s).  `--full` runs the oracle check and the probe after the same timed steps (on a
small batch; legs, live counter passes and the CPU baseline are left out here: they take minutes).  Each run in a process of its own."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ['--gpus', '1', '--steps', '2', '--warmup', '1']
SMALL = ['--batch', '2', '--frames', '40']


def _bench(extra_args):
    """(result line, wall seconds of the whole process)"""
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + STEPS + extra_args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), wall


def _headline(res):
    assert res['metric'] == 'audio samples/sec (HiFi-GAN vocoder inference)' and res['unit'] == 'samples/s' and res['higher_is_better'] is True
    assert res['steps'] == 2 and res['warmup'] == 1 and res['value'] > 0 and res['ms_per_step'] > 0
    samples = res['config']['global_batch'] * res['config']['samples_per_utt']
    assert abs(res['value'] - samples / (res['ms_per_step'] * 1e-3)) <= 1e-6 * res['value']
    assert res['dtype'].startswith('f32')


@pytest.mark.gpu
def test_plain_run_stops_after_the_timed_steps():
    res, wall = _bench([])
    _headline(res)
    outside = wall - (res['steps'] + res['warmup']) * res['ms_per_step'] * 1e-3
    assert outside < 30.0, 'a plain run spent %.1f s outside its steps' % outside
    assert 'extra' not in res and res['cpu_baseline'] is None and res['self_check_rms_vs_oracle'] is None
    assert 'sustained_f16_mfma_tflops' not in res['roofline'] and 'traffic_detail' not in res['roofline']


@pytest.mark.gpu
def test_full_run_adds_the_oracle_check_and_the_probe():
    res, _ = _bench(SMALL + ['--full', '--no-extra', '--no-cpu-baseline'])
    _headline(res)
    assert res['self_check_rms_vs_oracle'] is not None and res['self_check_rms_vs_oracle'] < 1e-4
    if res['config']['precision'] == 'f16x3':
        sus = res['roofline']['sustained_f16_mfma_tflops']
        assert 'error' not in sus and sus['split_mix'] > 0, sus
    assert 'extra' not in res and res['cpu_baseline'] is None
