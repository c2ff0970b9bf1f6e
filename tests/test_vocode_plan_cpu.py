"""CPU tests of the batched-vocoding planner (networks/vocode_plan.py) against the numpy restatement of the reference's fold / un-fold
(oracle/wavernn_ref.py::inference_batch, compose_batched_inference), and of scripts/vocode.py's argument parsing.  No HIP library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import wavernn_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_LISTS = [[1], [19], [20], [21], [1, 19, 20, 21], [40, 7, 23, 61, 20], [2, 2, 2], [399, 5, 77],
           [int(t) for t in np.random.RandomState(3).randint(1, 330, size=64)]]


def _plan(Ts, max_rows, seed=1000, num_batches=20):
    from ttscube_amd.networks.vocode_plan import plan_vocode
    return plan_vocode(Ts, [seed + i for i in range(len(Ts))], num_batches=num_batches, max_rows=max_rows)


@pytest.mark.parametrize('max_rows', [8, 24, 256])
@pytest.mark.parametrize('case', range(len(T_LISTS)))
def test_plan_folds_and_unfolds_like_the_reference(case, max_rows):
    Ts = T_LISTS[case]
    rng = np.random.RandomState(case)
    mels = [rng.randn(T, 80).astype(np.float32) for T in Ts]
    x_lrs = [rng.uniform(-1, 1, size=24 * T).astype(np.float32) for T in Ts]
    plan = _plan(Ts, max_rows)
    # every (utterance, chunk) exactly once; seeds and streams per row
    want = sorted((i, c) for i, T in enumerate(Ts) for c in range(min(T, 20)))
    assert sorted((r.utt, r.chunk) for r in plan.rows) == want
    assert sorted(k for l in plan.launches for k in l) == list(range(len(plan.rows)))
    for r in plan.rows:
        assert r.seed == 1000 + r.utt and r.stream == r.chunk
    # launches: at most max_rows rows, longest first (across the launches too)
    lens = [plan.rows[k].out_len for l in plan.launches for k in l]
    assert all(len(l) <= max_rows for l in plan.launches) and lens == sorted(lens, reverse=True)
    assert all(len(l) <= max_rows for l in plan.lr_launches)
    assert sorted(i for l in plan.lr_launches for i in l) == list(range(len(Ts)))
    # fold: the rows' valid prefixes equal the reference's folded arrays
    mel_src = np.concatenate([np.full((1, 80), -5.0, dtype=np.float32)] + mels)
    low_src = np.concatenate([np.zeros(1, dtype=np.float32)] + x_lrs)
    folded = [O.inference_batch(m[None], x[None], num_batches=20) for m, x in zip(mels, x_lrs)]
    rng2 = np.random.RandomState(99)
    fake, launch_out = {}, []
    for li, launch in enumerate(plan.launches):
        im, il = plan.fold_index(li)
        fr, ll, sd, st = plan.hr_tables(li)
        m, xl = mel_src[im], low_src[il]
        W = plan.launch_width(li)
        out = np.zeros((len(launch), W), dtype=np.float32)
        for k, ri in enumerate(launch):
            r = plan.rows[ri]
            f = folded[r.utt]
            assert (fr[k], ll[k]) == (f['mel'].shape[1], f['x_low'].shape[1]) == (r.frames, r.low_len)
            assert (sd[k], st[k]) == (r.seed, r.stream)
            assert np.array_equal(m[k, :fr[k]], f['mel'][r.chunk]) and np.array_equal(xl[k, :ll[k]], f['x_low'][r.chunk])
            assert r.out_len == min(240 * r.frames, 10 * r.low_len) <= W
            fake[(r.utt, r.chunk)] = rng2.randn(r.out_len).astype(np.float32)   # what the hr net would emit for this row
            out[k, :r.out_len] = fake[(r.utt, r.chunk)]
        launch_out.append(out.reshape(-1))
    # un-fold: the inverse plan reassembles compose_batched_inference's output
    flat = np.concatenate(launch_out)
    for i, ix in enumerate(plan.unfold_index()):
        batched = np.stack([fake[(i, c)] for c in range(plan.utts[i].nb)])
        assert np.array_equal(flat[ix][None], O.compose_batched_inference(batched))
    # low-resolution rows
    for li, launch in enumerate(plan.lr_launches):
        lengths, sd, st = plan.lr_tables(li)
        m = mel_src[plan.lr_mel_index(li)]
        for r, i in enumerate(launch):
            assert lengths[r] == Ts[i] and sd[r] == 1000 + i and st[r] == 0 and np.array_equal(m[r, :Ts[i]], mels[i])
    batch_steps, loop_steps = plan.steps()
    assert loop_steps == sum(24 * T + plan.utts[i].keep + 240 for i, T in enumerate(Ts))
    assert batch_steps == (sum(24 * max(Ts[i] for i in l) for l in plan.lr_launches) +
                           sum(max(plan.rows[k].out_len for k in l) for l in plan.launches))
    if len(plan.launches) == 1 and len(plan.lr_launches) == 1:   # everything in one launch per net: never more steps than the loop
        assert batch_steps <= loop_steps


def test_plan_rejects_bad_input():
    from ttscube_amd.networks.vocode_plan import plan_vocode
    for args in (([], []), ([3, 0], [1, 2]), ([3], [1, 2])):
        with pytest.raises(ValueError):
            plan_vocode(*args)
    with pytest.raises(ValueError):
        plan_vocode([3], [1], max_rows=0)


def test_vocode_script_help_needs_no_hip_library(tmp_path):
    """--help parses and prints without the HIP library (or torch) being loaded"""
    probe = ("import runpy, sys\n"
             "sys.argv = [%r, '--help']\n"
             "try:\n"
             "    runpy.run_path(sys.argv[0], run_name='__main__')\n"
             "except SystemExit as e:\n"
             "    assert e.code in (0, None), e.code\n"
             "assert 'ttscube_amd._lib' not in sys.modules and 'torch' not in sys.modules\n") % os.path.join(ROOT, 'scripts', 'vocode.py')
    r = subprocess.run([sys.executable, '-c', probe], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    for flag in ('--model', '--input', '--output-folder', '--batch', '--seed', '--argmax', '--device'):
        assert flag in r.stdout
