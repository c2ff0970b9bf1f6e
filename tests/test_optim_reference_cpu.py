"""The reference of tests/test_adamw_f64_gpu.py and tests/test_train_sums_f64_gpu.py, checked without a GPU (tests/optim_reference.py): the float64
AdamW statement is torch.optim.AdamW in float64, both float32 restatements stay inside the counted per-element bound from every state they pass
through, the exact-data generator gives sums that no float32 order can round, and the statements of the sums are the torch formulations they
stand for."""
import numpy as np
import pytest
import torch

from tests import optim_reference as R

SETTINGS = [R.PRODUCT, (1e-3, (0.9, 0.999), 1e-8, 0.0), (3e-2, (0.5, 0.9), 1e-6, 0.1), (1e-4, (0.7, 0.95), 1e-8, 1e-2)]


@pytest.mark.parametrize('hyper', SETTINGS)
def test_adamw_step_is_torch_adamw_in_float64(hyper):
    """50 steps of torch.optim.AdamW(foreach=False) on float64 CPU tensors, the learning rate changed between steps, against adamw_step fed with
    the same gradients: parameters and both moments to 1e-14 relative"""
    lr, betas, eps, wd = hyper
    r = np.random.RandomState(1)
    n = 301
    p0 = r.randn(n)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 51):
        cur = R.lr_at(lr, step - 1) if step % 2 else lr * 0.37
        g = r.randn(n) * 10.0 ** r.uniform(-3, 1)
        opt.param_groups[0]['lr'] = cur
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adamw_step(p, g, m, v, step, cur, betas, eps, wd)
        st = opt.state[q]
        for got, ref in ((p, q.detach().numpy()), (m, st['exp_avg'].numpy()), (v, st['exp_avg_sq'].numpy())):
            assert np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref)), step
        assert float(st['step']) == step


def _ratios(c, steps=6):
    """walk `steps` steps from a family's state with both restatements (each from ITS OWN float32 state: the bound is about one step from a given
    float32 state) and return the worst error / bound of p, m, v over all of them"""
    worst = {}
    for kind in (False, True):
        p, g, m, v = c['p'], c['g'], c['m'], c['v']
        for k in range(steps):
            step = c['step'] + k
            hyper = c['hyper']
            ref = R.adamw_step(p, g, m, v, step, *R.f32_hyper(*hyper))
            bound = R.adamw_step_bound(p, g, m, v, *ref, R.true_scalars(step, *R.f32_hyper(*hyper)))
            got = R.adamw_step_f32(p, g, m, v, R.host_scalars(step, *hyper), fused=kind)
            for name, a, b, c_ in zip('pmv', got, ref, bound):
                assert np.all(np.isfinite(a)), (name, step)
                key = ('fused' if kind else 'plain', name)
                worst[key] = max(worst.get(key, 0.0), R.worst_ratio(a, b, c_))
            p, m, v = got
    return worst


def test_float32_restatements_stay_inside_the_step_bound(capsys):
    """Both restatements, six consecutive steps from each family of section 2 of the GPU test and from the generic state of its section 1 at step
    counts 1, 2, 1000 and 1 000 000: every element of p, m and v inside adamw_step_bound.  The worst error / bound is printed per family.

    Where the figures sit (this file prints them; 4099 elements, six steps, plain and fused alike): m 0.10 .. 0.25, v 0.25 .. 0.58 (both exactly
    0 in zero_grad, where nothing rounds; tiny_grad's v 0.66, of the 1.5 subnormal spacings that are its whole bound), p 0.25 .. 0.36 where only
    the decay acts and 0.58 .. 0.60 wherever the update does.  So m and v sit between or at the two marks (0.01: too loose to catch anything, 0.5: too
    tight to be honest about the kernel), and p sits just ABOVE the upper one: the count for p is a worst case with little to spare — ten
    roundings on the update, of which some element among 25 000 gets six tenths — not a loose one.  It stays as counted: every operation in it is
    one the kernel performs, and a kernel that performs them correctly rounded cannot leave it.  (A division or root that were only faithful,
    one ulp instead of a half, would add 2 of the 10 and still fit.)"""
    rows = []
    cases = dict(R.adamw_families(4099, seed=5))
    for step in (1, 2, 1000, 1000000):
        p, g, m, v = R.random_state(4099, seed=step % 97)
        cases['generic@%d' % step] = dict(p=p, g=g, m=m, v=v, step=step, hyper=R.PRODUCT)
    for name, c in cases.items():
        w = _ratios(c)
        rows.append((name, w))
        for key, val in w.items():
            assert val <= 1.0, (name, key, val)
    with capsys.disabled():
        print('\nAdamW float32 restatements, worst error / bound over six steps (plain | fused):')
        for name, w in rows:
            print('  %-18s p %.3f | %.3f   m %.3f | %.3f   v %.3f | %.3f' % (name, w[('plain', 'p')], w[('fused', 'p')], w[('plain', 'm')],
                                                                            w[('fused', 'm')], w[('plain', 'v')], w[('fused', 'v')]))
    # not loose where something rounds: every family but zero_grad (m, v exact) moves each of p, m, v by more than a hundredth of its bound
    for name, w in rows:
        for key, val in w.items():
            assert val > 0.01 or (name == 'zero_grad' and key[1] in 'mv'), (name, key, val)


def test_bound_rejects_a_bias_correction_one_step_off_and_a_missing_tail_update():
    """what the GPU test relies on: inv_bc2s taken at step - 1 leaves the bound by orders of magnitude at small step counts, and an element that was
    not updated at all does too"""
    p, g, m, v = R.random_state(1024, seed=3)
    hyper = R.PRODUCT
    for step in (2, 41):
        ref = R.adamw_step(p, g, m, v, step, *R.f32_hyper(*hyper))
        bound = R.adamw_step_bound(p, g, m, v, *ref, R.true_scalars(step, *R.f32_hyper(*hyper)))
        s = R.host_scalars(step, *hyper)
        s['inv_bc2s'] = R.host_scalars(step - 1, *hyper)['inv_bc2s']
        assert R.worst_ratio(R.adamw_step_f32(p, g, m, v, s)[0], ref[0], bound[0]) > 100
        assert R.worst_ratio(p, ref[0], bound[0]) > 100 and R.worst_ratio(m, ref[1], bound[1]) > 100
    # a resume that restarted the bias correction at 1 instead of 41
    ref = R.adamw_step(p, g, m, v, 41, *R.f32_hyper(*hyper))
    bound = R.adamw_step_bound(p, g, m, v, *ref, R.true_scalars(41, *R.f32_hyper(*hyper)))
    assert R.worst_ratio(R.adamw_step_f32(p, g, m, v, R.host_scalars(1, *hyper))[0], ref[0], bound[0]) > 1000


@pytest.mark.parametrize('shape,terms', [((16, 5, 12064), 16 * 12064), ((1, 1, 1024 * 1024 + 1), 1024 * 1024 + 1), ((300, 257), 300), ((3, 2, 7), 21)])
def test_exact_values_sum_the_same_in_three_orders_and_in_float64(shape, terms):
    x = R.exact_values(shape, terms, seed=4)
    assert x.dtype == np.float32 and np.abs(x).max() > 0
    flat = (x.transpose(1, 0, 2).reshape(shape[1], -1) if len(shape) == 3 else x.T.copy())       # one row per output, `terms` values each
    assert flat.shape[1] == terms
    ref = flat.astype(np.float64).sum(axis=1)
    f = np.float32
    forward = np.cumsum(flat, axis=1, dtype=f)[:, -1]                      # one at a time (a float32 running sum)
    backward = np.cumsum(flat[:, ::-1], axis=1, dtype=f)[:, -1]
    pad = (-terms) % 256
    strided = np.concatenate([flat, np.zeros((flat.shape[0], pad), dtype=f)], axis=1).reshape(flat.shape[0], -1, 256)
    lanes = np.cumsum(strided, axis=1, dtype=f)[:, -1, :]                  # 256 strided chains, then a pairwise tree: the kernels' own shape
    while lanes.shape[1] > 1:
        lanes = lanes[:, :lanes.shape[1] // 2] + lanes[:, lanes.shape[1] // 2:]
    for s in (forward, backward, lanes[:, 0]):
        assert s.dtype == f
        np.testing.assert_array_equal(s.astype(np.float64), ref)
    with pytest.raises(AssertionError):
        R.exact_values((4,), 2 ** 24)


def test_statements_of_the_sums_are_the_torch_formulations():
    r = np.random.RandomState(2)
    dy = r.randn(3, 5, 17)
    np.testing.assert_allclose(R.bias_grad(dy), torch.from_numpy(dy).sum((0, 2)).numpy(), rtol=1e-14, atol=1e-14)
    V, Cc, n = 9, 6, 40
    table, gout = r.randn(V, Cc), r.randn(n, Cc)
    idx = r.randint(0, V, size=n)
    idx[idx == 4] = 5                                                     # row 4: named by nobody
    np.testing.assert_array_equal(R.rows_gather(table, idx), torch.from_numpy(table).index_select(0, torch.from_numpy(idx)).numpy())
    wild = idx.copy()
    wild[[0, 7]] = (-1, V)
    got = R.rows_gather(table, wild)
    assert not got[0].any() and not got[7].any() and np.array_equal(got[1:7], table[idx[1:7]])
    for skip in (-1, 0, 5):
        ref = torch.zeros(V, Cc, dtype=torch.float64).index_add_(0, torch.from_numpy(idx), torch.from_numpy(gout)).numpy()
        if skip >= 0:
            ref[skip] = 0
        got = R.rows_scatter_add(gout, idx, V, skip)
        np.testing.assert_allclose(got, ref, rtol=1e-14, atol=1e-14)
        assert not got[4].any()
    srt = np.sort(idx)
    ref = torch.zeros(V, Cc, dtype=torch.float64).index_add_(0, torch.from_numpy(srt), torch.from_numpy(gout)).numpy()
    np.testing.assert_allclose(R.rows_segment_sum(gout, srt, V), ref, rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(R.rows_depth(srt, V), np.bincount(srt, minlength=V))


def test_bias_grad_depth_follows_the_kernels_loops():
    """S and the chain length at the edges the GPU test visits (hand-counted from bias_grad_kernel)"""
    assert R.bias_grad_splits(1, 1, 1024 * 1024 + 1) == 1024 and R.bias_grad_splits(16, 32, 12064) == 12
    assert R.bias_grad_splits(2, 512, 5000) == 2 and R.bias_grad_splits(2, 1024, 5000) == 1 and R.bias_grad_splits(2, 3, 1) == 1
    for n, trips in ((255, 1), (256, 1), (257, 2), (1023, 3), (1024, 1), (1025, 0), (1793, 0)):
        # B = 1, L = n <= 1024: one slice.  n = 1024: every thread takes one four-way trip and nothing else (a0 once); n = 1023: thread 255 fails i + 768 < n and walks 255, 511, 767 in the remainder loop
        d, S = R.bias_grad_depth(1, 3, n)
        assert S == (2 if n > 1024 else 1) and (S == 2 or d == trips + 12 + 1), (n, d)
    d, S = R.bias_grad_depth(11, 3, 163)           # n = 1793, S = 1
    assert (d, S) == (4 + 2 + 6 + 4 + 1, 1)
    d, S = R.bias_grad_depth(1, 3, 257)
    assert (d, S) == (2 + 12 + 1, 1)
    d, S = R.bias_grad_depth(5, 3, 205)            # n = 1025
    assert (d, S) == (2 + 12 + 1, 1)
