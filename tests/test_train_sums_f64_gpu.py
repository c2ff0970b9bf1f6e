"""GPU: the four summation kernels of csrc/train_ops.hip behind every bias gradient and embedding gradient — bias_grad_kernel (through
hifigan/autograd.py::_bias_grad, as the product allocates its workspace), rows_gather_kernel, rows_scatter_add_kernel, rows_segment_sum_kernel —
against the float64 statements of tests/optim_reference.py, two ways each:

  exact data   values k / 64 small enough that no float32 partial sum can round: assert_array_equal against float64 — one lost or doubled element
               of a 10^5-term sum shows, whatever the order
  random data  |err| <= (d + 2) u sum|terms| per output, d = the length of the longest chain of additions the kernel's own order gives that output
               (bias_grad: per-accumulator trips + 2 joins + 6 shuffle levels + 4 waves + S partials, computed from the shape by
               optim_reference.bias_grad_depth; row sums: the run length)

Measured on an MI355X: d and the worst error / bound per case are printed here and recorded in DESIGN.md section 2d."""
import numpy as np
import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

BIAS_SHAPES = [
    # n = B * w of a block at the edges of the four-way loop (i + 768 < n) and its remainder loop; one slice each (L <= 1024)
    (1, 3, 255), (1, 3, 256), (1, 3, 257), (3, 3, 341), (1, 3, 1024), (5, 3, 205), (11, 3, 163),
    # L around the slice length; the product's last generator layer
    (2, 3, 1), (2, 3, 1025), (2, 3, 2049), (16, 32, 12064),
    # C = 1: S at its cap of 1024, the last slice ragged (2 of 1025 positions)
    (1, 1, 1024 * 1024 + 1),
    # S = 1 by the cap, or by L
    (3, 5, 17), (2, 512, 50), (2, 1024, 33), (2, 1024, 2049), (2, 512, 2049),
]


def _bias_case(B, C, L, seed):
    exact = R.exact_values((B, C, L), B * L, seed=seed)
    rnd = (np.random.RandomState(seed + 1).standard_normal((B, C, L)) * 10.0 ** np.random.RandomState(seed + 2).uniform(-2, 2, size=(1, C, 1))).astype(np.float32)
    return exact, rnd


def _bias_check(tc, dy, exact, label):
    from ttscube_amd.hifigan.autograd import _bias_grad
    B, C, L = dy.shape
    got = _bias_grad(tc, torch.from_numpy(dy).cuda()).cpu().numpy().astype(np.float64)
    ref = R.bias_grad(dy)
    if exact:
        np.testing.assert_array_equal(got, ref, err_msg=label)
        return 0.0
    d, S = R.bias_grad_depth(B, C, L)
    bound = (d + 2) * R.U * np.abs(dy.astype(np.float64)).sum(axis=(0, 2))
    ratio = R.worst_ratio(got, ref, bound)
    print('SUM bias_grad %s: S %d  d %d  worst error / bound %.4f' % (label, S, d, ratio))
    assert ratio <= 1.0, label
    return ratio


@pytest.mark.parametrize('shape', BIAS_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_bias_grad_on_exact_and_random_data(shape):
    from ttscube_amd.hifigan.autograd import TrainConv
    B, C, L = shape
    assert R.bias_grad_splits(B, C, L) == {(16, 32, 12064): 12, (1, 1, 1024 * 1024 + 1): 1024, (2, 3, 1025): 2, (2, 3, 2049): 3, (2, 512, 2049): 2}.get(shape, 1)
    tc = TrainConv(4, 4, 1)
    exact, rnd = _bias_case(B, C, L, seed=B + C + L)
    _bias_check(tc, exact, True, 'exact')
    _bias_check(tc, rnd, False, '%dx%dx%d' % shape)


def test_bias_grad_twice_on_one_layer_and_after_another_shape():
    """each call equals ITS OWN float64 sum: a ticket or a partial left by the call before would show (S = 12, then S = 3 and back)"""
    from ttscube_amd.hifigan.autograd import TrainConv
    tc = TrainConv(4, 4, 1)
    a = (4, 32, 12064)
    for rep in range(2):
        _bias_check(tc, R.exact_values(a, 4 * 12064, seed=30 + rep), True, 'call %d' % rep)
    ws = next(iter(tc._bg_ws.values()))
    _bias_check(tc, R.exact_values((2, 3, 2049), 2 * 2049, seed=33), True, 'another shape')
    _bias_check(tc, R.exact_values(a, 4 * 12064, seed=34), True, 'first shape again')
    _bias_check(tc, _bias_case(*a, seed=35)[1], False, 'first shape again, random')
    assert next(iter(tc._bg_ws.values())) is not ws        # (one workspace per layer: a new shape replaces it, and the new one starts at zero)


# ---- embedding rows ---------------------------------------------------------------------------------------------------------------------------------

def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda() if dtype else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _gather(table, idx):
    from ttscube_amd import _lib
    V, C = table.shape
    t, i = _dev(table), _dev(idx, torch.int32)
    out = torch.full((len(idx) + 1, C), -7.0, device='cuda')            # one row more: a write past n * C would show
    _lib.check(_lib.lib().ttsc_rows_gather(_lib.dev_ptr(t), _lib.dev_ptr(i), _lib.dev_ptr(out), len(idx), C, V, _lib.current_stream()), 'ttsc_rows_gather')
    torch.cuda.synchronize()
    assert bool((out[-1] == -7.0).all())
    return out[:-1].cpu().numpy()


@pytest.mark.parametrize('C', [1, 3, 64, 257])
def test_rows_gather_has_the_bits_of_the_table_rows(C):
    V = 11
    r = np.random.RandomState(C)
    table = r.standard_normal((V, C)).astype(np.float32)
    idx = np.concatenate([[0, V - 1, -1, V, 5, V + 1000, -2 ** 31], r.randint(0, V, size=300)])
    for ix in (idx, idx[:1], idx[2:3], idx[1:2]):                        # the list; n = 1 at row 0, outside, at the last row
        got = _gather(table, ix)
        ref = R.rows_gather(table, ix)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float64), ref)
    assert not _gather(table, idx)[[2, 3, 5, 6]].any()


def _scatter(gout, idx, V, skip):
    from ttscube_amd import _lib
    n, C = gout.shape
    g, i = _dev(gout), _dev(idx, torch.int32)
    out = torch.full((V + 1, C), -7.0, device='cuda')
    _lib.check(_lib.lib().ttsc_rows_scatter_add(_lib.dev_ptr(g), _lib.dev_ptr(i), _lib.dev_ptr(out), n, C, V, skip, _lib.current_stream()),
               'ttsc_rows_scatter_add')
    torch.cuda.synchronize()
    assert bool((out[-1] == -7.0).all())
    return out[:-1].cpu().numpy()


def _segment(gout, idx, V):
    from ttscube_amd import _lib
    n, C = gout.shape
    g, i = _dev(gout), _dev(idx, torch.int32)
    out = torch.full((V + 1, C), -7.0, device='cuda')
    _lib.check(_lib.lib().ttsc_rows_segment_sum(_lib.dev_ptr(g), _lib.dev_ptr(i), _lib.dev_ptr(out), n, C, V, _lib.current_stream()), 'ttsc_rows_segment_sum')
    torch.cuda.synchronize()
    assert bool((out[-1] == -7.0).all())
    return out[:-1].cpu().numpy()


V_ROWS = 13


def _sorted_lists():
    """name -> non-decreasing index list over V_ROWS rows"""
    r = np.random.RandomState(8)
    free = np.sort(r.randint(1, V_ROWS - 1, size=200))
    return {
        'one run': np.full(150, 6),
        'all distinct': np.arange(V_ROWS),
        'a run at the first index': np.concatenate([np.zeros(90, dtype=np.int64), free]),
        'a run at the last index': np.concatenate([free, np.full(70, V_ROWS - 1)]),
        'a value missing in the middle': np.sort(np.where(free == 6, 7, free)),
        'one entry': np.array([4]),
        'one entry, last row': np.array([V_ROWS - 1]),
    }


def _rows_data(n, C, seed):
    exact = R.exact_values((n, C), n, seed=seed)
    scale = 10.0 ** np.random.RandomState(seed + 2).uniform(-2, 2, size=(n, 1))
    rnd = (np.random.RandomState(seed + 1).standard_normal((n, C)) * scale).astype(np.float32)
    return exact, rnd


def _rows_check(kernel, got, gout, idx, skip, exact, label):
    ref = R.rows_scatter_add(gout, idx, V_ROWS, skip)
    unnamed = [v for v in range(V_ROWS) if v == skip or not (idx == v).any()]
    assert not got[unnamed].any(), label                                 # rows no index names, and the skipped row: zeros
    if exact:
        np.testing.assert_array_equal(got.astype(np.float64), ref, err_msg=label)
        return
    d = R.rows_depth(idx, V_ROWS)
    bound = (d[:, None] + 2) * R.U * R.rows_abs_sum(gout, idx, V_ROWS, skip)
    ratio = R.worst_ratio(got, ref, bound)
    print('SUM %s %s: d %d  worst error / bound %.4f' % (kernel, label, d.max(), ratio))
    assert ratio <= 1.0, label


@pytest.mark.parametrize('C', [1, 3, 64, 257, 300])
def test_scatter_add_and_segment_sum_on_sorted_lists(C):
    for name, idx in _sorted_lists().items():
        for which, gout in zip(('exact', 'random'), _rows_data(len(idx), C, seed=C + len(idx))):
            seg = _segment(gout, idx, V_ROWS)
            _rows_check('segment_sum', seg, gout, idx, -1, which == 'exact', '%s C=%d %s' % (name, C, which))
            for skip in (-1, 0, 6):
                sc = _scatter(gout, idx, V_ROWS, skip)
                _rows_check('scatter_add', sc, gout, idx, skip, which == 'exact', '%s C=%d skip=%d %s' % (name, C, skip, which))
                keep = np.arange(V_ROWS) != skip
                assert np.array_equal(sc[keep], seg[keep]), (name, skip)       # the two kernels, bit for bit


@pytest.mark.parametrize('C', [1, 3, 64, 257, 300])
def test_scatter_add_on_unsorted_lists(C):
    r = np.random.RandomState(C + 1)
    idx = r.randint(0, V_ROWS, size=333)
    idx[idx == 9] = 2                                                      # row 9: named by nobody
    lists = {'unsorted': idx, 'unsorted with entries outside the table': np.concatenate([idx[:50], [-1, V_ROWS, V_ROWS + 7], idx[50:]]),
             'one entry': idx[:1]}
    for name, ix in lists.items():
        for which, gout in zip(('exact', 'random'), _rows_data(len(ix), C, seed=C + 5)):
            for skip in (-1, 0, 6):
                _rows_check('scatter_add', _scatter(gout, ix, V_ROWS, skip), gout, ix, skip, which == 'exact', '%s C=%d skip=%d %s' % (name, C, skip, which))
