"""CPU: the host build of include/ttscube_math.h (oracle/wavernn_ref.c, gcc) against float64 over the input sets of tests/math_sweep.py.

The functions are deterministic and the sets are fixed, so the measured maxima are constants: TABLE holds them rounded UP to two significant
digits, the same figures stand in the header's comment and in DESIGN.md ("Shared math: measured accuracy"), and the tests assert them with no
margin.  The device is held to the host bit for bit in tests/test_shared_math_gpu.py, so these figures are the kernels' as well.  Every test
prints what it measured (pytest -s)."""
import os
import re

import numpy as np
import pytest
from scipy.special import ndtri

from oracle import wavernn_ref as O
from tests import math_sweep as M
from tests.conftest import ROOT

F32 = np.float32

# function: (max error in ulps of the result, max relative error, max absolute error) over the function's domain (_measure below)
TABLE = {
    'expf': (0.9, 7.5e-08, 2.6e+30),
    'logf': (2.7, 2e-07, 3.9e-06),
    'sigmoidf': (2.1, 1.4e-07, 8.9e-08),
    'tanhf': (27.0, 1.7e-06, 1.1e-07),
    'normal_icdf': (2300.0, 0.00014, 0.00027),
    'gumbel': (15000000.0, 1.0, 5.4e-07),
    'gumbel_clip': (15000000.0, 1.0, 5.7e-07),
    'logistic': (1100.0, 0.00012, 9.4e-07),
}
# what the project claimed before this table existed, asserted as stated
CLAIM_EXPF_REL = 1.2e-7            # include/ttscube_math.h
CLAIM_LOGF_REL = 2e-7              # include/ttscube_math.h
ACT_ABS = 2.0 ** -23               # tests/test_rnn_train_gpu.py (sigmoid, tanh)
CLAIM_ICDF_ABS = 5e-4              # tests/test_oracle_wavernn.py


def _ulp(want):
    """spacing of float32 at |want| (float64 array); 2^-149 in the subnormal range"""
    _, e = np.frexp(np.maximum(np.abs(want), 2.0 ** -126))
    return np.ldexp(1.0, e - 1 - 23)


def _errors(got, want, arg):
    """(max ulp, max rel, max abs) of float32 `got` against float64 `want`, and the argument of each maximum"""
    got = got.astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    d = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(d == 0, 0.0, d / np.abs(want))
    ulp = d / _ulp(want)
    out, where = [], []
    for e in (ulp, rel, d):
        i = int(np.argmax(e))
        out.append(float(e[i]))
        where.append(arg[i])
    return tuple(out), tuple(where)


@pytest.fixture(scope='module')
def xs():
    return M.float_inputs()


@pytest.fixture(scope='module')
def rs():
    return M.u32_inputs()


def _measure(name, xs, rs):
    """got, want, argument over the documented domain of `name`"""
    if name in ('expf', 'sigmoidf'):
        x = xs[np.isfinite(xs) & (np.abs(xs) <= 87)]
        x64 = x.astype(np.float64)
        want = np.exp(x64) if name == 'expf' else 1.0 / (1.0 + np.exp(-x64))
        return O.math_array(O.FN_EXPF if name == 'expf' else O.FN_SIGMOIDF, x), want, x
    if name == 'tanhf':
        x = xs[np.isfinite(xs)]
        return O.math_array(O.FN_TANHF, x), np.tanh(x.astype(np.float64)), x
    if name == 'logf':
        x = xs[np.isfinite(xs) & (xs >= M.FLT_MIN)]
        return O.math_array(O.FN_LOGF, x), np.log(x.astype(np.float64)), x
    if name == 'normal_icdf':
        p = O.math_array(O.FN_U01, rs)
        return O.math_array(O.FN_NORMAL_ICDF, p), ndtri(p.astype(np.float64)), p
    if name == 'gumbel':
        return O.math_array(O.FN_GUMBEL, rs), -np.log(-np.log(M.u01_exact(rs))), rs
    if name == 'gumbel_clip':   # the Gumbel terms of ttsc_noise_mol: the same two logs on the clipped uniform
        u = O.math_array(O.FN_U01_CLIP, rs)
        return -O.math_array(O.FN_LOGF, -O.math_array(O.FN_LOGF, u)), -np.log(-np.log(u.astype(np.float64))), u
    assert name == 'logistic'
    u = np.unique(np.concatenate([O.math_array(O.FN_U01, rs), O.math_array(O.FN_U01_CLIP, rs)]))
    u64 = u.astype(np.float64)
    return O.math_array(O.FN_LOGISTIC, u), np.log(u64) - np.log1p(-u64), u


_MEASURED = {}


def _measured(name, xs, rs):
    if name not in _MEASURED:
        got, want, arg = _measure(name, xs, rs)
        _MEASURED[name] = _errors(got, want, arg) + (got.size,)
        (u, r, a), (wu, wr, wa), n = _MEASURED[name]
        print('\nttsc_%-12s n=%8d  max ulp %.4g at %r | max rel %.4g at %r | max abs %.4g at %r' % (name, n, u, wu, r, wr, a, wa))
    return _MEASURED[name]


def test_input_sets(xs, rs):
    assert M.stratified_u32().size == -(-(1 << 32) // M.STRIDE) == 4206629
    b = M.bits(xs)
    assert len(np.unique(b >> 23)) == 512                      # every exponent, both signs
    assert np.isnan(xs).any() and np.isinf(xs).any() and (b == 0x80000000).any() and (b == 0).any()
    for p in M.boundary_points():                              # the point, and 64 patterns on either side
        nb = M.neighbours(p)
        assert np.isin(nb, b).all() and nb.size >= 2 * M.RADIUS + 1
    for q in (0, 1, 1 << 22, (1 << 23) - 1):
        assert np.isin(np.array([q << 9, (q << 9) + 511], dtype=np.uint32), rs).all()
    assert rs[0] == 0 and rs[-1] == 0xffffffff


@pytest.mark.parametrize('name', sorted(TABLE))
def test_measured_accuracy_is_the_documented_one(name, xs, rs):
    """the three maxima of every function are at most the figures of the table — and the table is the measured maximum rounded up to two
    digits, so a figure that improves by more than that rounding is flagged as well (the table would be stale)"""
    (u, r, a), _, _ = _measured(name, xs, rs)
    tu, tr, ta = TABLE[name]
    assert u <= tu and r <= tr and a <= ta, (name, (u, r, a), TABLE[name])
    assert u > 0.9 * tu and r > 0.9 * tr and a > 0.9 * ta, 'the table overstates the error of %s: measured %r, written %r' % (name, (u, r, a), TABLE[name])


def test_existing_claims_hold(xs, rs):
    assert _measured('expf', xs, rs)[0][1] <= CLAIM_EXPF_REL
    assert _measured('logf', xs, rs)[0][1] <= CLAIM_LOGF_REL
    assert _measured('tanhf', xs, rs)[0][2] <= ACT_ABS
    assert _measured('sigmoidf', xs, rs)[0][2] <= ACT_ABS
    assert _measured('normal_icdf', xs, rs)[0][2] <= CLAIM_ICDF_ABS


def test_uniforms_are_exact(rs):
    u = O.math_array(O.FN_U01, rs)
    assert np.array_equal(u.astype(np.float64), M.u01_exact(rs))              # 23 bits + one half: no rounding at all
    assert u.min() == M.U01_MIN and u.max() == M.U01_MAX
    c = O.math_array(O.FN_U01_CLIP, rs)
    want = u.astype(np.float64) * np.float64(F32(1.0) - F32(2e-5)) + np.float64(F32(1e-5))
    assert np.abs(c.astype(np.float64) - want).max() <= 2.0 ** -25 * (1 + 1e-6)   # one fmaf: half an ulp of [0.5, 1)
    assert c.min() >= M.CLIP_LO and c.max() <= F32(1.0) - M.CLIP_LO
    print('\nttsc_u01_clip range [%r, %r]' % (c.min(), c.max()))


def _one(fn, x):
    return O.math_array(fn, np.array([x], dtype=np.uint32 if fn >= O.FN_U01 else np.float32))[0]


def test_out_of_domain_behaviour_is_pinned():
    """outside the documented domains the contract is only that host and device agree; these are the values as they are"""
    inf, nan = F32(np.inf), F32(np.nan)
    # both clamps of expf
    for x in (-200.0, -87.000008, -inf):
        assert M.bits(_one(O.FN_EXPF, x)) == M.bits(_one(O.FN_EXPF, -87.0))
    for x in (1000.0, 88.00001, inf):
        assert M.bits(_one(O.FN_EXPF, x)) == M.bits(_one(O.FN_EXPF, 88.0))
    assert _one(O.FN_EXPF, -87.0) == F32(1.6458115e-38) and _one(O.FN_EXPF, 88.0) == F32(1.6516363e+38)
    # sigmoid never reaches 0: below -87.34 it is subnormal, and it stops at 1 / (1 + expf(88))
    assert 0 < _one(O.FN_SIGMOIDF, -87.5) < M.FLT_MIN
    assert M.bits(_one(O.FN_SIGMOIDF, -inf)) == M.bits(_one(O.FN_SIGMOIDF, -88.0)) and 0 < _one(O.FN_SIGMOIDF, -inf) < M.FLT_MIN
    assert _one(O.FN_SIGMOIDF, inf) == 1.0
    # tanh
    assert _one(O.FN_TANHF, inf) == 1.0 and _one(O.FN_TANHF, -inf) == -1.0
    assert M.bits(_one(O.FN_TANHF, -0.0)) == 0                                  # +0, not -0
    assert M.bits(_one(O.FN_TANHF, 0.0)) == 0
    # NaN in, NaN out — for everything built on expf, and for the central branch of the quantile
    for fn in (O.FN_EXPF, O.FN_SIGMOIDF, O.FN_TANHF, O.FN_NORMAL_ICDF):
        assert np.isnan(_one(fn, nan)), fn
    # logf reads the exponent and mantissa fields and never looks at the class: finite garbage for 0, subnormals, negatives, inf AND NaN
    garbage = {0.0: -88.02969, 1e-40: -88.02122, -2.0: 178.13882, float(inf): 88.72284, float(nan): 89.1283}
    for x, want in garbage.items():
        got = _one(O.FN_LOGF, x)
        assert np.isfinite(got) and got == F32(want), (x, got)
    assert _one(O.FN_LOGISTIC, nan) == 0.0                                      # ... so the logistic of NaN is logf(NaN) - logf(NaN)


    assert _one(O.FN_NORMAL_ICDF, 0.0) == F32(-13.003056) and _one(O.FN_NORMAL_ICDF, 1.0) == F32(13.003056)   # ... and of logf(0) in the tails


def _table_row(text, name):
    m = re.search(r'^[ */|]*`?ttsc_%s`?\s*\|(.*)$' % name, text, flags=re.M)
    assert m, 'no table row for ttsc_%s' % name
    return m.group(1)


@pytest.mark.parametrize('doc', ['include/ttscube_math.h', 'DESIGN.md'])
def test_documents_print_the_asserted_figures(doc):
    text = open(os.path.join(ROOT, doc)).read()
    for name, figs in TABLE.items():
        cells = []
        for c in _table_row(text, name).split('|'):
            try:
                cells.append(float(c))
            except ValueError:
                pass
        for f in figs:
            assert f in cells, (doc, name, f, cells)
