"""GPU: include/ttscube_math.h on the device (csrc/probe.hip, built with the library's ordinary flags) against the host build of the same
header (oracle/wavernn_ref.c), bit for bit, function by function — so that a change in how the compiler rounds a division or a square root,
or treats subnormals, names the function it broke instead of "decode mismatch at step N".

The only relaxation anywhere in this file: where the host result is NaN the device result must be NaN (payload not compared).  The only
finding: ttsc_logistic of a NaN argument differs (LOGISTIC_OF_NAN below: outside the function's domain, reached by no caller, both sides
pinned as they are).  Everything else — subnormal sigmoids and gamma variates included — is equal."""
import numpy as np
import pytest
import torch

from oracle import wavernn_ref as O
from tests import math_sweep as M

pytestmark = pytest.mark.gpu

F32 = np.float32
O_LOG_SCALE_MIN = -32.23619130191664                             # TTSC_LOG_SCALE_MIN of include/ttscube_math.h
_INT_VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_INT_VIEW.get(a.dtype, a.dtype))).cuda()


def _call(name, *args):
    from ttscube_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream()), name)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def probe_math(fn, x):
    x = np.ascontiguousarray(x, dtype=np.uint32 if fn >= O.FN_U01 else np.float32)
    src, out = _dev(x), torch.empty(x.size, dtype=torch.float32, device='cuda')      # (named: the inputs must outlive the launch)
    _call('ttsc_probe_math', fn, src.data_ptr(), out.data_ptr(), x.size)
    return out.cpu().numpy()


def probe_philox(ctr, key):
    c, k, out = _dev(ctr), _dev(key), torch.empty(ctr.shape, dtype=torch.int32, device='cuda')
    _call('ttsc_probe_philox', c.data_ptr(), k.data_ptr(), out.data_ptr(), ctr.shape[0])
    return out.cpu().numpy().view(np.uint32)


def probe_noise(kind, t, b, seed):
    d = [_dev(t), _dev(b), _dev(seed)]
    out = torch.empty((t.size, O.NOISE_WIDTH[kind]), dtype=torch.float32, device='cuda')
    _call('ttsc_probe_noise', O.OUT_KIND[kind], *[a.data_ptr() for a in d], out.data_ptr(), t.size)
    return out.cpu().numpy()


def probe_sample(kind, mode, impl, y, noise=None, t=None, b=None, seed=None):
    n = y.shape[0]
    d = [_dev(a) if a is not None else None for a in (y, noise, t, b, seed)]
    wv = torch.empty(n, dtype=torch.float32, device='cuda')
    k = torch.empty(n, dtype=torch.int32, device='cuda')
    _call('ttsc_probe_sample', O.OUT_KIND[kind], mode, impl, *[_ptr(a) for a in d], wv.data_ptr(), k.data_ptr(), n)
    return wv.cpu().numpy(), k.cpu().numpy()


def _assert_same(got, want, arg, what):
    bad = np.flatnonzero(M.same_bits_or_nan(got, want).reshape(-1))
    if bad.size:
        g, w, a = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1), np.asarray(arg)
        rows = ['  %s: host %r (0x%08x)  device %r (0x%08x)' % (a[i] if a.ndim == 1 and a.size == g.size else 'element %d' % i, w[i],
                                                                 int(M.bits(w[i:i + 1])[0]), g[i], int(M.bits(g[i:i + 1])[0])) for i in bad[:8]]
        pytest.fail('%s: %d of %d results differ between host and device\n%s' % (what, bad.size, g.size, '\n'.join(rows)))


# ---- unary functions -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def xs():
    return M.float_inputs()


@pytest.fixture(scope='module')
def rs():
    return M.u32_inputs()


@pytest.mark.parametrize('fn', range(9), ids=O.FN_NAMES)
def test_unary_function_device_equals_host(fn, xs, rs):
    """one launch over the stratified and the boundary set; no input is left out — every step of these functions is an IEEE operation or an
    integer move, so host and device agree outside the documented domains as well"""
    x = rs if fn >= O.FN_U01 else xs
    if fn == O.FN_LOGISTIC:
        x = x[~np.isnan(x)]          # the one documented limit: test_logistic_of_nan_is_outside_the_contract
    _assert_same(probe_math(fn, x), O.math_array(fn, x), x, 'ttsc_' + O.FN_NAMES[fn])


# ttsc_logistic(NaN) = ttsc_logf(NaN) - ttsc_logf(1.0f - NaN), and ttsc_logf reads the BITS of its argument without testing its class.  Which sign
# and payload the NaN of `1.0f - NaN` carries is not fixed by IEEE 754: x86 returns the operand quieted with its sign kept, gfx950 subtracts by
# adding the negated operand and returns it with the sign flipped — and the sign bit is exponent bit 8 to ttsc_logf (256 ln 2 = 177.45).  No
# caller reaches this: ttsc_noise_mol and wr_sample_continuous pass ttsc_u01_clip(r), which lies in [1e-5, 1 - 1e-5] for every r
# (tests/test_shared_math_cpu.py::test_uniforms_are_exact).  Removing it would take a class test inside the header, on the decode kernels' path;
# instead the domain is documented (u must not be NaN) and both sides are pinned as they are, so that a change on either is noticed.
LOGISTIC_OF_NAN = {   # NaN bit pattern: (host bits, device bits)
    0x7fc00000: (0x00000000, 0xc3317218),   # host 0.0, device -177.44568
    0xffc00000: (0x00000000, 0x43317218),   # host 0.0, device 177.44568
    0x7f800001: (0xbecf9900, 0xc331d9e4),   # host -0.40546417, device -177.85114
    0xff800001: (0xbecf9800, 0x43310a4c),   # host -0.40545654, device 177.04022
    0x7fffffff: (0x00000000, 0xc3317218),
    0xffffffff: (0x00000000, 0x43317218),
}


def test_logistic_of_nan_is_outside_the_contract():
    u = M.floats(np.array(sorted(LOGISTIC_OF_NAN), dtype=np.uint32))
    assert np.isnan(u).all()
    host, dev = M.bits(O.math_array(O.FN_LOGISTIC, u)), M.bits(probe_math(O.FN_LOGISTIC, u))
    for p, h, d in zip(sorted(LOGISTIC_OF_NAN), host, dev):
        assert (int(h), int(d)) == LOGISTIC_OF_NAN[p], 'ttsc_logistic(NaN 0x%08x): host 0x%08x device 0x%08x' % (p, h, d)


def test_probe_argument_checks():
    from ttscube_amd import _lib
    L = _lib.lib()
    x = torch.zeros(4, device='cuda')
    s = _lib.current_stream()
    assert L.ttsc_probe_math(9, x.data_ptr(), x.data_ptr(), 4, s) == -1 and b'fn 9' in L.ttsc_last_error()
    assert L.ttsc_probe_math(0, None, x.data_ptr(), 4, s) == -1
    assert L.ttsc_probe_math(0, x.data_ptr(), x.data_ptr(), 0, s) == -1
    assert L.ttsc_probe_philox(None, x.data_ptr(), x.data_ptr(), 1, s) == -1
    assert L.ttsc_probe_noise(0, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, s) == -1
    p = x.data_ptr()
    assert L.ttsc_probe_sample(1, 1, 0, p, p, None, None, None, p, p, 1, s) == -1        # not a continuous head
    assert L.ttsc_probe_sample(3, 1, 2, p, p, None, None, None, p, p, 1, s) == -1        # impl
    assert L.ttsc_probe_sample(3, 1, 0, p, None, None, None, None, p, p, 1, s) == -1     # MODE_NOISE without noise
    assert L.ttsc_probe_sample(3, 2, 1, p, None, p, p, None, p, p, 1, s) == -1           # MODE_PHILOX without seeds


# ---- counters and noise ----------------------------------------------------------------------------------------------------------------------
def test_philox_device_equals_host_and_known_answers():
    rng = np.random.RandomState(11)
    ctr = rng.randint(0, 1 << 32, size=(65536 + 2, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.randint(0, 1 << 32, size=(65536 + 2, 2), dtype=np.uint64).astype(np.uint32)
    ctr[0], key[0] = 0, 0                                   # Random123 known answers, philox4x32-10
    ctr[1], key[1] = 0xffffffff, 0xffffffff
    got = probe_philox(ctr, key)
    assert [hex(v) for v in got[0]] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    assert [hex(v) for v in got[1]] == ['0x408f276d', '0x41c83b0e', '0xa20bc7c6', '0x6d5451fd']
    assert np.array_equal(got, O.philox_array(ctr, key))


def _noise_tuples(n=4096, seed=12):
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    t = np.array([0, 1, (1 << 24) - 1, 1 << 31, (1 << 32) - 1], dtype=np.uint32)[i % 5]
    b = np.array([0, 255, 1 << 31], dtype=np.uint32)[(i // 5) % 3]
    lo = rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    hi = rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    lo[i % 4 == 0] = 0                                       # either half zero, both halves full, and plain random keys
    hi[i % 4 == 1] = 0
    lo[i % 4 == 2] = hi[i % 4 == 2] = 0xffffffff
    return t, b, (hi << np.uint64(32)) | lo


@pytest.mark.parametrize('kind', ['mol', 'gm', 'beta'])
def test_noise_device_equals_host(kind):
    t, b, seed = _noise_tuples()
    want = O.noise_array(kind, t, b, seed)
    assert np.isfinite(want).all()
    _assert_same(probe_noise(kind, t, b, seed), want, np.arange(want.size), 'ttsc_noise_' + kind)


# ---- continuous samplers ---------------------------------------------------------------------------------------------------------------------
def _three_way(kind, mode, y, noise=None, t=None, b=None, seed=None):
    """device impl 0 (the header's sampler) and impl 1 (wr_sample_continuous) both equal the host's wr_sample_array; returns the host's"""
    wv, k = O.sample_array(kind, mode, y, noise, t, b, seed)
    for impl, what in ((0, 'header sampler on the device'), (1, 'wr_sample_continuous')):
        gwv, gk = probe_sample(kind, mode, impl, y, noise if mode == O.MODE_NOISE else None, *((t, b, seed) if mode == O.MODE_PHILOX else (None,) * 3))
        _assert_same(gwv, wv, np.arange(wv.size), '%s, %s, mode %d' % (kind, what, mode))
        assert np.array_equal(gk, k), '%s, %s, mode %d: mixture index differs at rows %s' % (kind, what, mode, np.flatnonzero(gk != k)[:8])
    return wv, k


def _random_rows(kind, n=4096, seed=21):
    rng = np.random.RandomState(seed)
    z = rng.randn(n, O.SAMPLE_SIZE[kind])
    if kind == 'mol':                                        # mixture logits | means | log-scales in [-8, 1]
        z[:, 10:20] *= 0.5
        z[:, 20:] = np.clip(-3.5 + 1.5 * z[:, 20:], -8, 1)
    elif kind == 'gm':                                       # mean | log-std in [-8, 1]
        z[:, 0] *= 0.3
        z[:, 1] = np.clip(-2.0 + z[:, 1], -8, 1)
    else:                                                    # Beta logits in [-3, 4]
        z = np.clip(0.5 + 1.2 * z, -3, 4)
    return z.astype(np.float32)


@pytest.mark.parametrize('kind', ['mol', 'gm', 'beta'])
def test_samplers_on_random_rows(kind):
    y = _random_rows(kind)
    t, b, seed = _noise_tuples(seed=22)
    t = np.random.RandomState(23).randint(0, 1 << 31, size=t.size, dtype=np.uint64).astype(np.uint32)
    noise = O.noise_array(kind, t, b, seed)
    wv1, k1 = _three_way(kind, O.MODE_NOISE, y, noise=noise)
    wv2, k2 = _three_way(kind, O.MODE_PHILOX, y, t=t, b=b, seed=seed)
    assert np.array_equal(M.bits(wv1), M.bits(wv2)) and np.array_equal(k1, k2)      # injected Philox noise == in-kernel Philox noise
    assert np.isfinite(wv1).all() and np.abs(wv1).max() <= (1.0 if kind != 'gm' else 50.0)
    if kind == 'mol':
        assert len(np.unique(k1)) == 10
    _three_way(kind, O.MODE_ARGMAX, y[:64])


def test_mol_crafted_rows():
    """exact ties of the mixture scores (lowest index wins in the oracle's sequential scan; the device takes a 16-lane butterfly), the
    log-scale clamp, and both +-1 clamps"""
    ys, nzs, want_k, want_wv = [], [], [], []

    def row(score, ls=-3.0, lg=0.5, mean=None, k=None, wv=None, negzero=None):
        y = np.zeros(30, dtype=np.float32)
        y[:10] = (np.arange(10) % 4) * 0.25 - 0.5              # exactly representable, so that y + g hits the score exactly
        y[10:20] = -0.9 + 0.2 * np.arange(10) if mean is None else mean
        y[20:] = ls
        nz = np.zeros(11, dtype=np.float32)
        nz[:10] = np.asarray(score, dtype=np.float32) - y[:10]
        nz[10] = lg
        if negzero is not None:                               # -0 + -0 is the only sum that gives -0
            y[negzero] = nz[negzero] = -0.0
        assert np.array_equal(M.bits(y[:10] + nz[:10]), M.bits(np.asarray(score, dtype=np.float32)))
        ys.append(y), nzs.append(nz), want_k.append(k), want_wv.append(wv)

    base = 1.0 - 0.125 * np.arange(10)                           # distinct, all below the tie value 2
    for tie in ([0, 9], [3, 4], [7, 8, 9], list(range(10)), [9], [1, 2, 4, 8]):
        s = base.copy()
        s[tie] = 2.0
        row(s, k=min(tie))
    s = np.full(10, -1.0)                                        # +0 on the higher component, -0 on the lower: equal, the lower wins
    s[2], s[6] = -0.0, 0.0
    row(s, k=2, negzero=2)
    one = base.copy()
    one[5] = 2.0
    lsmin = F32(O_LOG_SCALE_MIN)
    for ls in (lsmin, np.nextafter(lsmin, F32(-np.inf)), np.nextafter(lsmin, F32(0)), F32(-100.0), F32(-np.inf)):
        row(one, ls=ls, lg=3.0, k=5)
    for mean, lg, wv in ((3.0, 11.0, 1.0), (-3.0, -11.0, -1.0), (3.0, -11.0, -1.0), (-3.0, 11.0, 1.0)):
        row(one, ls=0.0, lg=lg, mean=mean, k=5, wv=wv)
    y, nz = np.stack(ys), np.stack(nzs)
    wv, k = _three_way('mol', O.MODE_NOISE, y, noise=nz)
    assert k.tolist() == want_k
    for i, w in enumerate(want_wv):
        if w is not None:
            assert wv[i] == w, (i, wv[i], w)
    clamp = [i for i, r in enumerate(ys) if r[20] <= lsmin]      # everything at or below the clamp samples like the clamp itself
    assert len(clamp) == 4 and len({int(M.bits(wv[i:i + 1])[0]) for i in clamp}) == 1



def test_gaussian_crafted_rows():
    """log-std beyond both clamps of ttsc_expf, z at zero and at 0.8 x the extremes of the quantile function"""
    ext = O.math_array(O.FN_NORMAL_ICDF, np.array([M.U01_MIN, M.U01_MAX], dtype=np.float32))
    assert ext[0] < -5 and ext[1] > 5
    zs = [F32(0.0)] + [F32(0.8) * e for e in ext] + [-(F32(0.8) * e) for e in ext]
    y = np.array([[0.25, ls] for ls in (-100.0, -87.0, 88.0, 100.0, -87.5, 88.5, 0.0) for _ in zs], dtype=np.float32)
    nz = np.array(zs * 7, dtype=np.float32).reshape(-1, 1)
    wv, _ = _three_way('gm', O.MODE_NOISE, y, noise=nz)
    assert M.bits(wv[0:5]).tolist() == M.bits(wv[5:10]).tolist() and M.bits(wv[10:15]).tolist() == M.bits(wv[15:20]).tolist()   # the clamps
    assert wv[0] == F32(0.25) and wv[10] == F32(0.25) and np.isinf(wv[11:15]).all()


def _beta_crafted():
    NV = 9
    default = [0.5, 0.3, 0.4, 0.1, 0.5, -0.2, 0.5, 0.7, 0.5]
    variants = {
        'every round has 1 + c x <= 0 (v stays 1)': [0.5] + [-1e6, 0.5] * 4,
        'only the last round is taken': [0.5] + [-1e6, 0.5] * 3 + [0.5, 0.5],
        'first round rejected, second accepted': [0.5, 3.0, 0.1, 0.1, 0.5, -0.2, 0.5, 0.7, 0.5],
        'boost uniform at its minimum': [float(M.U01_MIN)] + default[1:],
        'boost uniform at its maximum': [float(M.U01_MAX)] + default[1:],
    }
    # alpha = e^-6, 0.4, just below 1, exactly 1, just above 1, 30, e^20
    logits = [-6.0, float(np.log(0.4)), -2.0 ** -20, 0.0, 2.0 ** -20, float(np.log(30.0)), 20.0]
    rows = [(a, b, default, default) for a in logits for b in logits]
    for v in variants.values():
        rows += [(a, 0.5, v, default) for a in logits] + [(0.3, a, default, v) for a in logits] + [(a, a, v, v) for a in logits]
    clamp_lo = len(rows)
    rows.append((-6.0, 20.0, variants['boost uniform at its maximum'], default))     # s underflows: clamped to FLT_MIN
    clamp_hi = len(rows)
    rows.append((20.0, -6.0, default, variants['boost uniform at its maximum']))     # s rounds to 1: clamped to 1 - 2^-24
    y = np.array([[r[0], r[1]] for r in rows], dtype=np.float32)
    nz = np.array([r[2] + r[3] for r in rows], dtype=np.float32)
    assert nz.shape[1] == 2 * NV
    return y, nz, logits, clamp_lo, clamp_hi


def test_beta_crafted_rows():
    """both sides of the alpha < 1 boost, exhausted and late rejection rounds, the boost uniform at both ends of ttsc_u01's range, both clamps
    of s; the small-alpha rows push scale * d * v and the quotient into the subnormal range, which is the point"""
    y, nz, logits, clamp_lo, clamp_hi = _beta_crafted()
    alpha = O.math_array(O.FN_EXPF, np.array(logits, dtype=np.float32))
    assert alpha[2] < 1.0 and alpha[3] == 1.0 and alpha[4] > 1.0                     # both sides of the branch, and the branch point
    wv, _ = _three_way('beta', O.MODE_NOISE, y, noise=nz)
    assert wv[clamp_lo] == F32((np.float64(M.FLT_MIN) - 0.5) * 2.0) == F32(-1.0)
    assert wv[clamp_hi] == F32((F32(0.99999994) - F32(0.5)) * F32(2.0))
    assert not np.isnan(wv).any() and (np.abs(wv) <= 1.0).all()
    # a gamma variate of the small-alpha rows is subnormal: alpha = e^-6 with the boost uniform at its maximum gives
    # scale = expf(-87) = 1.6e-38 (the clamp), d < 1 and v = 1 at most in the exhausted-rounds row
    scale = O.math_array(O.FN_EXPF, O.math_array(O.FN_LOGF, np.array([1.0 - M.U01_MAX], dtype=np.float32)) / alpha[0])[0]
    assert scale * (alpha[0] + F32(1.0) - F32(1.0) / F32(3.0)) < M.FLT_MIN
