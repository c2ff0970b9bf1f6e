"""GPU: the GEMM family of csrc/gemm.hip and the two mat-vecs, per element against float64 (tests/gemm_reference.py; the yardstick itself is
checked without a GPU in tests/test_gemm_reference_cpu.py):

    |got - ref64| <= 2^-20 * S + 1e-30,     S = |A| . |B| (+ |bias| + |C0|)       (through an activation: x its Lipschitz constant)

no absolute floor, so every operand scale is held to the same relative bound.  2^-20 is 4 x the worst ratio of a serial float32 evaluation
at these shapes (2^-22.6 .. 2^-21.8); every defect the CPU test injects exceeds 2^-16.

  ttsc_linear_forward_split   scale sweep x ~ 2^sx, w ~ 2^sw (sx in +10 .. -12, sw in 0 .. -14), embedding-like mixed scales, |v| next to
                              65504; ldx > K, ldy > N, accumulate, activations, lengths / period with half-padding tiles
  ttsc_linear_forward         M, N around one tile, K around the k-slice; the float4 path and the scalar path by each of its triggers
                              (K % 4, ldx % 4, a pointer one float off); overlapping rows (ldx < K); ldy > N; accumulate; activations
  ttsc_gemm                   NN / TN / NT / TT at one split (K = 17, 260) and split-K (K = 1040: 5 splits of 208); odd leading dimensions,
                              pointers one float off, ldc > N, accumulate; row shifts -1, +1, -3, +3 at period 13 and period K; the guard
  ttsc_colsum, ttsc_matvec    around the parts switches

Measured on an MI355X, worst err / S per kernel and path (every test prints its own as `MEASURED <key> 2^<log2>`):
  split linear      sweep 2^-23.2 .. 2^-22.3 over all 50 (K, sx, sw) cells (K = 36: 2^-22.3, K = 256: 2^-22.7); mixed scales 2^-20.9 (K = 36) and
                    2^-21.4 (K = 256) — one or two products carry such a sum, so their 2^-22 each does not average out; next to 65504 2^-23.9;
                    ldx / ldy 2^-22.7; lengths 2^-23.2; activations none / relu 2^-22.7, tanh 2^-23.5, sigmoid 2^-24.7
                    (the kernel before the low half was scaled, same cases: 2^-20.1 at w ~ 2^-7, 2^-16.1 at 2^-11, 2^-19.2 at x ~ 2^-8,
                    2^-15.3 at x ~ 2^-12 for K = 256, 2^-18.5 / 2^-17.7 / 2^-13.8 for K = 36, and 2^-10.4 on the mixed case: 12 cases failed)
  exact linear      float4 2^-22.0, scalar by K % 4 2^-22.2, by ldx % 4 2^-22.2, by an x / w pointer one float off 2^-22.6; overlapping rows
                    2^-22.0; activations none 2^-22.5, relu 2^-22.9, tanh 2^-23.1, sigmoid 2^-24.8
  ttsc_gemm         one split NN 2^-22.1, TN 2^-22.2, NT 2^-22.0, TT 2^-22.1; split-K NN 2^-23.7, TN 2^-23.5, NT 2^-23.6, TT 2^-23.8;
                    row-shifted TN 2^-23.6 (and the rows it reads are exactly those of the materialised h_prev)
  ttsc_colsum       one part 2^-24.0, four / five parts 2^-25.4          ttsc_matvec    W x 2^-24.6, W^T u 2^-23.0
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ACTS = (None, 'relu', 'tanh', 'sigmoid')
MEASURED = {}


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), ratio)
    print('MEASURED %-34s 2^%.1f' % (key, R.log2_ratio(ratio)))


def _hold(got, ref, S, key, act=None):
    """note the worst err / S under `key`, then assert the bound"""
    got = R.f64(got)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    ratio = R.worst_ratio(got, ref, S)
    _note(key, ratio)
    assert R.within(got, ref, S, act=act), '%s: worst err / S = 2^%.1f' % (key, R.log2_ratio(ratio))


def _L():
    from ttscube_amd import _lib
    return _lib, _lib.lib()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _place(rows, ld, off=0, fill=float('nan')):
    """a flat device buffer with rows[r] at off + r * ld, NaN everywhere else: whatever a kernel reads outside its operand poisons the result"""
    rows = np.asarray(rows, np.float32)
    n, c = rows.shape
    buf = np.full(off + (n - 1) * ld + max(c, ld) + 8, fill, np.float32)
    for r in range(n):
        buf[off + r * ld:off + r * ld + c] = rows[r]
    return torch.from_numpy(buf).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ybuf(M, N, ldy, y0):
    y = torch.full((M, ldy), SENTINEL, dtype=torch.float32)
    if y0 is not None:
        y[:, :N] = torch.from_numpy(np.asarray(y0, np.float32))
    return y.cuda()


def _tail_untouched(y, N):
    return bool((_bits(y[:, N:]) == _bits(torch.full_like(y[:, N:], SENTINEL))).all())


def _linear_raw(x, w, bias, M, N, K, ldx=None, ldy=None, x_off=0, w_off=0, act=None, y0=None, split=False, lengths=None, period=0, xflat=None):
    """ttsc_linear_forward(_split) through the C ABI: x [M, K] rows placed at stride ldx (or xflat: a flat signal read as overlapping rows),
    y [M, ldy] sentinel-filled (y0 in its first N columns under accumulate).  Returns the whole y buffer."""
    from ttscube_amd.hip_layers import ACT
    _lib, L = _L()
    ldx = K if ldx is None else ldx
    ldy = N if ldy is None else ldy
    if xflat is not None:
        xb = torch.from_numpy(np.concatenate([np.full(x_off, np.nan, np.float32), np.asarray(xflat, np.float32)])).cuda()
    else:
        xb = _place(x, ldx, x_off)
    wb = _place(w, K, w_off)
    bb = torch.from_numpy(np.asarray(bias, np.float32)).cuda() if bias is not None else None
    y = _ybuf(M, N, ldy, y0)
    head = (_ptr(xb, x_off), _ptr(wb, w_off), _ptr(bb) if bb is not None else None, _ptr(y), M, N, K, ldx, ldy, ACT[act], int(y0 is not None))
    if split:
        ld = torch.tensor(lengths, dtype=torch.int32).cuda() if lengths is not None else None
        _lib.check(L.ttsc_linear_forward_split(*head, _ptr(ld) if ld is not None else None, period, _lib.current_stream()), 'split')
    else:
        _lib.check(L.ttsc_linear_forward(*head, _lib.current_stream()), 'linear')
    torch.cuda.synchronize()
    return y


def _split_status():
    return int(_L()[1].ttsc_gemm_split_status())


# ---- B: the split-precision linear ---------------------------------------------------------------------------------------------------------

def _split_hip(x, w, b, monkeypatch=None, **kw):
    """linear_hip(split=True), and proof that the split kernel (not the exact one) took the call"""
    from ttscube_amd.hip_layers import linear_hip
    _lib, L = _L()
    calls = []
    if monkeypatch is not None:
        real = L.ttsc_linear_forward_split
        monkeypatch.setattr(L, 'ttsc_linear_forward_split', lambda *a: calls.append(1) or real(*a))
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    bd = torch.from_numpy(b).cuda() if b is not None else None
    y = linear_hip(xd, wd, bd, split=True, **kw)
    again = linear_hip(xd, wd, bd, split=True, **kw)
    if monkeypatch is not None:
        assert len(calls) == 2
    return y, again


@pytest.mark.parametrize('sx', R.SPLIT_SX)
@pytest.mark.parametrize('K', R.SPLIT_KS)
def test_split_linear_holds_the_bound_at_every_operand_scale(K, sx, monkeypatch):
    assert _split_status() == 0
    for sw in R.SPLIT_SW:
        x, w, b = R.sweep_operands(K, sx, sw)
        ref, S, _ = R.linear_f64(x, w, b)
        y, again = _split_hip(x, w, b, monkeypatch if sw == 0 else None)
        _hold(y, ref, S, 'split sweep K=%d' % K)
        _note('split x 2^%d w 2^%d' % (sx, sw), R.worst_ratio(y, ref, S))
        assert torch.equal(y, again), (sx, sw)
    assert _split_status() == 0


@pytest.mark.parametrize('K', R.SPLIT_KS)
def test_split_linear_mixed_scales_and_the_top_of_the_fp16_range(K, monkeypatch):
    assert _split_status() == 0
    for name, (x, w, b) in (('mixed', R.mixed_operands(K)), ('edge', R.edge_operands(K))):
        ref, S, _ = R.linear_f64(x, w, b)
        y, again = _split_hip(x, w, b, monkeypatch if name == 'mixed' else None)
        _hold(y, ref, S, 'split ' + name)
        assert torch.equal(y, again), name
        assert _split_status() == 0, name            # a scaled low half next to 65504 stays finite, and the range word stays clear


@pytest.mark.parametrize('K,ldx,ldy', [(36, 40, 129), (36, 36, 133), (256, 260, 131)])
def test_split_linear_leading_dimensions(K, ldx, ldy):
    M, N = R.SPLIT_M, R.SPLIT_N
    x, w, b = R.sweep_operands(K, -4, -7)
    ref, S, _ = R.linear_f64(x, w, b)
    y = _linear_raw(x, w, b, M, N, K, ldx=ldx, ldy=ldy, split=True)
    _hold(y[:, :N], ref, S, 'split ldx / ldy')
    assert _tail_untouched(y, N)
    assert torch.equal(y, _linear_raw(x, w, b, M, N, K, ldx=ldx, ldy=ldy, split=True))
    assert _split_status() == 0


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('bias', [True, False])
def test_split_linear_accumulate_and_activations(bias, act):
    M, N, K = R.SPLIT_M, R.SPLIT_N, 36
    x, w, b = R.sweep_operands(K, 0, -3)
    b = b if bias else None
    y0 = np.random.RandomState(8).randn(M, N).astype(np.float32)
    for acc0 in (None, y0):
        ref, S, _ = R.linear_f64(x, w, b, act, acc0)
        y = _linear_raw(x, w, b, M, N, K, ldy=N + 1, act=act, y0=acc0, split=True)
        _hold(y[:, :N], ref, S, 'split act %s' % act, act=act)
        assert _tail_untouched(y, N)
    assert _split_status() == 0


def test_split_linear_skips_only_tiles_that_are_all_padding():
    """B = 3 utterances of period 192 = 576 rows = 128-row tiles 0 .. 4; lengths [192, 0, 64]: tile 1 is half utterance 0's live tail and half
    utterance 1's padding, tile 3 half live rows of utterance 2 and half its padding — both must be computed; tile 2 (utterance 1 only) and
    the partial tile 4 (utterance 2's rows 128 ..) are padding only and stay unwritten"""
    T, K, N = 192, 64, 129
    lens = [192, 0, 64]
    rng = np.random.RandomState(4)
    x = (rng.randn(3 * T, K) * 2.0 ** -6).astype(np.float32)
    w = (rng.randn(N, K) * 2.0 ** -5).astype(np.float32)
    b = rng.randn(N).astype(np.float32) * np.float32(2.0 ** -8)
    ref, S, _ = R.linear_f64(x, w, b)
    full = _linear_raw(x, w, b, 3 * T, N, K, split=True)
    _hold(full, ref, S, 'split lengths')
    y = _linear_raw(x, w, b, 3 * T, N, K, ldy=N + 2, split=True, lengths=lens, period=T)
    assert _tail_untouched(y, N)
    for u, n in enumerate(lens):
        assert torch.equal(y[u * T:u * T + n, :N], full[u * T:u * T + n]), u            # live rows: the bits of the unmasked run
    assert torch.equal(y[128:256, :N], full[128:256]) and torch.equal(y[384:512, :N], full[384:512])   # the half-padding tiles ran whole
    for lo, hi in ((256, 384), (512, 576)):
        assert bool((_bits(y[lo:hi]) == _bits(torch.full_like(y[lo:hi], SENTINEL))).all()), lo
    assert _split_status() == 0


# ---- C: the exact fp32 kernels -----------------------------------------------------------------------------------------------------------------

def _lin_case(M, N, K, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(M, K).astype(np.float32), (rng.randn(N, K) / np.sqrt(K)).astype(np.float32), rng.randn(N).astype(np.float32)


@pytest.mark.parametrize('K', [15, 16, 17, 33, 64])
def test_linear_tile_edges(K):
    for M in (127, 128, 129):
        for N in (127, 128, 129):
            x, w, b = _lin_case(M, N, K, M * N + K)
            ref, S, _ = R.linear_f64(x, w, b)
            y = _linear_raw(x, w, b, M, N, K)
            _hold(y, ref, S, 'linear %s' % ('float4' if K % 4 == 0 else 'scalar K%4'))


@pytest.mark.parametrize('path,K,ldx,x_off,w_off', [
    ('float4', 36, 36, 0, 0), ('float4', 36, 40, 0, 0), ('float4', 64, 64, 4, 8),
    ('scalar K%4', 33, 36, 0, 0), ('scalar ldx%4', 36, 37, 0, 0), ('scalar x ptr', 36, 36, 1, 0), ('scalar w ptr', 36, 36, 0, 1),
    ('scalar ldx%4', 36, 39, 3, 2)])
def test_linear_vector_and_scalar_paths(path, K, ldx, x_off, w_off):
    """the float4 loads need K % 4 == 0, ldx % 4 == 0 and 16-byte aligned x and w; each condition alone sends the call to the scalar kernel"""
    M, N = 130, 129
    x, w, b = _lin_case(M, N, K, K + ldx)
    y0 = np.random.RandomState(2).randn(M, N).astype(np.float32)
    for acc0 in (None, y0):
        ref, S, _ = R.linear_f64(x, w, b, None, acc0)
        y = _linear_raw(x, w, b, M, N, K, ldx=ldx, ldy=N + 3, x_off=x_off, w_off=w_off, y0=acc0)
        _hold(y[:, :N], ref, S, 'linear ' + path)
        assert _tail_untouched(y, N)
        assert torch.equal(y, _linear_raw(x, w, b, M, N, K, ldx=ldx, ldy=N + 3, x_off=x_off, w_off=w_off, y0=acc0))


@pytest.mark.parametrize('ldx,x_off', [(8, 0), (7, 0), (8, 1)])
def test_linear_overlapping_rows(ldx, x_off):
    """ldx < K: row m starts ldx floats after row m - 1 (the STFT frames a signal this way)"""
    M, N, K = 130, 70, 36
    rng = np.random.RandomState(ldx)
    sig = rng.randn((M - 1) * ldx + K).astype(np.float32)
    w = rng.randn(N, K).astype(np.float32)
    x = R.overlapping_rows(sig, M, K, ldx)
    ref, S, _ = R.linear_f64(x, w)
    y = _linear_raw(None, w, None, M, N, K, ldx=ldx, x_off=x_off, xflat=sig)
    _hold(y, ref, S, 'linear overlapping %s' % ('float4' if ldx % 4 == 0 and x_off == 0 else 'scalar'))


@pytest.mark.parametrize('act', ACTS)
def test_linear_activations(act):
    M, N, K = 129, 130, 33
    x, w, b = _lin_case(M, N, K, 12)
    y0 = np.random.RandomState(3).randn(M, N).astype(np.float32)
    for acc0 in (None, y0):
        ref, S, _ = R.linear_f64(x, w, b, act, acc0)
        y = _linear_raw(x, w, b, M, N, K, act=act, y0=acc0)
        _hold(y, ref, S, 'linear act %s' % act, act=act)


def _gemm_raw(a, b, ta, tb, M, N, K, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c0=None, shift=0, period=0):
    """ttsc_gemm through the C ABI; a, b as stored ([K, M] when ta, [N, K] when tb).  Returns (the whole C buffer, splits launched)."""
    _lib, L = _L()
    lda = a.shape[1] if lda is None else lda
    ldb = b.shape[1] if ldb is None else ldb
    ldc = N if ldc is None else ldc
    ab, bb = _place(a, lda, a_off), _place(b, ldb, b_off)
    c = _ybuf(M, N, ldc, c0)
    wsb = int(L.ttsc_gemm_workspace_bytes(M, N, K))
    splits, _ = R.gemm_splits(M, N, K)
    assert wsb == (splits * M * N * 4 if splits > 1 else 0)                  # the plan the host model states is the one that runs
    ws = torch.full((max(wsb // 4, 1),), float('nan'), device='cuda')
    _lib.check(L.ttsc_gemm(int(ta), int(tb), M, N, K, _ptr(ab, a_off), lda, _ptr(bb, b_off), ldb, _ptr(c), ldc, int(c0 is not None), shift, period,
                           _ptr(ws) if wsb else None, wsb, _lib.current_stream()), 'ttsc_gemm')
    torch.cuda.synchronize()
    return c, splits


def _odd(n):
    return n + 1 if n % 2 == 0 else n + 2


@pytest.mark.parametrize('K', [17, 260, 1040])
@pytest.mark.parametrize('ta,tb', [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_transposes_leading_dimensions_and_split_k(ta, tb, K):
    M, N = 130, 70
    rng = np.random.RandomState(K + 2 * ta + tb)
    a = rng.randn(*((K, M) if ta else (M, K))).astype(np.float32)
    b = rng.randn(*((N, K) if tb else (K, N))).astype(np.float32)
    c0 = rng.randn(M, N).astype(np.float32)
    name = 'gemm %s%s %s' % ('T' if ta else 'N', 'T' if tb else 'N', 'split-K' if K == 1040 else 'one split')
    variants = {
        'aligned': dict(lda=a.shape[1] + (-a.shape[1]) % 4, ldb=b.shape[1] + (-b.shape[1]) % 4),
        'odd ld': dict(lda=_odd(a.shape[1]), ldb=_odd(b.shape[1])),
        'offset': dict(lda=a.shape[1] + (-a.shape[1]) % 4, ldb=b.shape[1] + (-b.shape[1]) % 4, a_off=1, b_off=1),
        'ldc': dict(ldc=N + 3),
        'accumulate': dict(ldc=N + 1, c0=c0),
    }
    for v, kw in variants.items():
        ref, S = R.gemm_f64(a, b, ta, tb, acc0=kw.get('c0'))
        c, splits = _gemm_raw(a, b, ta, tb, M, N, K, **kw)
        assert splits == (5 if K == 1040 else 1)
        _hold(c[:, :N], ref, S, name)
        assert _tail_untouched(c, N), v
        assert torch.equal(c, _gemm_raw(a, b, ta, tb, M, N, K, **kw)[0]), v


@pytest.mark.parametrize('period', [13, 1040])
@pytest.mark.parametrize('shift', [-1, 1, -3, 3])
def test_gemm_row_shift_is_h_prev(shift, period):
    """dW_hh = dG^T . h_prev (TN) with K = 1040 in 5 splits of 208 rows — no multiple of the period 13, so sequences straddle the splits"""
    M, N, K = 130, 70, 1040
    rng = np.random.RandomState(40 + shift)
    a = rng.randn(K, M).astype(np.float32)
    b = rng.randn(K, N).astype(np.float32)
    c0 = rng.randn(M, N).astype(np.float32)
    for kw in (dict(), dict(ldb=_odd(N), b_off=1), dict(ldc=N + 2, c0=c0)):
        ref, S = R.gemm_f64(a, b, True, False, shift=shift, period=period, acc0=kw.get('c0'))
        c, splits = _gemm_raw(a, b, True, False, M, N, K, shift=shift, period=period, **kw)
        assert splits == 5
        _hold(c[:, :N], ref, S, 'gemm TN row shift')
        assert _tail_untouched(c, N)
    # which rows of B the contraction sees, exactly: A = the identity picks them out (products by 1 and 0 only — no rounding anywhere)
    eye = np.eye(K, dtype=np.float32)
    want = R.shift_rows(b, shift, period)
    c, _ = _gemm_raw(eye, b, True, False, K, N, K, shift=shift, period=period)
    assert np.array_equal(c.cpu().numpy(), want)
    edges = ~want.any(axis=1)
    assert int(edges.sum()) == abs(shift) * (K // period)                      # a zero block at every sequence edge and nowhere else
    r = np.arange(K) % period
    assert np.array_equal(edges, (r + shift < 0) | (r + shift >= period))


def test_gemm_refuses_a_row_shift_over_a_partial_period_before_any_launch(monkeypatch):
    """K % b_period != 0 under a forward shift would read B row K; both the wrapper and the C entry refuse it.  The C entry is only ever
    asked with a BACKWARD shift here, which reads inside B whatever the guard does: nothing out of bounds is launched by this test."""
    from ttscube_amd.hip_layers import gemm_hip
    _lib, L = _L()
    launched = []
    real = L.ttsc_gemm
    monkeypatch.setattr(L, 'ttsc_gemm', lambda *a: launched.append(a) or real(*a))
    a = torch.randn(1045, 130, device='cuda')
    b = torch.randn(1045, 70, device='cuda')
    for shift in (1, -1, 3):
        with pytest.raises(_lib.TTSCError):
            gemm_hip(a, b, trans_a=True, b_row_shift=shift, b_period=13)
    with pytest.raises(_lib.TTSCError):
        gemm_hip(a[:1040], b[:1040], trans_a=True, b_row_shift=13, b_period=13)
    assert not launched
    out = torch.full((130, 70), SENTINEL, device='cuda')
    ws = torch.empty(max(int(L.ttsc_gemm_workspace_bytes(130, 70, 1045)) // 4, 1), device='cuda')
    rc = real(1, 0, 130, 70, 1045, _ptr(a), 130, _ptr(b), 70, _ptr(out), 70, 0, -1, 13, _ptr(ws), ws.numel() * 4, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'whole periods' in L.ttsc_last_error()
    assert bool((out == SENTINEL).all())                                       # refused in the argument check: nothing ran
    gemm_hip(a[:1040], b[:1040], trans_a=True, b_row_shift=1, b_period=13)
    assert len(launched) == 1                                                  # (the spy does see a launch)


@pytest.mark.parametrize('R_', [1, 1023, 1024, 1025])
def test_colsum_around_the_parts_switch(R_):
    _lib, L = _L()
    for Cn in (63, 64, 65, 257):
        rng = np.random.RandomState(R_ + Cn)
        x = rng.randn(R_, Cn).astype(np.float32)
        o0 = rng.randn(Cn).astype(np.float32)
        for ld, acc0 in ((Cn, None), (Cn + 5, None), (Cn + 4, o0)):
            ref, S = R.colsum_f64(x, acc0)
            xb = _place(x, ld)
            out = torch.full((Cn + 3,), SENTINEL, device='cuda')
            if acc0 is not None:
                out[:Cn] = torch.from_numpy(acc0).cuda()
            wsb = int(L.ttsc_colsum_workspace_bytes(R_, Cn))
            assert wsb == R.colsum_parts(R_) * Cn * 4
            ws = torch.full((wsb // 4,), float('nan'), device='cuda')
            _lib.check(L.ttsc_colsum(_ptr(xb), R_, Cn, ld, _ptr(out), int(acc0 is not None), _ptr(ws), wsb, _lib.current_stream()), 'colsum')
            torch.cuda.synchronize()
            _hold(out[:Cn], ref, S, 'colsum %s' % ('parts' if R_ >= 1024 else 'one part'))
            assert bool((out[Cn:] == SENTINEL).all())


@pytest.mark.parametrize('cols', [255, 256, 257])
def test_matvec_both_directions_around_the_parts_switch(cols):
    _lib, L = _L()
    for rows in (1, 63, 64, 65, 1025):
        rng = np.random.RandomState(rows + cols)
        W = rng.randn(rows, cols).astype(np.float32)
        Wd = torch.from_numpy(W).cuda()
        for tr, n_in, n_out in ((0, cols, rows), (1, rows, cols)):
            v = rng.randn(n_in).astype(np.float32)
            ref, S = R.matvec_f64(W, v, bool(tr))
            out = torch.full((n_out + 2,), SENTINEL, device='cuda')
            wsb = int(L.ttsc_matvec_workspace_bytes(rows, cols))
            assert wsb == R.matvec_parts(rows) * cols * 4
            ws = torch.full((wsb // 4,), float('nan'), device='cuda')
            _lib.check(L.ttsc_matvec(_ptr(Wd), rows, cols, _ptr(torch.from_numpy(v).cuda()), tr, _ptr(out), _ptr(ws) if tr else None,
                                     wsb if tr else 0, _lib.current_stream()), 'matvec')
            torch.cuda.synchronize()
            _hold(out[:n_out], ref, S, 'matvec %s' % ('W^T u' if tr else 'W x'))
            assert bool((out[n_out:] == SENTINEL).all())
