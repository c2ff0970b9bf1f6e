"""GPU: the small kernels text-side training runs on, per element against float64 on every dispatch path (tests/text_train_reference.py; the
yardstick itself is checked without a GPU in tests/test_text_train_reference_cpu.py):

    |got - ref64| <= tau * S + 2^-126        S = the abs-value companion of each expression, tau = 4 x the float32 host model's worst err / S

  BatchNorm -> tanh -> dropout   six channels, one regime each (benign, mean 1e3 / std 1e-2, constant, gamma 50, gamma 0, scale 1e-20) at the
                                 smallest legal shapes (n - 1 = 1), the float4 kernels (F % 4 == 0, one and several trips per thread), the
                                 scalar kernels by F % 4 and by each operand 4 bytes off a 16-byte boundary; Philox masks rebuilt on the host
  cross-entropy                  through ttsc_textcoder_loss (both heads) and ttsc_masked_ce: K = 1, 7, 63, 64, 65, 201, R = 1 and one below, at
                                 and above each grid cap, logits randn / 80 randn / one +80 among -80s, a third of the targets ignored with
                                 ignore_index inside and beyond [0, K), gradients pre-filled with NaN; the out-of-range status
  mel L1                         n = 4 and around the 512-workgroup cap, exact ties, a tail only the strided trip reaches
  tag head                       one class .. K + P = 4096 (the LDS limit), a second 128-class pass, ldx > K, ragged lengths with tiles of
                                 padding only, mixed scales, exact ties across lanes and passes, a row of NaN; with and without logits
  ttsc_dropout_scale             n = 1, 3, 4, 1025; injected and Philox masks, p = 0, the adjoint call
Every launch is repeated and must give the same bits.

Measured on an MI355X, worst err / S per operation and path (test_zz_report_measured prints them; tau in brackets).  Nothing exceeded its
bound, so no kernel changed:
  BN y            [2^-20]   2^-24.7 on every path (float4, scalar, misaligned fallback, Philox float4 / scalar)
  BN statistics   [2^-19]   mean 2^-24.2, invstd 2^-24.5, running mean 2^-23.5, running variance 2^-23.6 (scalar) / 2^-24.1 (float4)
  BN dx           [2^-21]   float4 2^-23.5, scalar 2^-23.4, misaligned 2^-23.9, Philox 2^-23.7 (float4) / 2^-24.2 (scalar)
  BN dgamma/dbeta [2^-21]   float4 2^-25.0 / 2^-23.5, scalar 2^-26.3 / 2^-23.7, misaligned 2^-27.8 / 2^-24.5, Philox 2^-26.6 / 2^-24.8
  CE value        [2^-19]   below the caps 2^-25.0, at 2^-26.1, beyond 2^-26.0 (duration, pitch and ttsc_masked_ce alike)
  CE gradient     [2^-21]   2^-23.3 .. 2^-23.5 below, at and beyond every cap; rows left out are written zeros
  L1 value        [2^-9]    n = 4 2^-24.9, below the cap 2^-24.9, at 2^-24.8, beyond 2^-25.7 (tau is the one-at-a-time float32 sum's)
  L1 gradient     [2^-24]   2^-38 (n next to 2^21), exact where n is a power of two; zeros exactly at the ties
  tag logits      [2^-19]   P = 1 2^-25.1, P = 7 2^-23.6, P = 129 2^-22.6, P = 300 2^-22.7, K + P = 4096 2^-22.3, ldx 2^-23.2, ragged 2^-22.5,
                            mixed scales 2^-22.0, ties 2^-23.1; no row's float64 top two were within the bound of each other
  dropout_scale   [2^-21]   2^-23.5 (injected and Philox, forward and adjoint); p = 0 returns the bits of x
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import text_train_reference as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 4                      # floats of NaN in front of and behind every placed operand
MEASURED = {}


def _L():
    from ttscube_amd import _lib
    return _lib, _lib.lib()


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), ratio)


def _hold(op, key, got, ref, S):
    """note the worst err / S under `key`, then assert the bound of operation `op`"""
    got, ref, S = R.f64(got), np.asarray(ref, np.float64), np.asarray(S, np.float64)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    ratio = R.worst_ratio(got, ref, S)
    _note(key, ratio)
    print('MEASURED %-40s 2^%.1f' % (key, R.log2_ratio(ratio)))
    assert R.within(got, ref, S, R.TAU[op]), '%s: worst err / S = 2^%.1f, tau = 2^%d' % (key, R.log2_ratio(ratio), int(np.log2(R.TAU[op])))


class Buf:
    """a float32 operand on the device inside NaN guards, `off` floats (4 bytes each) past the allocation's 16-byte aligned start"""

    def __init__(self, a=None, shape=None, off=0, fill=NAN):
        a = np.full(shape, fill, np.float32) if a is None else np.asarray(a, np.float32)
        self.shape, self.off, self.n = a.shape, GUARD + off, a.size
        host = np.full(self.n + 2 * GUARD + off, NAN, np.float32)
        host[self.off:self.off + self.n] = a.reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * self.off)

    def get(self):
        return self.t[self.off:self.off + self.n].cpu().numpy().reshape(self.shape)

    def guards_untouched(self):
        h = self.t.cpu().numpy()
        return bool(np.isnan(h[:self.off]).all() and np.isnan(h[self.off + self.n:]).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- BatchNorm -> tanh -> dropout ----------------------------------------------------------------------------------------------------------------

def _bn_run(c, off=None, philox=None):
    """forward + backward through the C ABI -> {name: array}; off: {operand: floats off alignment}; philox: (seed, layer) instead of c['mask']"""
    _lib, L = _L()
    off = off or {}
    B, C_, F = c['x'].shape
    x, dy = Buf(c['x'], off=off.get('x', 0)), Buf(c['dy'], off=off.get('dy', 0))
    mask = None if philox else Buf(c['mask'], off=off.get('mask', 0))
    g, b = Buf(c['gamma']), Buf(c['beta'])
    rm, rv = Buf(c['rm0']), Buf(c['rv0'])
    y, dx = Buf(shape=c['x'].shape, off=off.get('y', 0)), Buf(shape=c['x'].shape, off=off.get('dx', 0))
    mean, inv, dg, db = (Buf(shape=(C_,)) for _ in range(4))
    seed, layer = philox or (0, 0)
    s = _lib.current_stream()
    _lib.check(L.ttsc_bn_tanh_dropout_train_forward(x.ptr, g.ptr, b.ptr, rm.ptr, rv.ptr, B, C_, F, 0.1, 1e-5, c['p'], mask.ptr if mask else None, seed,
                                                    layer, y.ptr, mean.ptr, inv.ptr, s), 'bn forward')
    _lib.check(L.ttsc_bn_tanh_dropout_train_backward(dy.ptr, x.ptr, g.ptr, b.ptr, mean.ptr, inv.ptr, B, C_, F, c['p'], mask.ptr if mask else None, seed,
                                                     layer, dx.ptr, dg.ptr, db.ptr, s), 'bn backward')
    torch.cuda.synchronize()
    bufs = dict(y=y, mean=mean, invstd=inv, rmean=rm, rvar=rv, dx=dx, dgamma=dg, dbeta=db)
    for k, v in bufs.items():
        assert v.guards_untouched(), k
    return {k: v.get() for k, v in bufs.items()}


def _bn_check(c, path, **kw):
    got, again = _bn_run(c, **kw), _bn_run(c, **kw)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), (path, k)
    if kw.get('philox'):
        B, C_, F = c['x'].shape
        c = dict(c, mask=R.bn_philox_mask(B, C_, F, c['p'], *kw['philox']))
        assert np.array_equal(got['y'] == 0, c['mask'] == 0)                  # the kernel drew exactly the documented mask
        assert 0 < (c['mask'] == 0).sum() < c['mask'].size
    ref = R.bn_f64(**c)
    for k in ref:
        _hold(R.BN_GROUP[k], 'bn %s %s' % (path, k), got[k], *ref[k])
    assert np.array_equal(got['y'] == 0, c['mask'] == 0)
    assert not got['dx'][:, 4].any()                                          # gamma = 0: exact zeros
    return got


@pytest.mark.parametrize('B,F', R.BN_SHAPES[:-1])
def test_bn_block_holds_the_bound_in_every_regime(B, F):
    _bn_check(R.bn_case(B, F), 'float4' if F % 4 == 0 else 'scalar')


@pytest.mark.parametrize('which', ['x', 'y', 'dy', 'dx', 'mask'])
def test_bn_block_falls_back_to_scalar_on_a_misaligned_operand(which):
    """F % 4 == 0 with one operand 4 bytes past a 16-byte boundary: that pass takes the scalar kernel, and nothing outside the operand is
    touched (x and the mask misalign both passes, y the forward, dy and dx the backward)"""
    _bn_check(R.bn_case(2, 8), 'misaligned', off={which: 1})


def test_bn_block_refuses_a_single_value_per_channel():
    _lib, L = _L()
    c = R.bn_case(1, 2)
    one = dict(c, x=c['x'][:, :, :1], dy=c['dy'][:, :, :1], mask=c['mask'][:, :, :1])
    with pytest.raises(_lib.TTSCError, match='more than 1 value'):
        _bn_run(one)


@pytest.mark.parametrize('B,F', [(3, 8), (5, 7)])
def test_bn_block_philox_mask_is_the_host_rebuild(B, F):
    _bn_check(R.bn_case(B, F), 'philox ' + ('float4' if F % 4 == 0 else 'scalar'), philox=(0x1234567887654321, 2))


# ---- the loss launch ---------------------------------------------------------------------------------------------------------------------------------

def _tc_loss(dur, pitch, mel, ignore):
    """ttsc_textcoder_loss through the C ABI.  dur / pitch: (logits [R, K], targets) or None (R = 0); mel: (pre, post, target) flat.
    -> (out [4], g_dur, g_pitch, g_pre, g_post, status)"""
    _lib, L = _L()
    heads = []
    for h in (dur, pitch):
        if h is None:
            heads.append((None, None, None, 0, 0))
        else:
            x, t = h
            heads.append((Buf(x), torch.from_numpy(np.asarray(t, np.int64)).cuda(), Buf(shape=x.shape), x.shape[0], x.shape[1]))
    pre, post, tm = (Buf(a) for a in mel)
    n = pre.n
    gpre, gpost = Buf(shape=(n,)), Buf(shape=(n,))
    out = Buf(shape=(4,))
    status = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    wsb = int(L.ttsc_textcoder_loss_workspace_bytes(heads[0][3], heads[1][3], n))
    assert wsb == R.tc_loss_workspace_bytes(heads[0][3], heads[1][3], n)
    ws = torch.full((wsb // 8,), NAN, dtype=torch.float64, device='cuda')
    (xd, td, gd, Rd, Kd), (xp, tp, gp, Rp, Kp) = heads
    _lib.check(L.ttsc_textcoder_loss(xd.ptr if xd else None, _p(td), Rd, Kd, xp.ptr if xp else None, _p(tp), Rp, Kp, pre.ptr, post.ptr, tm.ptr, n,
                                     ignore, out.ptr, gd.ptr if gd else None, gp.ptr if gp else None, gpre.ptr, gpost.ptr, _p(status), _p(ws), wsb,
                                     _lib.current_stream()), 'ttsc_textcoder_loss')
    torch.cuda.synchronize()
    for b in (out, gd, gp, gpre, gpost):
        assert b is None or b.guards_untouched()
    return out.get(), gd.get() if gd else None, gp.get() if gp else None, gpre.get(), gpost.get(), int(status.item())


def _masked_ce(x, t, ignore):
    """ttsc_masked_ce through the C ABI -> (loss, dlogits, status word of the launch)"""
    _lib, L = _L()
    Rn, K = x.shape
    xb, g, out = Buf(x), Buf(shape=x.shape), Buf(shape=(1,))
    td = torch.from_numpy(np.asarray(t, np.int64)).cuda()
    status = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    wsb = int(L.ttsc_masked_ce_workspace_bytes(Rn))
    assert wsb == R.masked_ce_workspace_bytes(Rn)
    ws = torch.full((wsb // 8,), NAN, dtype=torch.float64, device='cuda')
    _lib.check(L.ttsc_masked_ce(xb.ptr, _p(td), Rn, K, ignore, out.ptr, g.ptr, _p(status), _p(ws), wsb, _lib.current_stream()), 'ttsc_masked_ce')
    torch.cuda.synchronize()
    assert g.guards_untouched() and out.guards_untouched()
    return float(out.get()[0]), g.get(), int(status.item())


MEL4 = (np.array([1.0, -2.0, 0.5, 3.0], np.float32), np.array([0.0, 1.0, 0.5, -1.0], np.float32), np.array([0.5, -1.0, 0.5, 1.0], np.float32))


def _same_bits(a, b):
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert np.array_equal(u.view(np.int32), v.view(np.int32))
        elif not (isinstance(u, float) and np.isnan(u) and np.isnan(v)):
            assert u == v


def _ce_check(key, value, grad, x, t, ignore, empty):
    v, S_v, g, S_g = R.ce_f64(x, t, ignore, empty)
    if np.isnan(v):
        assert np.isnan(value), key
    else:
        _hold('ce_value', key + ' value', np.asarray(value), v, S_v)
    _hold('ce_grad', key + ' grad', grad, g, S_g)
    assert not grad[~R.ce_valid(t, x.shape[1], ignore)].any(), key            # rows left out: written, and zero


@pytest.mark.parametrize('K', R.CE_KS)
def test_cross_entropy_through_the_textcoder_loss(K):
    for Rd, Rp in zip(R.CE_ROWS['dur'], R.CE_ROWS['pitch']):
        for inside in (False, True):
            xd, td, ignore = R.ce_case(Rd, K, inside)
            xp, tp, _ = R.ce_case(Rp, K, inside, seed=1)
            got = _tc_loss((xd, td), (xp, tp), MEL4, ignore)
            _same_bits(got, _tc_loss((xd, td), (xp, tp), MEL4, ignore))
            out, gd, gp, gpre, gpost, status = got
            assert status == 0
            where = 'at cap' if Rd == 1024 else 'below cap' if Rd < 1024 else 'beyond cap'
            _ce_check('ce dur %s' % where, out[0], gd, xd, td, ignore, 'nan')
            _ce_check('ce pitch %s' % where, out[1], gp, xp, tp, ignore, 'nan')
            assert out[2] == np.float32(0.875) and out[3] == np.float32(1.125)                  # mean |d| of MEL4: exact in float32
            assert np.array_equal(gpre, np.float32([0.25, -0.25, 0.0, 0.25])) and np.array_equal(gpost, np.float32([-0.25, 0.25, 0.0, -0.25]))


@pytest.mark.parametrize('K', R.CE_KS)
def test_cross_entropy_through_masked_ce(K):
    _, L = _L()
    L.ttsc_phonemizer_status()                                                # (clears whatever an earlier test left in the sticky word)
    for Rn in R.CE_ROWS['masked']:
        for inside in (False, True):
            x, t, ignore = R.ce_case(Rn, K, inside, seed=2)
            got = _masked_ce(x, t, ignore)
            _same_bits(got, _masked_ce(x, t, ignore))
            value, grad, status = got
            assert status == 0
            where = 'at cap' if Rn == 2048 else 'below cap' if Rn < 2048 else 'beyond cap'
            if not R.ce_valid(t, K, ignore).any():
                assert value == 0.0 and not grad.any()                        # this entry's convention for no valid row
            _ce_check('ce masked %s' % where, value, grad, x, t, ignore, 'zero')
    assert int(L.ttsc_phonemizer_status()) == 0


def test_an_out_of_range_target_is_left_out_reported_and_forgotten():
    _, L = _L()
    L.ttsc_phonemizer_status()
    K = 7
    xd, td, ignore = R.ce_case(1025, K, False, bad_row=1024)                 # the bad row is one only a workgroup's second trip reaches
    xp, tp, _ = R.ce_case(2049, K, False, seed=1)
    out, gd, gp, _, _, status = _tc_loss((xd, td), (xp, tp), MEL4, ignore)
    assert status == 1 and not gd[1024].any()
    _ce_check('ce bad target', out[0], gd, xd, td, ignore, 'nan')
    _ce_check('ce bad target', out[1], gp, xp, tp, ignore, 'nan')
    tp_bad = tp.copy()
    tp_bad[5] = -3
    clean_d = R.ce_case(1025, K, False)
    out, gd, gp, _, _, status = _tc_loss(clean_d[:2], (xp, tp_bad), MEL4, ignore)
    assert status == 2 and not gp[5].any()
    _ce_check('ce bad target', out[1], gp, xp, tp_bad, ignore, 'nan')
    assert _tc_loss(clean_d[:2], (xp, tp), MEL4, ignore)[5] == 0              # the next launch is clean
    value, grad, status = _masked_ce(xd, td, ignore)
    assert status == 2 and not grad[1024].any()
    _ce_check('ce bad target', value, grad, xd, td, ignore, 'zero')
    assert int(L.ttsc_phonemizer_status()) == 2 and int(L.ttsc_phonemizer_status()) == 0       # sticky until read, then cleared
    assert _masked_ce(*clean_d)[2] == 0 and int(L.ttsc_phonemizer_status()) == 0


@pytest.mark.parametrize('n', R.L1_NS)
def test_mel_l1_around_the_grid_cap(n):
    pre, post, t = R.l1_case(n)
    got = _tc_loss(None, None, (pre, post, t), 0)
    _same_bits(got[2:], _tc_loss(None, None, (pre, post, t), 0)[2:])
    out, _, _, gpre, gpost, status = got
    assert status == 0 and np.isnan(out[0]) and np.isnan(out[1])              # no rows at all in either head: torch's mean over nothing
    where = 'n=4' if n == 4 else 'at cap' if n == R.L1_CAP_N else 'below cap' if n < R.L1_CAP_N else 'beyond cap'
    for a, value, grad in ((pre, out[2], gpre), (post, out[3], gpost)):
        v, S_v, g, S_g = R.l1_f64(a, t)
        _hold('l1_value', 'l1 value %s' % where, np.asarray(value), v, S_v)
        _hold('l1_grad', 'l1 grad %s' % where, grad, g, S_g)
        assert np.array_equal(grad == 0, g == 0) and (g == 0).sum() == sum(1 for i in R.L1_TIES if i + 1 < n)


# ---- tag head ----------------------------------------------------------------------------------------------------------------------------------------

def _tag_run(c, want_logits=True):
    _lib, L = _L()
    x, W = c['x'], c['W']
    M, K = x.shape
    P, ldx = W.shape[0], c['ldx']
    rows = np.full((M, ldx), NAN, np.float32)
    ok = R.tag_valid(M, c['lens'], c['period'])
    rows[ok, :K] = x[ok]                                                       # padding rows stay NaN: they must enter the tile as zeros
    xb, wb, bb = Buf(rows), Buf(W), Buf(c['b'])
    lens = torch.from_numpy(c['lens']).cuda() if c['lens'] is not None else None
    tags = torch.full((M + 2,), -1, dtype=torch.int32, device='cuda')
    lg = Buf(shape=(M, P)) if want_logits else None
    _lib.check(L.ttsc_tag_argmax(xb.ptr, wb.ptr, bb.ptr, _p(lens), c['period'], M, P, K, ldx, _p(tags), lg.ptr if lg else None, _lib.current_stream()),
               'ttsc_tag_argmax')
    torch.cuda.synchronize()
    tags = tags.cpu().numpy()
    assert (tags[M:] == -1).all() and (lg is None or lg.guards_untouched())
    return tags[:M], lg.get() if lg else None


@pytest.mark.parametrize('name', R.TAG_CASES)
def test_tag_head_logits_and_first_maximum(name):
    c = R.tag_case(name)
    lg, S, want, amb = R.tag_f64(c['x'], c['W'], c['b'], c['lens'], c['period'])
    tags, got = _tag_run(c)
    again = _tag_run(c)
    assert np.array_equal(tags, again[0]) and np.array_equal(got.view(np.int32), again[1].view(np.int32))
    fin = np.isfinite(lg)
    assert np.array_equal(np.isnan(got), ~fin)
    path = name if name in ('ldx', 'ragged', 'mixed', 'ties', 'nan') else 'P=%d K=%d' % c['W'].shape
    _hold('tag_logits', 'tag logits ' + path, np.where(fin, got, 0.0), np.where(fin, lg, 0.0), np.where(fin, S, 0.0))
    assert amb.mean() <= R.TAG_AMBIGUOUS_CAP
    assert np.array_equal(tags[~amb], want[~amb]), (tags, want)
    ok = R.tag_valid(len(want), c['lens'], c['period'])
    assert not tags[~ok].any() and not got[~ok].any()
    if name == 'ties':
        assert (tags == R.TAG_TIE_CLASSES[0]).all()
        assert all(np.array_equal(got[:, p], got[:, R.TAG_TIE_CLASSES[0]]) for p in R.TAG_TIE_CLASSES)
    if name == 'nan':
        assert tags[2] == 0
    else:
        assert np.array_equal(_tag_run(c, want_logits=False)[0], tags)


def test_tag_head_refuses_more_than_the_lds_holds_before_any_launch():
    _lib, L = _L()
    M, P, K = 1, 516, 3584                                                     # K + P = 4100
    x, W, b = Buf(shape=(M, K), fill=0.5), Buf(shape=(P, K), fill=0.25), Buf(shape=(P,), fill=0.0)
    tags = torch.full((M,), -1, dtype=torch.int32, device='cuda')
    lg = Buf(shape=(M, P))
    rc = L.ttsc_tag_argmax(x.ptr, W.ptr, b.ptr, None, 0, M, P, K, K, _p(tags), lg.ptr, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'exceeds' in L.ttsc_last_error()
    assert int(tags[0]) == -1 and np.isnan(lg.get()).all()                     # refused in the argument check: nothing ran


# ---- ttsc_dropout_scale --------------------------------------------------------------------------------------------------------------------------------

def _dropout(v, p, keep=None, seed=0, stream_id=0):
    _lib, L = _L()
    xb, y = Buf(v), Buf(shape=v.shape)
    kb = Buf(keep) if keep is not None else None
    _lib.check(L.ttsc_dropout_scale(xb.ptr, v.size, p, kb.ptr if kb else None, seed, stream_id, y.ptr, _lib.current_stream()), 'ttsc_dropout_scale')
    torch.cuda.synchronize()
    assert y.guards_untouched()
    return y.get()


@pytest.mark.parametrize('n', R.DROPOUT_NS)
def test_dropout_scale_injected_philox_p_zero_and_adjoint(n):
    x, keep, dy = R.dropout_case(n)
    seed, stream_id = 0x0123456789abcdef, 3
    host = R.dropout_philox_mask(n, R.DROPOUT_P, seed, stream_id)
    for name, v in (('forward', x), ('adjoint', dy)):
        for path, k, kw in (('injected', keep, dict(keep=keep)), ('philox', host, dict(seed=seed, stream_id=stream_id))):
            got = _dropout(v, R.DROPOUT_P, **kw)
            assert np.array_equal(got.view(np.int32), _dropout(v, R.DROPOUT_P, **kw).view(np.int32))
            assert np.array_equal(got == 0, (k == 0) | (v == 0)), (name, path)                  # (philox: exactly the host-rebuilt mask)
            ref, S = R.dropout_f64(v, k, R.DROPOUT_P)
            _hold('dropout', 'dropout %s %s' % (path, name), got, ref, S)
        for kw in (dict(), dict(keep=np.ones(n, np.float32))):
            assert np.array_equal(_dropout(v, 0.0, **kw).view(np.int32), v.view(np.int32))       # p = 0: the values themselves


def test_zz_report_measured():
    """prints log2 of the worst measured err / S per operation and path"""
    for k in sorted(MEASURED):
        print('MEASURED %-40s 2^%.1f' % (k, R.log2_ratio(MEASURED[k])))
