"""Plain references for the inference convolutions (no GPU): a float64 statement of every operation the kernels fuse, a float32
restatement that accumulates one (input channel, tap) term at a time as the yardstick, the magnitude budget of the derived error bound,
and inputs on which the right answer has no rounding at all.

The operation (Conv1dHip.__call__ / ttsc_conv1d_forward):

    x' = leaky_relu(x * in_scale, in_slope)
    y  = act((conv(x', w) + b + resid) * out_scale)  [+ acc0 when accumulate]

Scalars reach the kernels as C floats, so the references round in_scale, in_slope and out_scale to float32 first: the float64 reference is
the high-precision value of the operation the kernel was asked for, not of a neighbouring one.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

CHAIN_SLOPE = 0.1   # the ResBlock chain kernels hard-code leaky_relu(., 0.1f)
U = 2.0 ** -24      # unit roundoff of float32


def f32(v):
    return float(np.float32(v))


def out_len(Lin, k, stride=1, padding=0, dilation=1, transposed=False):
    if transposed:
        return (Lin - 1) * stride - 2 * padding + k
    return Lin + 2 * padding - dilation * (k - 1)


def prologue_f64(x, in_scale=1.0, in_slope=1.0):
    return F.leaky_relu(x.double() * f32(in_scale), f32(in_slope))


def _act(t, act):
    if act is None:
        return t
    if act == 'tanh':
        return torch.tanh(t)
    raise ValueError(act)


def conv_f64(x, w, b=None, stride=1, padding=0, dilation=1, transposed=False, in_scale=1.0, in_slope=1.0, resid=None, acc0=None,
             out_scale=1.0, act=None):
    """float64 torch on the CPU; x [B, Cin, L], w in torch layout ([Cout, Cin, K], transposed: [Cin, Cout, K])"""
    xp = prologue_f64(x, in_scale, in_slope)
    wd = w.double()
    bd = b.double() if b is not None else None
    if transposed:
        t = F.conv_transpose1d(xp, wd, bd, stride=stride, padding=padding)
    else:
        t = F.conv1d(xp, wd, bd, padding=padding, dilation=dilation)
    if resid is not None:
        t = t + resid.double()
    t = _act(t * f32(out_scale), act)
    if acc0 is not None:
        t = t + acc0.double()
    return t


def conv_f64_ragged(x, lengths, w, b=None, **kw):
    """every utterance computed alone at its own length: a list of [1, Cout, Lout_b]"""
    return [conv_f64(x[i:i + 1, :, :n], w, b, **kw) for i, n in enumerate(lengths)]


def chain_f64(x, layers, k, post=None, post_kw=None, ysum=None, dtype=torch.float64):
    """ResBlock1 chain x <- x + conv2(lrelu(conv1_d(lrelu(x)))) per (w1, b1, w2, b2, d); optional conv_post (w, b) with its epilogue.
    Also returns every activation that enters a convolution (for the exactness conditions)."""
    s = f32(CHAIN_SLOPE)
    x = x.to(dtype)
    entering = []
    for w1, b1, w2, b2, d in layers:
        a1 = F.leaky_relu(x, s)
        xt = F.conv1d(a1, w1.to(dtype), b1.to(dtype), padding=d * (k - 1) // 2, dilation=d)
        a2 = F.leaky_relu(xt, s)
        x = x + F.conv1d(a2, w2.to(dtype), b2.to(dtype), padding=(k - 1) // 2)
        entering += [a1, a2]
    if ysum is not None:
        x = x + ysum.to(dtype)
    if post is not None:
        kw = dict(post_kw or {})
        pw, pb = post
        return conv_f64(x, pw, pb, padding=(pw.shape[-1] - 1) // 2, **kw), entering
    return x, entering


def chain_f64_ragged(x, lengths, layers, k):
    return [chain_f64(x[i:i + 1, :, :n], layers, k)[0] for i, n in enumerate(lengths)]


# ---- the float32 yardstick ---------------------------------------------------------------------------------------------------------------------

def _lrelu32(x, slope):
    return np.where(x >= 0, x, (x * np.float32(slope)).astype(np.float32)).astype(np.float32)


def _conv_core_f32(xp, w, stride, padding, dilation, transposed, reverse, init=None):
    """sum over (input channel, tap) of w * x', ONE term at a time: product rounded, then the sum rounded (numpy has no FMA and no blocked
    summation for an elementwise multiply followed by an elementwise add)"""
    B, Cin, L = xp.shape
    K = w.shape[-1]
    Lout = out_len(L, K, stride, padding, dilation, transposed)
    terms = [(ci, k) for ci in range(Cin) for k in range(K)]
    if reverse:
        terms.reverse()
    if transposed:
        Cout = w.shape[1]
        full = np.zeros((B, Cout, (L - 1) * stride + K), np.float32)
        span = (L - 1) * stride + 1
        for ci, k in terms:
            v = full[:, :, k:k + span:stride]
            v += w[ci, :, k][None, :, None] * xp[:, ci, None, :]
        return np.ascontiguousarray(full[:, :, padding:padding + Lout])
    Cout = w.shape[0]
    buf = np.zeros((B, Cin, L + 2 * padding), np.float32)
    buf[:, :, padding:padding + L] = xp
    acc = np.zeros((B, Cout, Lout), np.float32) if init is None else init.astype(np.float32).copy()
    for ci, k in terms:
        acc += w[:, ci, k][None, :, None] * buf[:, ci, None, k * dilation:k * dilation + Lout]
    return acc


def _np32(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


def conv_f32_sequential(x, w, b=None, stride=1, padding=0, dilation=1, transposed=False, in_scale=1.0, in_slope=1.0, resid=None, acc0=None,
                        out_scale=1.0, act=None, reverse=False, init_first=False):
    """the same formula in numpy float32, every operation rounded on its own; returns a float32 torch tensor.
    init_first: the sum STARTS at (resid + acc0) + b and the terms are added onto it, the order of the layers whose kernels take the epilogue
    operands as the accumulators' initial value (square 128 / 256-channel ResBlock layers; plain affine epilogue only)"""
    xn, wn, bn, rn, an = _np32(x), _np32(w), _np32(b), _np32(resid), _np32(acc0)
    xp = _lrelu32((xn * np.float32(in_scale)).astype(np.float32), in_slope)
    if init_first:
        assert not transposed and act is None and out_scale == 1.0
        Lo = out_len(xn.shape[2], wn.shape[2], stride, padding, dilation, transposed)
        init = np.zeros((xn.shape[0], wn.shape[0], Lo), np.float32)
        if rn is not None:
            init = init + rn
        if an is not None:
            init = init + an
        if bn is not None:
            init = init + bn[None, :, None]
        t = _conv_core_f32(xp, wn, stride, padding, dilation, transposed, reverse, init=init)
        return torch.from_numpy(np.ascontiguousarray(t.astype(np.float32)))
    t = _conv_core_f32(xp, wn, stride, padding, dilation, transposed, reverse)
    if bn is not None:
        t = t + bn[None, :, None]
    if rn is not None:
        t = t + rn
    t = (t * np.float32(out_scale)).astype(np.float32)
    if act == 'tanh':
        t = np.tanh(t.astype(np.float64)).astype(np.float32)   # correctly rounded: the yardstick charges nothing for the transcendental
    elif act is not None:
        raise ValueError(act)
    if an is not None:
        t = t + an
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.float32)))


def chain_f32_sequential(x, layers, k, post=None, post_kw=None, ysum=None, reverse=False):
    s = CHAIN_SLOPE
    x = x.float()
    for w1, b1, w2, b2, d in layers:
        xt = conv_f32_sequential(x, w1, b1, padding=d * (k - 1) // 2, dilation=d, in_slope=s, reverse=reverse)
        x = conv_f32_sequential(xt, w2, b2, padding=(k - 1) // 2, in_slope=s, resid=x, reverse=reverse)
    if ysum is not None:
        x = x + ysum.float()
    if post is not None:
        pw, pb = post
        return conv_f32_sequential(x, pw, pb, padding=(pw.shape[-1] - 1) // 2, reverse=reverse, **dict(post_kw or {}))
    return x


# ---- the derived bound -------------------------------------------------------------------------------------------------------------------------

def abs_budget(x, w, b=None, stride=1, padding=0, dilation=1, transposed=False, in_scale=1.0, in_slope=1.0, resid=None, acc0=None):
    """A = conv_f64(|x'|, |w|, |b|) + |resid| + |acc0| (x' = the prologue's output) and W = the sum of |w| over each output's receptive field
    (position-dependent at the edges and across the phases of a transposed layer)"""
    xp = prologue_f64(x, in_scale, in_slope).abs()
    kw = dict(stride=stride, padding=padding, dilation=dilation, transposed=transposed)
    A = conv_f64(xp, w.abs(), b.abs() if b is not None else None, **kw)
    if resid is not None:
        A = A + resid.double().abs()
    if acc0 is not None:
        A = A + acc0.double().abs()
    W = conv_f64(torch.ones_like(xp), w.abs(), None, **kw)
    return A, W


def n_terms(cin, k, stride=1, transposed=False, bias=True, resid=False, acc0=False):
    n = cin * (-(-k // stride) if transposed else k)
    return n + int(bias) + int(resid) + int(acc0)


def derived_bound(n, A, W, out_scale=1.0):
    """|y - ref64| <= (n + 16) * 2^-24 * A + 2^-24 * W, element-wise ('inference convolutions against float64')"""
    return ((n + 16) * U * A + U * W) * abs(f32(out_scale))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------

def _mk(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def random_case(cin, cout, k, L, B=2, stride=1, dilation=1, transposed=False, resid=False, acc0=False, seed=0):
    """N(0,1) activations, weights N(0, 1 / fan-in), bias N(0, 0.01): what the existing kernel tests use"""
    if transposed:
        padding = (k - stride) // 2
        w = _mk((cin, cout, k), seed + 1, 1.0 / (cin * k / stride) ** 0.5)
    else:
        padding = dilation * (k - 1) // 2
        w = _mk((cout, cin, k), seed + 1, 1.0 / (cin * k) ** 0.5)
    Lo = out_len(L, k, stride, padding, dilation, transposed)
    c = dict(x=_mk((B, cin, L), seed + 3), w=w, b=_mk((cout,), seed + 2, 0.1),
             kw=dict(stride=stride, padding=padding, dilation=dilation, transposed=transposed))
    c['resid'] = _mk((B, cout, Lo), seed + 4) if resid else None
    c['acc0'] = _mk((B, cout, Lo), seed + 5) if acc0 else None
    return c


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_case(cin, cout, k, L, B=2, stride=1, dilation=1, transposed=False, resid=False, acc0=False, in_scale=1.0, in_slope=0.5, seed=0):
    """Single layer on which nothing rounds: weights m / 8 with integer |m| <= 8 (fp16 holds them after any power-of-two pre-scale: hi exact,
    lo = 0), integer activations in [-8, 8] (signed: the leaky-relu slope of 0.25 or 0.5 is exercised and stays exact), integer bias, residual
    and running sum, a power-of-two in_scale.  Every partial sum is a multiple of 2^-6 below 2^16."""
    assert in_slope in (0.25, 0.5) and np.log2(in_scale) == int(np.log2(in_scale))
    if transposed:
        padding = (k - stride) // 2
        w = _ints((cin, cout, k), -8, 8, seed + 1) / 8.0
    else:
        padding = dilation * (k - 1) // 2
        w = _ints((cout, cin, k), -8, 8, seed + 1) / 8.0
    Lo = out_len(L, k, stride, padding, dilation, transposed)
    c = dict(x=_ints((B, cin, L), -8, 8, seed + 3), w=w, b=_ints((cout,), -5, 5, seed + 2),
             kw=dict(stride=stride, padding=padding, dilation=dilation, transposed=transposed, in_scale=in_scale, in_slope=in_slope))
    c['resid'] = _ints((B, cout, Lo), -9, 9, seed + 4) if resid else None
    c['acc0'] = _ints((B, cout, Lo), -9, 9, seed + 5) if acc0 else None
    return c


def exact_chain_case(C, k, dils, L, B=2, seed=0):
    """ResBlock1 chain on which nothing rounds.  The chain kernels hard-code the slope 0.1, which is not a float16 number, so the data stay
    non-negative (leaky-relu is then the identity): activations are integers in [0, 7], biases integers in [0, 3], and every weight row holds
    three non-negative entries 1/4, 1/8, 1/8 (row sum 1/2: values do not grow through the six convolutions, and every value stays a multiple
    of 2^-18 below 2^6).  Row co puts its entries at taps (3 co + j) mod K and input chunks (co + j) mod (C / 16), j = 0..2, so that every tap
    and every 16-channel input chunk is used inside every 32-row tile; the channel inside the chunk and the positions vary pseudo-randomly."""
    g = torch.Generator().manual_seed(seed)
    nch = C // 16

    def sparse_w():
        w = torch.zeros(C, C, k)
        for co in range(C):
            for j, v in enumerate((0.25, 0.125, 0.125)):
                ci = ((co + j) % nch) * 16 + int(torch.randint(0, 16, (1,), generator=g))
                w[co, ci, (3 * co + j) % k] += v
        return w

    layers = []
    for d in dils:
        layers.append((sparse_w(), torch.randint(0, 4, (C,), generator=g).float(), sparse_w(), torch.randint(0, 4, (C,), generator=g).float(), d))
    x = torch.randint(0, 8, (B, C, L), generator=g).float()
    acc0 = torch.randint(0, 8, (B, C, L), generator=g).float()
    return dict(x=x, layers=layers, acc0=acc0)


def random_chain_layers(C, k, dils, seed=0):
    layers = []
    for m, d in enumerate(dils):
        layers.append((_mk((C, C, k), seed + 10 * m + 1, 1.0 / (C * k) ** 0.5), _mk((C,), seed + 10 * m + 2, 0.1),
                       _mk((C, C, k), seed + 10 * m + 3, 1.0 / (C * k) ** 0.5), _mk((C,), seed + 10 * m + 4, 0.1), d))
    return layers


def is_split_exact(v):
    """v == float16(v) + float16(v - float16(v)) and |v| < 65504: the two fp16 halves of the split path carry v without loss"""
    v = v.double()
    hi = v.to(torch.float16).double()
    lo = (v - hi).to(torch.float16).double()
    return bool(((hi + lo) == v).all()) and bool((v.abs() < 65504).all())


# ---- cached evaluation (the yardstick costs about a second at 256 channels with k = 11) ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cached_random(cin, cout, k, L, B=2, stride=1, dilation=1, transposed=False, resid=False, acc0=False, in_scale=1.0, in_slope=1.0,
                  out_scale=1.0, act=None, seed=0, init_first=False):
    """(case, ref64, yardstick32, A, W) of one random single-layer case; shared by the tests, never modified"""
    c = random_case(cin, cout, k, L, B, stride, dilation, transposed, resid, acc0, seed)
    kw = dict(c['kw'], in_scale=in_scale, in_slope=in_slope)
    ref = conv_f64(c['x'], c['w'], c['b'], resid=c['resid'], acc0=c['acc0'], out_scale=out_scale, act=act, **kw)
    yard = conv_f32_sequential(c['x'], c['w'], c['b'], resid=c['resid'], acc0=c['acc0'], out_scale=out_scale, act=act, init_first=init_first, **kw)
    A, W = abs_budget(c['x'], c['w'], c['b'], resid=c['resid'], acc0=c['acc0'], **kw)
    c = dict(c, kw=kw, out_scale=out_scale, act=act)
    return c, ref, yard, A, W


def err_stats(y, ref):
    e = (y.double() - ref).abs()
    return float(e.max()), float((e * e).mean().sqrt())


# ---- the variants and their shapes (shared by the CPU check of the exactness conditions and the GPU tests) --------------------------------------

def mt_class(cout, stride=1, transposed=False):
    """the row-tile class ttsc_conv1d_create picks: the largest of 32 / 64 / 128 that does not pad the (virtual) rows further than 32 does.  A
    transposed layer with a multiple of 32 output channels runs all its phases as stride * Cout virtual rows."""
    rows = stride * cout if (transposed and cout % 32 == 0 and stride > 1) else cout
    best, best_pad = 32, -(-rows // 32) * 32
    for mt in (64, 128):
        pad = -(-rows // mt) * mt
        if pad <= best_pad:
            best, best_pad = mt, pad
    return best


def tiles_of(prec, mt):
    """(rows, cols) of every tile the fill rule can pick for a layer of this class"""
    if prec == 'f16x3':
        return [(64, 256), (64, 128), (32, 128)] if mt >= 64 else [(32, 512), (32, 256), (32, 128)]
    return {128: [(128, 128), (64, 128), (64, 64)], 64: [(64, 256), (64, 128), (64, 64)], 32: [(32, 512), (32, 256), (32, 128)]}[mt]


# ---- the dispatch, restated (csrc/conv_plan.hpp; tests/test_conv_plan_cpu.py compares this with ttsc_conv1d_plan) --------------------------------

PATH_NONE, PATH_COUT1, PATH_TALL, PATH_WIDE, PATH_F16X3, PATH_FP32 = range(6)   # TTSC_CONV_PATH_*
INT_MAX = 2 ** 31 - 1
FP32_NARROWER = {512: 256, 256: 128, 128: 64}   # the column count the fp32 fill rule weighs a tile's padding against


class PlanError(ValueError):
    pass


def _cdiv(a, b):
    return -(-a // b)


def pipe_lds(span, mi):
    """dynamic LDS of the wide / tall tile pipeline: two activation buffers of 4 planes + a dump slot pair, two weight slots, 16-byte items"""
    return 2 * (4 * span + 2) * 16 + 2 * (2 * mi * 2 * 64) * 16


def plan(cin, cout, k, B, Lin, prec='f16x3', stride=1, padding=0, dilation=1, transposed=False, groups=1, phase=0, gate=False, act=None,
         out_scale=1.0, in_scale=1.0, wide=1, lean=True, tile=None):
    """what ttsc_conv1d_forward launches for one phase of a layer: dict(family, rows, cols, tap_bucket, grid, lds, lean, acc_init, short_from).
    wide / lean / tile are TTSC_CONV_WIDE / TTSC_CONV_LEAN / TTSC_CONV_TILE (tile: the variable's text or None); the once-per-process
    switches are at their defaults.  Raises PlanError where the launch is refused."""
    vfused = transposed and cout % 32 == 0 and stride > 1
    if groups > 1:
        cout_g, cin_g = cout // groups, cin // groups
        mt = 128 if cout_g % 128 == 0 else (64 if cout_g % 64 == 0 else 32)
        cin_tile = (mt // cout_g if mt > cout_g else 1) * cin_g
    else:
        mt, cin_tile = mt_class(cout, stride, transposed), cin
    rows_v = stride * cout if vfused else cout
    coutp, cinp = _cdiv(rows_v, mt) * mt, _cdiv(cin_tile, 16) * 16
    # ttsc_conv1d_set_precision: the split kernel's register window holds 64 positions of halo and 16 taps; grouped layers are fp32 only
    J = _cdiv(k, stride)
    if prec == 'f16x3' and ((J - 1 if transposed else (k - 1) * dilation) > 64 or (J if transposed else k) > 16 or groups > 1):
        prec = 'fp32'
    f16 = prec == 'f16x3'
    vrow4 = vfused and f16 and stride == 4 and k == 4 and padding == 0
    Lout = out_len(Lin, k, stride, padding, dilation, transposed)
    # the phase: taps and positions q with o = q * stride + r - padding inside [0, Lout)
    if not transposed:
        ntaps, halo, q_cnt = k, (k - 1) * dilation, Lout
    else:
        r_lo, r_hi = (stride - 1, 0) if vfused else (phase, phase)
        ntaps = J if vfused else len(range(phase, k, stride))
        qlo, qhi = -((r_lo - padding) // stride), (Lout - 1 - r_hi + padding) // stride + 1
        if qhi <= qlo:
            return dict(family=PATH_NONE, rows=0, cols=0, tap_bucket=0, grid=(0, 0, 0), lds=0, lean=0, acc_init=0, short_from=INT_MAX)
        halo, q_cnt = ntaps - 1, qhi - qlo
    forced = None
    if tile:
        parts = tile.lower().split('x')
        if len(parts) != 2 or not all(s.isdigit() and int(s) > 0 for s in parts):
            raise PlanError('malformed TTSC_CONV_TILE')
        forced = (int(parts[0]), int(parts[1]))
    p = dict(tap_bucket=0, lean=0, acc_init=0, short_from=INT_MAX)
    if not transposed and groups == 1 and cout == 1 and cin <= 64 and k <= 16 and dilation == 1 and not gate:
        return dict(p, family=PATH_COUT1, rows=1, cols=1024, grid=(_cdiv(Lout, 1024), B, 1), lds=0)
    tiles = tiles_of(prec, mt)
    if f16:
        if ntaps > 16:
            raise PlanError('more than 16 taps')
        affine = act is None and f32(out_scale) == 1.0
        small = B * cout * Lout < 2 ** 32
        wide_shape = (not transposed and not gate and cin == cout and cout in (128, 256) and k in (3, 7, 11) and dilation in (1, 3, 5)
                      and padding == dilation * (k - 1) // 2)
        p['acc_init'] = int(bool(wide and wide_shape and affine and coutp == cout and small))
        tall0 = cin == 512 and ntaps == 4 and coutp % 256 == 0
        tall1 = cin == 256 and ntaps == 6 and coutp % 128 == 0
        tall_shape = vfused and not vrow4 and not gate and cinp == cin and (tall0 or tall1)
        trows, tcols = (256, 128) if tall0 else (128, 256)
        s = f32(in_scale)
        p['lean'] = int(bool(lean and cin * Lin * 4 < 2 ** 31 and s > 0 and np.isfinite(s)))
        if tall_shape and trows == cout:
            p['short_from'] = k - (ntaps - 1) * stride
        if tall_shape and (wide == 2 or _cdiv(q_cnt, tcols) * (coutp // trows) * B >= 512):
            nx, ny = _cdiv(q_cnt, tcols), coutp // trows
            grid = (_cdiv(nx * B, 8) * 8 * ny, 1, 1) if ny > 1 else (nx, ny, B)   # (XCD-aware 1-D launch)
            return dict(p, family=PATH_TALL, rows=trows, cols=tcols, grid=grid, lds=pipe_lds(tcols + ntaps - 1, trows // 64))
        if wide and wide_shape and (wide == 2 or _cdiv(Lout, 256) * (cout // 128) * B >= 512):
            return dict(p, family=PATH_WIDE, rows=128, cols=256, grid=(_cdiv(Lout, 256), cout // 128, B), lds=pipe_lds(256 + halo, 2))
        p['tap_bucket'] = next(t for t in (3, 7, 11, 16) if ntaps <= t)

    def wgs(t):
        return _cdiv(q_cnt, t[1]) * (coutp // t[0]) * B

    def fills(t):
        if f16:
            return wgs(t) >= 512
        padded = lambda n: _cdiv(q_cnt, n) * n
        return wgs(t) >= 512 and not padded(FP32_NARROWER[t[1]]) * 8 < padded(t[1]) * 7

    if forced:
        if forced not in tiles:
            raise PlanError('not a tile of this layer')
        t = forced
    else:
        t = next((u for u in tiles[:2] if fills(u)), tiles[2])
    span = t[1] + halo
    lds = span * 4 * 16 + ntaps * (t[0] // 32) * 2 * 64 * 16 if f16 else 2 * 16 * (span + 1) * 4
    if not f16 and lds > 160 * 1024:
        raise PlanError('receptive field too large for LDS')
    return dict(p, family=PATH_F16X3 if f16 else PATH_FP32, rows=t[0], cols=t[1], grid=(_cdiv(q_cnt, t[1]), coutp // t[0], B), lds=lds)


def tile_lengths(nt):
    """the lengths at which a tile of nt columns can go wrong: one column either side of a seam, more than one block, and one position (shorter
    than every receptive field here)"""
    return [nt - 1, nt, nt + 1, 2 * nt + 1, 1]


# (cin, cout, k, dilation): conv_pre-like; Cin and Cout padded to the chunk / tile; a dilated 32-channel layer; a 64-row-class layer (the fp32
# 64 x 256 tile); 512 -> 80 runs 32-row tiles with 16 padded rows (80 is a 32-row class: 96 < 128), 512 -> 100 the 128-row tile with 28
GENERAL_CONV = [(80, 128, 7, 1), (20, 24, 3, 1), (32, 32, 11, 5), (64, 64, 7, 3), (512, 80, 5, 1), (512, 100, 5, 1)]
# (cin, cout, k, stride): the two k4 s4 layers store interleaved rows on the split path; two layers that run phase by phase
GENERAL_TRANS = [(128, 64, 4, 4), (64, 32, 4, 4), (32, 16, 16, 8), (16, 8, 3, 2)]


def general_lengths(cin, nt, transposed):
    if cin >= 512:
        return [nt - 1, nt + 1, 1]
    # transposed: the per-phase position count is Lin (k4 s4) or Lin + 1 for some phases of the layers that run phase by phase
    return ([nt - 2] if transposed else []) + tile_lengths(nt)


def general_variants(prec):
    """[(layer, transposed, (rows, cols), lengths)] for every tile of every general-kernel layer"""
    out = []
    for layer in GENERAL_CONV:
        for t in tiles_of(prec, mt_class(layer[1])):
            out.append((layer, False, t, general_lengths(layer[0], t[1], False)))
    for layer in GENERAL_TRANS:
        for t in tiles_of(prec, mt_class(layer[1], layer[3], True)):
            out.append((layer, True, t, general_lengths(layer[0], t[1], True)))
    return out


def general_exact(layer, transposed, L, seed=0):
    cin, cout, k, ds = layer
    kw = dict(stride=ds, transposed=True) if transposed else dict(dilation=ds)
    return exact_case(cin, cout, k, L, resid=True, acc0=True, in_scale=0.5, in_slope=0.25, seed=seed, **kw)


# wide kernel: every K and every d at 257, the other lengths on a diagonal of (K, d); 5 positions are shorter than the receptive field
WIDE_CASES = [(C, k, d, L) for C in (128, 256) for k, d, Ls in ((3, 1, (255, 257)), (3, 5, (257,)), (7, 3, (5, 256, 257)), (7, 1, (257,)),
                                                                 (11, 5, (257, 513)), (11, 1, (257,))) for L in Ls]
# tall kernel: (cin, cout, k, stride, Lin); 2 input positions are fewer than the 4 / 6 taps per phase
TALL_CASES = [(512, 256, 16, 5, L) for L in (2, 127, 128, 129)] + [(256, 128, 16, 3, L) for L in (2, 255, 256, 257)]
COUT1_CASES = [(cin, L) for cin in (32, 20) for L in (3, 1023, 1024, 1025)]
CHAIN_CONFIGS = [(32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (64, 11), (128, 3)]
CHAIN_DILS = (1, 3, 5)


def chain_geometry(C, k, dils=CHAIN_DILS, interleaved=True):
    """(large, ncol, halo, nto) of the tile ttsc_rbchain_forward picks by itself (shape = -1) for a small batch: halo = sum (d + 1)(K - 1) / 2 columns
    per side, the large tile once the halo would eat more than a sixth of the small one, nto = ncol - 2 halo output columns, rounded down to a
    multiple of 32 for interleaved tiles above 256.  The K = 7 block at 32 channels keeps the plain small tile."""
    halo = sum((d + 1) * (k - 1) // 2 for d in dils)
    small = 512 if C == 32 else 256
    large = 2 * halo * 6 > small
    ncol = small * (2 if (large and C != 128) else 1)
    il = interleaved and all(d in (1, 3, 5) for d in dils) and not (C == 32 and k == 7 and not large)
    nto = ncol - 2 * halo
    if il and nto > 256:
        nto &= ~31
    return large, ncol, halo, nto, il


def chain_lengths(nto):
    """one column either side of the seam, two tiles and one column (odd: the interleaved kernels' column-wise fallback), and a multiple of 4
    just above the seam (their vector path)"""
    return [nto - 1, nto, nto + 1, 2 * nto + 1, (nto + 4) // 4 * 4, 7]   # (7: shorter than every chain's receptive field)
