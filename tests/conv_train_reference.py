"""Plain references for the training convolutions (no GPU): the float64 statement of one generator layer and of its hand-written
vector-Jacobian products, the absolute-value companion S of each, a float32 restatement that adds one term at a time as the yardstick,
and the index maps of the ConvTranspose1d backward stated by brute force.

The layer (hifigan/autograd.py::HipConvFn, csrc/conv_train.hip, csrc/conv_wgrad.hip):

    a = leaky_relu(in_scale * x, in_slope)
    y = conv(a; w) + b (+ resid)              Conv1d (dilated, zero padded, stride 1) or ConvTranspose1d (stride u, padding p)
    dx = in_scale * lrelu'(in_scale * x) * conv^T(dy; w),   dw = sum_{n,t} dy (x) a,   db = sum_{n,t} dy,   dresid = dy

`absolute=True` evaluates the same linear operation on |operands| in float64 (oracle/gan_step_ref.py does this for the discriminator
layers, which have strides, groups and the period fold but no dilation and no in_scale; the convolutions here are written as ONE matrix
product over the stacked taps so that a 10^9-flop reference costs a fraction of a second).  A float32 evaluation's error on an element is a
small multiple of 2^-24 S whatever the cancellation, so the GPU tests bound errors per element by tau * S.

Scalars reach the kernels as C floats: in_scale, in_slope (and out_scale / gate_slope of a bare data-gradient launch, which ARE in_scale /
in_slope of the differentiated layer) are rounded to float32 first, as tests/conv_reference.py does."""
import numpy as np
import torch

from tests.conv_reference import f32

TAU_SPLIT = 2.0 ** -19   # oracle/gan_step_ref.TAU_SPLIT: the same kernels, the same derivation (tests/test_disc_f64_gpu.py)
TAU_EXACT = 2.0 ** -21   # oracle/gan_step_ref.TAU_EXACT
U = 2.0 ** -24


def _t(a, dtype=torch.float64):
    return None if a is None else a.detach().to('cpu', dtype)


def lrelu(x, slope):
    return x if slope == 1.0 else torch.where(x > 0, x, x * slope)


def lrelu_grad(x, slope):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))


def out_len(Lin, K, padding=0, dilation=1, stride=1, transposed=False):
    return (Lin - 1) * stride - 2 * padding + K if transposed else Lin + 2 * padding - dilation * (K - 1)


def _pad(a, left, right):
    N, C, L = a.shape
    out = torch.zeros((N, C, left + L + right), dtype=a.dtype)
    out[:, :, left:left + L] = a
    return out


def _taps(ap, K, step, Lout):
    """[K, N, C, Lout]: tap k is ap[..., k * step : k * step + Lout]"""
    return torch.stack([ap[:, :, k * step:k * step + Lout] for k in range(K)])


def _corr(ap, w, step, Lout):
    """y[n, o, t] = sum_{c, k} w[o, c, k] ap[n, c, t + k step]"""
    return torch.einsum('ock,kncl->nol', w, _taps(ap, w.shape[2], step, Lout))


def _corr_w(ap, dy, K, step):
    """G[o, c, k] = sum_{n, t} dy[n, o, t] ap[n, c, t + k step]"""
    return torch.einsum('nol,kncl->ock', dy, _taps(ap, K, step, dy.shape[2]))


def _upsample(a, u):
    """[N, C, L] -> [N, C, (L - 1) u + 1] with a at every u-th position"""
    N, C, L = a.shape
    out = torch.zeros((N, C, (L - 1) * u + 1), dtype=a.dtype)
    out[:, :, ::u] = a
    return out


def layer(x, w, b=None, resid=None, padding=0, dilation=1, stride=1, transposed=False, in_scale=1.0, in_slope=1.0, dtype=torch.float64,
          absolute=False):
    """x [N, Cin, L] (pre-activation), w in torch layout ([Cout, Cin, K]; transposed: [Cin, Cout, K]) -> y [N, Cout, Lout]"""
    x, w, b, resid = _t(x, dtype), _t(w, dtype), _t(b, dtype), _t(resid, dtype)
    a = lrelu(x * f32(in_scale), f32(in_slope))
    if absolute:
        a, w = a.abs(), w.abs()
        b, resid = (None if b is None else b.abs()), (None if resid is None else resid.abs())
    K = w.shape[2]
    Lo = out_len(x.shape[2], K, padding, dilation, stride, transposed)
    if transposed:
        # y[q] = sum_{i, k} w[ci, co, k] a[i] with q = i u - p + k: the correlation of the zero-stuffed input with the flipped kernel
        au = _pad(_upsample(a, stride), K - 1, K - 1)
        y = _corr(au, w.permute(1, 0, 2).flip(2), 1, (x.shape[2] - 1) * stride + K)[:, :, padding:padding + Lo]
    else:
        y = _corr(_pad(a, padding, padding), w, dilation, Lo)
    if b is not None:
        y = y + b.view(1, -1, 1)
    if resid is not None:
        y = y + resid
    return y


def layer_vjp(x, w, dy, padding=0, dilation=1, stride=1, transposed=False, in_scale=1.0, in_slope=1.0, dtype=torch.float64, absolute=False):
    """-> (dx, dw, db, dresid) of `layer` for the cotangent dy [N, Cout, Lout]"""
    x, w, dy = _t(x, dtype), _t(w, dtype), _t(dy, dtype)
    sc, sl = f32(in_scale), f32(in_slope)
    a, gate = lrelu(x * sc, sl), lrelu_grad(x * sc, sl) * sc
    if absolute:
        a, w, dy = a.abs(), w.abs(), dy.abs()
    N, Cin, L = x.shape
    K = w.shape[2]
    if transposed:
        u, Lo = stride, dy.shape[2]
        full = (L - 1) * u + K
        dyf = torch.zeros((N, w.shape[1], full), dtype=dy.dtype)
        dyf[:, :, padding:padding + Lo] = dy
        # da[ci, i] = sum_{co, k} w[ci, co, k] dyf[co, i u + k];  dw[ci, co, k] = sum_{n, i} a[ci, i] dyf[co, i u + k]
        taps = torch.stack([dyf[:, :, k:k + (L - 1) * u + 1:u] for k in range(K)])      # [K, N, Co, L]
        da = torch.einsum('cok,knol->ncl', w, taps)
        dw = torch.einsum('ncl,knol->cok', a, taps)
    else:
        pd = dilation * (K - 1) - padding
        assert pd >= 0
        da = _corr(_pad(dy, pd, pd), w.permute(1, 0, 2).flip(2), dilation, L)
        dw = _corr_w(_pad(a, padding, padding), dy, K, dilation)
    return da * gate, dw, dy.sum(dim=(0, 2)), dy


def wgrad(P, Q, J, base, step, q_scale=1.0, q_slope=1.0, dtype=torch.float64, absolute=False):
    """the contract of ttsc_conv_wgrad(_split): G[a, b, j] = sum_{n, t} P[n, a, t] lrelu(q_scale Q[n, b, t + base + j step], q_slope), Q zero outside"""
    P, Q = _t(P, dtype), _t(Q, dtype)
    A = lrelu(Q * f32(q_scale), f32(q_slope))
    if absolute:
        P, A = P.abs(), A.abs()
    LP, LQ = P.shape[2], Q.shape[2]
    offs = [base + j * step for j in range(J)]
    left = max(0, -min(offs))
    right = max(0, LP + max(offs) - LQ)
    Ap = _pad(A, left, right)
    taps = torch.stack([Ap[:, :, left + o:left + o + LP] for o in offs])              # [J, N, Bc, LP]
    return torch.einsum('nat,jnbt->abj', P, taps)


# ---- the bare launches of ttsc_conv_train, in the kernel's own terms ----------------------------------------------------------------------
def launch_fwd(x, w, b, resid, padding, dilation, in_scale, in_slope, absolute=False):
    return layer(x, w, b, resid, padding, dilation, in_scale=in_scale, in_slope=in_slope, absolute=absolute)


def launch_dgrad(dy, w, gate, padding, dilation, out_scale, gate_slope, absolute=False):
    """flip = 1: dy [B, Cin_k, Lin], w [Cin_k, Cout_k, K] = the forward weight of the differentiated layer, gate [B, Cout_k, Lout] its saved
    pre-activation: y = conv(dy; W) * (gate > 0 ? 1 : gate_slope) * out_scale with W[co, ci, k] = w[ci, co, K - 1 - k]"""
    dy, w, gate = _t(dy), _t(w), _t(gate)
    W = w.permute(1, 0, 2).flip(2)
    if absolute:
        dy, W = dy.abs(), W.abs()
    K = W.shape[2]
    y = _corr(_pad(dy, padding, padding), W, dilation, out_len(dy.shape[2], K, padding, dilation))
    return y * lrelu_grad(gate, f32(gate_slope)) * f32(out_scale)


# ---- the float32 yardstick: one term at a time, every product and every sum rounded on its own -----------------------------------------
def _seq_corr32(ap, w, step, Lout, init=None):
    N = ap.shape[0]
    O, Cc, K = w.shape
    acc = torch.zeros((N, O, Lout), dtype=torch.float32) if init is None else init.clone()
    for c in range(Cc):
        for k in range(K):
            acc += w[:, c, k].view(1, O, 1) * ap[:, c:c + 1, k * step:k * step + Lout]
    return acc


def launch_fwd_f32(x, w, b, resid, padding, dilation, in_scale, in_slope):
    x, w = _t(x, torch.float32), _t(w, torch.float32)
    a = lrelu(x * np.float32(in_scale), float(np.float32(in_slope)))
    y = _seq_corr32(_pad(a, padding, padding), w, dilation, out_len(x.shape[2], w.shape[2], padding, dilation))
    if b is not None:
        y = y + _t(b, torch.float32).view(1, -1, 1)
    if resid is not None:
        y = y + _t(resid, torch.float32)
    return y


def launch_dgrad_f32(dy, w, gate, padding, dilation, out_scale, gate_slope):
    dy, w, gate = _t(dy, torch.float32), _t(w, torch.float32), _t(gate, torch.float32)
    W = w.permute(1, 0, 2).flip(2).contiguous()
    y = _seq_corr32(_pad(dy, padding, padding), W, dilation, out_len(dy.shape[2], W.shape[2], padding, dilation))
    return (y * lrelu_grad(gate, float(np.float32(gate_slope)))) * np.float32(out_scale)


def wgrad_f32(P, Q, J, base, step, q_scale=1.0, q_slope=1.0, block=1):
    """float32, one position at a time (block = 1: strictly sequential over all N * LP terms of an element; block = 64: the sums of 64-position
    chunks added in order, the shape of the tile kernels' summation)"""
    P, Q = _t(P, torch.float32), _t(Q, torch.float32)
    A = lrelu(Q * np.float32(q_scale), float(np.float32(q_slope)))
    N, Aa, LP = P.shape
    LQ = Q.shape[2]
    offs = [base + j * step for j in range(J)]
    left = max(0, -min(offs))
    right = max(0, LP + max(offs) - LQ)
    Ap = _pad(A, left, right)
    G = torch.zeros((Aa, Q.shape[1], J), dtype=torch.float32)
    for n in range(N):
        for t0 in range(0, LP, block):
            t1 = min(t0 + block, LP)
            for j, o in enumerate(offs):
                if block == 1:
                    G[:, :, j] += P[n, :, t0].view(-1, 1) * Ap[n, :, left + o + t0].view(1, -1)
                else:
                    part = torch.zeros((Aa, Q.shape[1]), dtype=torch.float32)
                    for t in range(t0, t1):
                        part += P[n, :, t].view(-1, 1) * Ap[n, :, left + o + t].view(1, -1)
                    G[:, :, j] += part
    return G


def layer_f32(x, w, b=None, resid=None, padding=0, dilation=1, stride=1, transposed=False, in_scale=1.0, in_slope=1.0):
    """`layer` in float32, one (input channel, tap) term at a time"""
    if not transposed:
        return launch_fwd_f32(x, w, b, resid, padding, dilation, in_scale, in_slope)
    x, w = _t(x, torch.float32), _t(w, torch.float32)
    a = lrelu(x * np.float32(in_scale), float(np.float32(in_slope)))
    N, Ci, L = a.shape
    Co, K, u = w.shape[1], w.shape[2], stride
    full = torch.zeros((N, Co, (L - 1) * u + K), dtype=torch.float32)
    for ci in range(Ci):
        for k in range(K):
            full[:, :, k:k + (L - 1) * u + 1:u] += w[ci, :, k].view(1, Co, 1) * a[:, ci:ci + 1, :]
    y = full[:, :, padding:padding + out_len(L, K, padding, 1, u, True)]
    if b is not None:
        y = y + _t(b, torch.float32).view(1, -1, 1)
    if resid is not None:
        y = y + _t(resid, torch.float32)
    return y


def layer_vjp_f32(x, w, dy, padding=0, dilation=1, stride=1, transposed=False, in_scale=1.0, in_slope=1.0):
    """(dx, dw) of `layer` in float32: dx one (output channel, tap) term at a time, dw one position at a time"""
    if not transposed:
        K = w.shape[2]
        return (launch_dgrad_f32(dy, w, x, dilation * (K - 1) - padding, dilation, in_scale, in_slope),
                wgrad_f32(dy, x, K, -padding, dilation, in_scale, in_slope))
    x, w, dy = _t(x, torch.float32), _t(w, torch.float32), _t(dy, torch.float32)
    sc, sl = np.float32(in_scale), float(np.float32(in_slope))
    a = lrelu(x * sc, sl)
    N, Ci, L = x.shape
    Co, K, u = w.shape[1], w.shape[2], stride
    dyf = torch.zeros((N, Co, (L - 1) * u + K), dtype=torch.float32)
    dyf[:, :, padding:padding + dy.shape[2]] = dy
    da = torch.zeros((N, Ci, L), dtype=torch.float32)
    for co in range(Co):
        for k in range(K):
            da += w[:, co, k].view(1, Ci, 1) * dyf[:, co:co + 1, k:k + (L - 1) * u + 1:u]
    dw = torch.zeros((Ci, Co, K), dtype=torch.float32)
    for n in range(N):
        for i in range(L):
            dw += a[n, :, i].view(Ci, 1, 1) * dyf[n, :, i * u:i * u + K].view(1, Co, K)
    return (da * lrelu_grad(x * sc, sl)) * sc, dw


# ---- ConvTranspose1d backward: the index maps of TrainConv, stated by brute force --------------------------------------------------------
def bare_train_conv(Cin, Cout, K, stride, padding):
    """a TrainConv with the fields its index maps read, built without the library (TrainConv.__init__ creates kernel handles)"""
    from ttscube_amd.hifigan.autograd import TrainConv
    tc = TrainConv.__new__(TrainConv)
    tc.Cin, tc.Cout, tc.K = Cin, Cout, K
    tc.stride, tc.padding, tc.dilation, tc.transposed, tc.groups = stride, padding, 1, True, 1
    tc._dgrad = tc._maps = None
    tc._bg_ws = {}
    return tc


def transposed_backward_by_maps(tc, x, w, dy):
    """the route HipConvFn.backward takes for a ConvTranspose1d, in float64 and without kernels: de-interleave dy, gather the weights through
    w_map, dense stride-1 data gradient over the u Cout rows; G[r Co + co, ci, j] = sum_i x[ci, i] dyP[r Co + co, i + j] (the call
    _wgrad(dyP, x, ..., base = 0, step = -1)) gathered through g_map -> (dx, dw), in_scale = in_slope = 1"""
    m_lo, _, M = tc.taps_t()
    Lin = x.shape[2]
    dyp = tc.deinterleave(dy, Lin)
    w_map, g_map = tc.maps_t(torch.device('cpu'))
    wz = torch.cat([w.reshape(-1), w.new_zeros(1)])
    wd = wz[w_map]                                   # [Ci, u Co, M]
    dx = _corr(dyp, wd, 1, Lin)                      # dense stride-1 convolution, padding 0: [N, Ci, Lin]
    G = wgrad(dyp, x, M, 0, -1)                      # [u Co, Ci, M]
    return dx, G.reshape(-1)[g_map]
