"""ORACLE (test infrastructure — never imported by the product path): the Cubegan step's 45 x mel-L1 half and discriminator half restated
as plain torch ops on the CPU, with hand-written vector-Jacobian products, for tests only.

  conv_layer / conv_layer_vjp   one discriminator layer: y = Conv1d(leaky_relu(x, in_slope); w, b) with stride, padding, groups and MPD's
                                period fold (`period` P > 1: x is the flat [N, C, H * P] signal, the convolution runs over h with the P
                                columns apart — Conv2d((K, 1), (s, 1)) of hifigan's DiscriminatorP); a sum over taps of strided slices
  weight_norm(_vjp)             w = g v / ||v|| per output row
  spectral_norm(_vjp)           torch.nn.utils.spectral_norm, dim 0, one power iteration; u, v are constants of the backward pass
  mel_forward / mel_vjp         hifigan's mel_spectrogram (reflect pad (n_fft - hop) / 2) and MelVocoder's (centred, log10) for any
                                win_size <= n_fft (periodic Hann of win_size centred in n_fft, as torch.stft and melspec._bases place it),
                                fmin, fmax or None
  gan_losses                    feature / generator / discriminator losses with their gradients

Every function takes `dtype`: float64 is the reference, float32 of the same code is the yardstick (what plain fp32 arithmetic makes of
the same problem).  `absolute=True` evaluates the absolute-value companion S of a result: the same linear operation on |operands| in
float64 (conv: conv(|lrelu(x)|, |w|) + |b|; dw: sum |dy| |lrelu(x)|; ...).  An fp32 evaluation's error on an element is at most a
small multiple of 2^-24 S, whatever the cancellation, so the tests bound errors per element by tau * S."""
import math

import numpy as np
import torch

from oracle import melspec_ref


def _t(a, dtype):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.detach().to('cpu', dtype)


def lrelu(x, slope):
    return x if slope == 1.0 else torch.where(x > 0, x, x * slope)


def lrelu_grad(x, slope):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))


# ---------------------------------------------------------------------------------------------------------------------- conv layer
def _fold(x, P):
    """[N, C, H * P] -> [N * P, C, H]: the P columns of a period-folded signal as independent sequences"""
    N, C, HP = x.shape
    return x.view(N, C, HP // P, P).permute(0, 3, 1, 2).reshape(N * P, C, HP // P)


def _unfold(x, N, P):
    NP, C, H = x.shape
    return x.view(N, P, C, H).permute(0, 2, 3, 1).reshape(N, C, H * P)


def _conv(a, w, b, stride, padding, groups, mutate=None):
    """a [N, Cin, L] (already activated) -> [N, Cout, Lout]; a sum over taps of stride-`stride` slices of the zero-padded input"""
    N, Cin, L = a.shape
    Cout, Cg, K = w.shape
    G = groups
    pad_l = padding + (1 if mutate == 'pad' else 0)
    Lout = (L + 2 * padding - K) // stride + 1
    ap = torch.zeros((N, Cin, L + 2 * padding + 2), dtype=a.dtype)
    ap[:, :, pad_l:pad_l + L] = a
    ag = ap.view(N, G, Cg, -1)
    wg = w.view(G, Cout // G, Cg, K)
    if mutate == 'group' and G > 1:
        wg = wg[[1, 0] + list(range(2, G))]
    y = torch.zeros((N, G, Cout // G, Lout), dtype=a.dtype)
    for k in range(K):
        if mutate == 'tap' and k == K // 2:
            continue
        y += torch.einsum('goc,ngcl->ngol', wg[..., k], ag[..., k:k + stride * (Lout - 1) + 1:stride])
    y = y.reshape(N, Cout, Lout)
    if b is not None and mutate != 'bias':
        y = y + b.view(1, -1, 1)
    return y


def conv_layer(x, w, b, stride=1, padding=0, groups=1, period=1, in_slope=1.0, dtype=torch.float64, absolute=False, mutate=None):
    """x [N, Cin, L * period] (pre-activation), w [Cout, Cin / groups, K], b [Cout] or None -> y [N, Cout, Lout * period].
    mutate (sensitivity tests only): 'tap' drops the middle tap, 'pad' shifts the padding by one sample, 'bias' drops the bias, 'group' swaps
    the weight slices of groups 0 and 1"""
    x, w, b = _t(x, dtype), _t(w, dtype), _t(b, dtype)
    a = lrelu(x, in_slope)
    if absolute:
        a, w, b = a.abs(), w.abs(), None if b is None else b.abs()
    N = x.shape[0]
    y = _conv(_fold(a, period) if period > 1 else a, w, b, stride, padding, groups, mutate)
    return _unfold(y, N, period) if period > 1 else y


def conv_layer_vjp(x, w, dy, stride=1, padding=0, groups=1, period=1, in_slope=1.0, dtype=torch.float64, absolute=False):
    """-> (dx, dw, db) of conv_layer for the cotangent dy [N, Cout, Lout * period]"""
    x, w, dy = _t(x, dtype), _t(w, dtype), _t(dy, dtype)
    a, gate = lrelu(x, in_slope), lrelu_grad(x, in_slope)
    if absolute:
        a, w, dy = a.abs(), w.abs(), dy.abs()
    N = x.shape[0]
    if period > 1:
        a, dy = _fold(a, period), _fold(dy, period)
    NP, Cin, L = a.shape
    Cout, Cg, K = w.shape
    G, Lout = groups, dy.shape[2]
    ap = torch.zeros((NP, Cin, L + 2 * padding), dtype=a.dtype)
    ap[:, :, padding:padding + L] = a
    ag = ap.view(NP, G, Cg, -1)
    wg = w.view(G, Cout // G, Cg, K)
    dyg = dy.reshape(NP, G, Cout // G, Lout)
    dap = torch.zeros_like(ag)
    dw = torch.empty((G, Cout // G, Cg, K), dtype=a.dtype)
    for k in range(K):
        sl = slice(k, k + stride * (Lout - 1) + 1, stride)
        dap[..., sl] += torch.einsum('goc,ngol->ngcl', wg[..., k], dyg)
        dw[..., k] = torch.einsum('ngol,ngcl->goc', dyg, ag[..., sl])
    da = dap.reshape(NP, Cin, -1)[:, :, padding:padding + L]
    if period > 1:
        da = _unfold(da, N, period)
    dx = da * gate if in_slope != 1.0 else da
    db = dy.sum(dim=(0, 2))
    return dx, dw.reshape(Cout, Cg, K), db


def deinterleave_w(w, s):
    """wp[co, (r, ci), j] = w[co, ci, s j + r] (zero beyond K): the weight layout of a strided layer's stride-1 convolution"""
    Cout, Cg, K = w.shape
    J = -(-K // s)
    wz = torch.zeros((Cout, Cg, s * J), dtype=w.dtype)
    wz[:, :, :K] = w
    return wz.view(Cout, Cg, J, s).permute(0, 3, 1, 2).reshape(Cout, s * Cg, J)


def deinterleave_w_adjoint(wp, s, K):
    """the adjoint of deinterleave_w: wp [Cout, s Cg, J] -> w [Cout, Cg, K]; the slots of taps s j + r >= K are dropped"""
    Cout, sCg, J = wp.shape
    return wp.reshape(Cout, s, sCg // s, J).permute(0, 2, 3, 1).reshape(Cout, sCg // s, J * s)[:, :, :K]


# ---------------------------------------------------------------------------------------------------------------------- weight norms
def weight_norm(v, g, dtype=torch.float64):
    v, g = _t(v, dtype), _t(g, dtype)
    R = v.shape[0]
    n = v.reshape(R, -1).norm(dim=1)
    return (g.reshape(R) / n).view((R,) + (1,) * (v.dim() - 1)) * v


def weight_norm_vjp(v, g, dw, dtype=torch.float64):
    """-> (dv, dg)"""
    v, g, dw = _t(v, dtype), _t(g, dtype), _t(dw, dtype)
    R = v.shape[0]
    v2, d2 = v.reshape(R, -1), dw.reshape(R, -1)
    n = v2.norm(dim=1)
    dot = (d2 * v2).sum(dim=1)
    gs = g.reshape(R)
    dv = (gs / n)[:, None] * (d2 - (dot / n ** 2)[:, None] * v2)
    return dv.view(v.shape), (dot / n).view(g.shape)


def _normalize(t, eps):
    return t / torch.clamp(t.norm(), min=eps)


def spectral_norm(w, u, v, training=True, eps=1e-12, dtype=torch.float64):
    """-> (wn, u', v', sigma): in training mode one power iteration v' = normalize(W^T u), u' = normalize(W v') first"""
    w, u, v = _t(w, dtype), _t(u, dtype), _t(v, dtype)
    W2 = w.reshape(w.shape[0], -1)
    if training:
        v = _normalize(W2.t() @ u, eps)
        u = _normalize(W2 @ v, eps)
    sigma = u @ (W2 @ v)
    return w / sigma, u, v, sigma


def spectral_norm_vjp(w, u, v, sigma, dwn, dtype=torch.float64):
    """u, v, sigma of the forward pass (held constant): dW = dWn / sigma - (sum dWn . W / sigma^2) u v^T"""
    w, u, v, dwn = _t(w, dtype), _t(u, dtype), _t(v, dtype), _t(dwn, dtype)
    sigma = _t(torch.as_tensor(sigma), dtype)
    W2, d2 = w.reshape(w.shape[0], -1), dwn.reshape(w.shape[0], -1)
    return (d2 / sigma - ((d2 * W2).sum() / sigma ** 2) * torch.outer(u, v)).view(w.shape)


# ---------------------------------------------------------------------------------------------------------------------- mel spectrogram
def mel_bases(n_fft, win_size, sr, n_mels, fmin, fmax, dtype=torch.float64):
    """-> (basis [2 nb, n_fft] = rows hann cos | -hann sin, mel [n_mels, nb], hann [n_fft])"""
    assert win_size <= n_fft
    hann = np.zeros(n_fft)
    off = (n_fft - win_size) // 2
    hann[off:off + win_size] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_size) / win_size)
    nb = n_fft // 2 + 1
    ang = 2.0 * np.pi * np.outer(np.arange(nb), np.arange(n_fft)) / n_fft
    basis = np.concatenate([np.cos(ang) * hann, -np.sin(ang) * hann], axis=0)
    mel = melspec_ref.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    return _t(basis, dtype), _t(mel, dtype), _t(hann, dtype)


def _reflect_index(L, pad):
    i = np.arange(-pad, L + pad)
    i = np.abs(i)
    return torch.from_numpy(np.where(i > L - 1, 2 * (L - 1) - i, i))


def _frames(yp, n_fft, hop, shift=None):
    F_ = (yp.shape[-1] - n_fft) // hop + 1
    idx = torch.arange(F_)[:, None] * hop + torch.arange(n_fft)[None, :]
    if shift is not None:
        idx[shift] += 1
    return idx


def mel_forward(y, n_fft, n_mels, sr, hop, win_size, fmin, fmax, pad=None, eps=1e-9, minv=1e-5, scale=1.0, dtype=torch.float64):
    """y [B, L] -> dict(out [B, n_mels, F], lin, mag, reim, yp, A_f [B, F] = sum_n |frame_n hann_n|).
    pad None = hifigan's (n_fft - hop) / 2; MelVocoder: pad = n_fft // 2, eps = 0, scale = 1 / ln 10"""
    y = _t(y, dtype)
    pad = int((n_fft - hop) / 2) if pad is None else pad
    basis, mel, hann = mel_bases(n_fft, win_size, sr, n_mels, fmin, fmax, dtype)
    yp = y[:, _reflect_index(y.shape[1], pad)]
    fr = yp[:, _frames(yp, n_fft, hop)]                                   # [B, F, n_fft]
    reim = fr @ basis.t()
    nb = n_fft // 2 + 1
    mag = torch.sqrt(reim[..., :nb] ** 2 + reim[..., nb:] ** 2 + eps)
    lin = mag @ mel.t()                                                   # [B, F, n_mels]
    out = scale * torch.log(torch.clamp(lin, min=minv))
    A_f = (fr.abs() * hann.abs()).sum(-1)
    return dict(out=out.transpose(1, 2), lin=lin, mag=mag, reim=reim, yp=yp, A_f=A_f, mel=mel, basis=basis, pad=pad)


def mel_vjp(f, g, n_fft, hop, minv=1e-5, scale=1.0, dtype=torch.float64, absolute=False, mutate=None):
    """the cotangent g [B, n_mels, F] of mel_forward's `out` -> dy [B, L].  mutate (sensitivity tests only): 'frame' moves the middle frame one sample
    right in the overlap-add, 'clamp' inverts the clamp mask"""
    g = _t(g, dtype).transpose(1, 2)
    lin, mag, reim, mel, basis = (_t(f[k], dtype) for k in ('lin', 'mag', 'reim', 'mel', 'basis'))
    mask = lin > minv
    if mutate == 'clamp':
        mask = ~mask
    dlin = torch.where(mask, g * scale / lin, torch.zeros_like(lin))
    nb = n_fft // 2 + 1
    if absolute:
        dlin, mel, basis = dlin.abs(), mel.abs(), basis.abs()
    dmag = dlin @ mel
    r = reim / torch.cat([mag, mag], dim=-1)
    dreim = torch.cat([dmag, dmag], dim=-1) * (r.abs() if absolute else r)
    dfr = dreim @ basis                                                   # [B, F, n_fft]
    B, F_, _ = dfr.shape
    Lp = f['yp'].shape[1]
    F_ = f['lin'].shape[1]
    idx = _frames(f['yp'], n_fft, hop, shift=F_ // 2 if mutate == 'frame' else None)
    dyp = torch.zeros((B, Lp + 1), dtype=dfr.dtype)
    dyp.index_add_(1, idx.reshape(-1), dfr.reshape(B, -1))
    L = Lp - 2 * f['pad']
    dy = torch.zeros((B, L), dtype=dfr.dtype)
    dy.index_add_(1, _reflect_index(L, f['pad']), dyp[:, :Lp])
    return dy


# ---------------------------------------------------------------------------------------------------------------------- GAN losses
def gan_losses(kind, a, b=None, target=1.0, weight=1.0, slopes=None, dtype=torch.float64):
    """the loss kernels' two kinds over a list of segments -> (loss, [grad of each a_k], [grad of each b_k]):
    kind 0: sum_k weight mean |lrelu(a_k, s_k) - lrelu(b_k, s_k)|   (feature_loss: weight 2)
    kind 1: sum_k weight mean (a_k - target)^2                        (generator_loss: target 1; discriminator_loss: 1 on real, 0 on generated)"""
    a = [_t(t, dtype) for t in a]
    loss = torch.zeros((), dtype=dtype)
    ga, gb = [], []
    if kind == 1:
        for t in a:
            d = t - target
            loss = loss + weight * (d * d).mean()
            ga.append(2.0 * weight * d / t.numel())
        return loss, ga, gb
    b = [_t(t, dtype) for t in b]
    for i, (p, q) in enumerate(zip(a, b)):
        s = 1.0 if slopes is None else slopes[i]
        d = lrelu(p, s) - lrelu(q, s)
        loss = loss + weight * d.abs().mean()
        sg = weight * torch.sign(d) / p.numel()
        ga.append(sg * lrelu_grad(p, s) if s != 1.0 else sg)
        gb.append(-sg * lrelu_grad(q, s) if s != 1.0 else -sg)
    return loss, ga, gb


def feature_loss(fmap_r, fmap_g, dtype=torch.float64):
    return gan_losses(0, fmap_r, fmap_g, weight=2.0, dtype=dtype)


def generator_loss(outs, dtype=torch.float64):
    return gan_losses(1, outs, target=1.0, dtype=dtype)


def discriminator_loss(real, gen, dtype=torch.float64):
    lr, gr, _ = gan_losses(1, real, target=1.0, dtype=dtype)
    lg, gg, _ = gan_losses(1, gen, target=0.0, dtype=dtype)
    return lr + lg, gr, gg


def log_mel_bound(f, tau, scale=1.0):
    """forward bound of the log-domain mel output per element: tau * ((mel . (A_f + mag)) / max(lin, 1e-5) + |out|) — A_f bounds the fp32
    error of every DFT bin of a frame, mag the rounding of the magnitude itself (sqrt(eps) of an all-zero frame has no DFT error but rounds),
    the mel projection carries both to lin, the log divides by lin (`scale`: 1 / ln 10 for log10); |out| covers the rounding of the logarithm's own result.  -> [B, n_mels, F]"""
    melA = (f['A_f'][..., None] + f['mag']) @ f['mel'].abs().t()
    return (tau * (scale * melA / torch.clamp(f['lin'], min=1e-5) + f['out'].transpose(1, 2).abs())).transpose(1, 2)


LN10 = math.log(10.0)

# Per-element bounds err <= tau * S of the GPU tests (tests/test_disc_f64_gpu.py, tests/test_mel_loss_f64_gpu.py).  The float32 yardstick of
# this module stays below them (tests/test_oracle_gan_step.py asserts it); the GPU maxima are recorded next to each use.
TAU_SPLIT = 2.0 ** -19          # fp16 hi/lo x 3 products (conv_train.hip, conv_wgrad.hip split kernels): ~2^-22 per product, fp32 accumulation
TAU_EXACT = 2.0 ** -21          # fp32 MFMA / fma kernels
TAU_MEL = 2.0 ** -19            # log-mel forward, in units of (mel . A_f) / lin
