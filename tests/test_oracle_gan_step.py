"""CPU: the float64 GAN-step oracle (oracle/gan_step_ref.py) against torch float64 autograd over the torch-op formulations
(tests/torch_reference.py, torch's weight-norm / spectral-norm hooks, torch.stft) and against oracle/melspec_ref.py; the float32 yardstick of
the same code stays inside the per-element bounds tau * S the GPU tests use; and each bound catches a one-tap, one-sample, one-frame or
one-mask error by at least 100x."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import gan_step_ref as R
from oracle import melspec_ref as M

TOL = 1e-12
D64 = torch.float64


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def _ratio(got, ref, S):
    """max |got - ref| / S over the elements (S > 0)"""
    return float(((got.double() - ref).abs() / S.clamp(min=1e-300)).max())


# (Cin, Cout, K, stride, padding, groups, period, N, L): every MPD / MSD layer kind at small lengths
LAYERS = [(1, 32, 5, 3, 2, 1, 2, 2, 301), (32, 128, 5, 3, 2, 1, 3, 2, 101), (128, 512, 5, 3, 2, 1, 11, 1, 31), (1024, 1024, 5, 1, 2, 1, 5, 1, 9),
          (1024, 1, 3, 1, 1, 1, 7, 2, 6), (1, 128, 15, 1, 7, 1, 1, 2, 500), (128, 128, 41, 2, 20, 4, 1, 2, 400), (128, 256, 41, 2, 20, 16, 1, 2, 300),
          (256, 512, 41, 4, 20, 16, 1, 1, 200), (1024, 1024, 41, 1, 20, 16, 1, 1, 30), (1024, 1024, 5, 1, 2, 1, 1, 1, 40), (1024, 1, 3, 1, 1, 1, 1, 2, 30)]


def _layer_case(Cin, Cout, K, s, p, G, P, N, L, seed=0):
    g = torch.Generator().manual_seed(seed + Cin + Cout + K + P)
    x = torch.randn(N, Cin, L * P, generator=g, dtype=D64)
    w = torch.randn(Cout, Cin // G, K, generator=g, dtype=D64) / (Cin // G * K) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=D64) * 0.1
    return x, w, b, g


@pytest.mark.parametrize('Cin,Cout,K,s,p,G,P,N,L', LAYERS)
def test_conv_layer_matches_torch_autograd(Cin, Cout, K, s, p, G, P, N, L):
    x, w, b, g = _layer_case(Cin, Cout, K, s, p, G, P, N, L)
    for slope in (1.0, 0.1):
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        if P > 1:   # DiscriminatorP's Conv2d((K, 1), (s, 1)) on the [N, C, H, P] fold
            ref = F.conv2d(F.leaky_relu(xr.view(N, Cin, L, P), slope), wr[..., None], br, stride=(s, 1), padding=(p, 0)).flatten(2)
        else:
            ref = F.conv1d(F.leaky_relu(xr, slope), wr, br, stride=s, padding=p, groups=G)
        y = R.conv_layer(x, w, b, s, p, G, P, slope)
        assert y.shape == ref.shape and _rel(y, ref.detach()) < TOL
        dy = torch.randn(ref.shape, generator=g, dtype=D64)
        want = torch.autograd.grad(ref, (xr, wr, br), dy)
        for got, ref_, name in zip(R.conv_layer_vjp(x, w, dy, s, p, G, P, slope), want, 'xwb'):
            assert got.shape == ref_.shape and _rel(got, ref_) < TOL, (name, slope)


@pytest.mark.parametrize('kind', ['p', 's'])
def test_sub_discriminator_chain_matches_torch_reference(kind):
    """a whole sub-discriminator (torch's weight-norm hooks, TR.disc_p_forward / disc_s_forward) against the oracle's layers chained with the
    oracle's weight norm, values and every parameter gradient of a random cotangent on all feature maps"""
    from ttscube_amd.hifigan import discriminators as D
    from tests import torch_reference as TR
    torch.manual_seed(3)
    d = (D.DiscriminatorP(3) if kind == 'p' else D.DiscriminatorS()).double()
    x = torch.randn(2, 1, 1000 if kind == 'p' else 700, dtype=D64)
    out, fmaps = (TR.disc_p_forward if kind == 'p' else TR.disc_s_forward)(d, x)
    g = torch.Generator().manual_seed(4)
    cots = [torch.randn(f.shape, generator=g, dtype=D64) for f in fmaps]
    params = [p_ for p_ in d.parameters()]
    want = torch.autograd.grad(sum((f * c).sum() for f, c in zip(fmaps, cots)), params)
    want = dict(zip([n for n, _ in d.named_parameters()], want))
    layers = list(d.convs) + [d.conv_post]
    P = d.period if kind == 'p' else 1
    h = x
    if kind == 'p' and x.shape[2] % P:
        h = F.pad(h, (0, P - x.shape[2] % P), 'reflect')
    saved = []
    for i, l in enumerate(layers):
        w = R.weight_norm(l.weight_v, l.weight_g).reshape(l.out_channels, -1, l.kernel_size[0])
        st, pd = l.stride[0], l.padding[0]
        slope = 1.0 if i == 0 else 0.1
        y = R.conv_layer(h, w, l.bias, st, pd, l.groups, P, slope)
        f = R.lrelu(y, 0.1) if i < len(layers) - 1 else y
        assert _rel(f, fmaps[i].reshape(f.shape).detach()) < TOL, i
        saved.append((h, w, st, pd, l.groups, slope))
        h = y
    dh = None
    for i in reversed(range(len(layers))):
        l = layers[i]
        hin, w, st, pd, G, slope = saved[i]
        c = cots[i].reshape(hin.shape[0], l.out_channels, -1)          # (MPD's [N, C, H, P] maps flatten to the h P + w order)
        dy = c * R.lrelu_grad(saved[i + 1][0], 0.1) if i < len(layers) - 1 else c
        if dh is not None:
            dy = dy + dh
        dh, dw, db = R.conv_layer_vjp(hin, w, dy, st, pd, G, P, slope)
        dv, dg = R.weight_norm_vjp(l.weight_v, l.weight_g, dw.reshape(l.weight_v.shape))
        name = ('convs.%d' % i) if i < len(layers) - 1 else 'conv_post'
        assert _rel(dv, want[name + '.weight_v']) < TOL and _rel(dg, want[name + '.weight_g']) < TOL and _rel(db, want[name + '.bias']) < TOL, name


def test_spectral_norm_matches_torch_hook():
    from torch.nn.utils import spectral_norm
    torch.manual_seed(5)
    a = spectral_norm(nn.Conv1d(128, 256, 41, groups=16)).double()
    for training in (True, False):
        a.train(training)
        u0, v0 = a.weight_u.clone(), a.weight_v.clone()
        for hook in a._forward_pre_hooks.values():
            hook(a, (None,))
        wn, u, v, sigma = R.spectral_norm(a.weight_orig, u0, v0, training)
        assert _rel(wn, a.weight.detach()) < TOL and _rel(u, a.weight_u) < TOL and _rel(v, a.weight_v) < TOL
        dwn = torch.randn(a.weight.shape, dtype=D64)
        want, = torch.autograd.grad(a.weight, a.weight_orig, dwn)
        assert _rel(R.spectral_norm_vjp(a.weight_orig, u, v, sigma, dwn), want) < TOL


def test_gan_losses_match_torch_reference():
    from tests import torch_reference as TR
    g = torch.Generator().manual_seed(6)
    shapes = [(3, 7), (3, 1, 40), (3, 5, 11, 2), (3, 13)]
    r = [torch.randn(s, generator=g, dtype=D64, requires_grad=True) for s in shapes]
    q = [torch.randn(s, generator=g, dtype=D64, requires_grad=True) for s in shapes]
    loss, ga, gb = R.feature_loss(r, q)
    want = TR.feature_loss([r], [q])
    assert abs(float(loss - want)) < TOL * float(want)
    for got, ref_ in zip(ga + gb, torch.autograd.grad(want, r + q)):
        assert _rel(got, ref_) < TOL
    loss, ga, _ = R.generator_loss(q)
    want = TR.generator_loss(q)[0]
    assert abs(float(loss - want)) < TOL * float(want)
    for got, ref_ in zip(ga, torch.autograd.grad(want, q)):
        assert _rel(got, ref_) < TOL
    loss, ga, gb = R.discriminator_loss(r, q)
    want = TR.discriminator_loss(r, q)[0]
    assert abs(float(loss - want)) < TOL * float(want)
    for got, ref_ in zip(ga + gb, torch.autograd.grad(want, r + q)):
        assert _rel(got, ref_) < TOL
    # feature maps handed over as pre-activations: leaky-relu inside the loss
    loss, ga, gb = R.gan_losses(0, r, q, weight=2.0, slopes=[0.1] * len(r))
    want = TR.feature_loss([[F.leaky_relu(t, 0.1) for t in r]], [[F.leaky_relu(t, 0.1) for t in q]])
    assert abs(float(loss - want)) < TOL * float(want)
    for got, ref_ in zip(ga + gb, torch.autograd.grad(want, r + q)):
        assert _rel(got, ref_) < TOL


def _audio(B, L, seed, silence=True):
    rng = np.random.RandomState(seed)
    t = np.arange(L) / 24000.0
    y = np.stack([0.4 * np.sin(2 * np.pi * rng.uniform(80, 4000) * t + rng.uniform(0, 6)) + 0.05 * rng.randn(L) for _ in range(B)])
    if silence:
        y[:, :L // 5] = 0.0
    return torch.from_numpy(y)


def _mel_torch64(y, n_fft, n_mels, sr, hop, win, fmin, fmax):
    """hifigan's mel_spectrogram as tests/torch_reference.py writes it, in float64 throughout (torch.stft, float64 filterbank)"""
    pad = int((n_fft - hop) / 2)
    yp = F.pad(y.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1)
    spec = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=D64), center=False, normalized=False,
                      onesided=True, return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    mel = torch.from_numpy(M.mel_filterbank(sr, n_fft, n_mels, fmin, fmax))
    return torch.log(torch.clamp(torch.matmul(mel, spec), min=1e-5))


MEL_CASES = [(1024, 240, 1024, 0, 12000), (1024, 275, 1024, 0, 12000), (1024, 256, 800, 80, None), (512, 512, 512, 0, 8000)]


@pytest.mark.parametrize('n_fft,hop,win,fmin,fmax', MEL_CASES)
def test_mel_matches_torch_stft_autograd(n_fft, hop, win, fmin, fmax):
    y = _audio(2, 5003, 1, silence=False)   # (digital silence puts lin just above the clamp: 1 / lin magnifies float64 rounding to ~2e-12)
    yr = y.clone().requires_grad_()
    ref = _mel_torch64(yr, n_fft, 80, 24000, hop, win, fmin, fmax)
    f = R.mel_forward(y, n_fft, 80, 24000, hop, win, fmin, fmax)
    assert f['out'].shape == ref.shape and _rel(f['out'], ref.detach()) < TOL
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2), dtype=D64)
    want, = torch.autograd.grad(ref, yr, g)
    assert _rel(R.mel_vjp(f, g, n_fft, hop), want) < TOL


def test_mel_matches_melspec_oracle():
    y = _audio(2, 12007, 3)
    f = R.mel_forward(y, 1024, 80, 24000, 240, 1024, 0, 12000)
    for b in range(2):
        assert _rel(f['out'][b], M.mel_spectrogram_ln(y[b].numpy(), 1024, 80, 24000, 240, 1024, 0, 12000)) < TOL
    f = R.mel_forward(y, 1024, 80, 24000, 240, 1024, 0.0, None, pad=512, eps=0.0, scale=1.0 / R.LN10)
    for b in range(2):
        assert _rel(f['out'][b].t(), M.melspectrogram_log10(y[b].numpy())) < TOL


# ---------------------------------------------------------------------------------------------------------------------- yardstick and sensitivity
@pytest.mark.parametrize('Cin,Cout,K,s,p,G,P,N,L', LAYERS)
def test_conv_yardstick_within_tau_and_mutations_caught(Cin, Cout, K, s, p, G, P, N, L):
    """float32 of the same code: max err / S <= TAU_EXACT on y, dx, dw, db (measured: <= 5.5 * 2^-24 over these shapes); a dropped tap, padding
    shifted by one sample, a missing bias and (grouped layers) two swapped group slices each exceed TAU_SPLIT * S by >= 100x somewhere"""
    x, w, b, g = _layer_case(Cin, Cout, K, s, p, G, P, N, L, seed=11)
    for slope in (1.0, 0.1):
        args = (s, p, G, P, slope)
        y = R.conv_layer(x, w, b, *args)
        S = R.conv_layer(x, w, b, *args, absolute=True)
        assert _ratio(R.conv_layer(x, w, b, *args, dtype=torch.float32), y, S) <= R.TAU_EXACT
        dy = torch.randn(y.shape, generator=g, dtype=D64)
        ref = R.conv_layer_vjp(x, w, dy, *args)
        yard = R.conv_layer_vjp(x, w, dy, *args, dtype=torch.float32)
        Sg = R.conv_layer_vjp(x, w, dy, *args, absolute=True)
        for a, r_, s_ in zip(yard, ref, Sg):
            assert _ratio(a, r_, s_) <= R.TAU_EXACT
        muts = ['tap', 'pad', 'bias'] + (['group'] if G > 1 else [])
        if K == 1:
            muts.remove('tap')
        for m in muts:
            assert _ratio(R.conv_layer(x, w, b, *args, mutate=m), y, S) >= 100 * R.TAU_SPLIT, m


def test_mel_yardstick_within_bounds_and_mutations_caught():
    """forward: the float32 yardstick stays inside TAU_MEL * (mel . A_f) / lin (measured ~2^-23 of it); VJP: a frame moved by one sample in the
    overlap-add and the inverted clamp mask each exceed the GPU test's bound (4 x yardstick + 1e-6, relative L2 per utterance) by >= 100x"""
    y = _audio(2, 12007, 5)
    y[1] *= 1e-4
    kw = (1024, 80, 24000, 240, 1024, 0, 12000)
    f = R.mel_forward(y, *kw)
    f32 = R.mel_forward(y, *kw, dtype=torch.float32)
    bound = R.log_mel_bound(f, R.TAU_MEL)
    near = (f['lin'] - 1e-5).abs().transpose(1, 2) <= bound * f['lin'].clamp(min=1e-5).transpose(1, 2)
    err = (f32['out'].double() - f['out']).abs()
    assert bool((err[~near] <= bound[~near] / 4).all()), float((err[~near] / bound[~near]).max())
    assert int(near.sum()) < 0.01 * near.numel()
    g = torch.randn(f['out'].shape, generator=torch.Generator().manual_seed(9), dtype=D64)
    ref = R.mel_vjp(f, g, 1024, 240)
    yard = R.mel_vjp(f32, g, 1024, 240, dtype=torch.float32)
    for b in range(2):
        rel_y = float((yard[b].double() - ref[b]).norm() / ref[b].norm())
        lim = 4 * rel_y + 1e-6
        assert rel_y < 1e-4
        for m in ('frame', 'clamp'):
            mut = R.mel_vjp(f, g, 1024, 240, mutate=m)
            assert float((mut[b] - ref[b]).norm() / ref[b].norm()) >= 100 * lim, (m, b)
