"""GPU: the MPD / MSD convolutions of the GAN step (hifigan/disc_hip.py on csrc/conv_train.hip, conv_wgrad.hip, conv1d.hip and the
train_ops.hip de-interleave; weight preparation in wbank.py) and the GAN loss kernel against the float64 oracle (oracle/gan_step_ref.py).

Bound, per element: |got - ref| <= tau * S, S the absolute-value companion of the same linear operation in float64 (y: conv(|lrelu(x)|, |w|)
+ |b|; dx: the data gradient of |dy| through |w| and |lrelu'|; dw: sum |dy| |lrelu(x)|; db: sum |dy|).  tau = TAU_SPLIT (2^-19) where a
split-precision kernel (fp16 hi / lo x 3 products) may run the quantity, TAU_EXACT (2^-21) where only exact-fp32 kernels do; the float32
yardstick of the oracle stays under 5.5 * 2^-24 S on these shapes (tests/test_oracle_gan_step.py).  Measured on an MI355X, worst err / S in
units of 2^-24: split / banked / un-fused / grouped-split single layers 3.5-9.1 (bound 32), exact and fallback 3.5-6.8 (bound 8), whole modules
teacher-forced 9.1-10.1, weight norm 3.0-3.4, spectral norm 2.4-7.0, GAN losses 0.9-2.8; test_zz_report_measured prints them per path.

Single layers run every MPD (periods 2, 3, 5, 7, 11) and MSD layer shape at in_slope 1 and 0.1 under every dispatch switch: split / exact
(SPLIT_TRAIN), fused / un-fused de-interleave, banked (a WeightBank's prepared fragments) / per-launch weights, grouped split weight
gradients off, default and ALL; plus shapes outside ttsc_conv_train_supported (the automatic exact fallback).  Whole modules are checked
teacher-forced: every layer call's native input, weight and upstream gradient are captured and that layer alone is held to float64 at
those operands, so a leaky-relu gate that flips between native and float64 forward passes cannot make a correct kernel fail.  Outputs are
allocated fresh by the product code (torch.empty); every checked value must be finite."""
import contextlib

import pytest
import torch
import torch.nn as nn

from oracle import gan_step_ref as R

pytestmark = pytest.mark.gpu

MEASURED = {}


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), v)


def _bound(label, got, ref, S, tau):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), label + ': non-finite'
    r = float(((got - ref).abs() / S.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    _note(label.split(':')[0], r * 2 ** 24)
    assert r <= tau, '%s: max err / S = %.3g * 2^-24 > %.3g * 2^-24' % (label, r * 2 ** 24, tau * 2 ** 24)


@contextlib.contextmanager
def _switches(split=True, fused=True, gsplit=True, gsplit_all=False):
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan import disc_hip as DH
    old = (A.SPLIT_TRAIN, DH.FUSED_DEINTERLEAVE, A.GROUPED_SPLIT, A.GROUPED_SPLIT_ALL)
    A.SPLIT_TRAIN, DH.FUSED_DEINTERLEAVE, A.GROUPED_SPLIT, A.GROUPED_SPLIT_ALL = split, fused, gsplit, gsplit_all
    try:
        yield
    finally:
        A.SPLIT_TRAIN, DH.FUSED_DEINTERLEAVE, A.GROUPED_SPLIT, A.GROUPED_SPLIT_ALL = old


MODES = {'split': dict(), 'exact': dict(split=False), 'unfused': dict(fused=False), 'banked': dict(),
         'gsplit_off': dict(gsplit=False), 'gsplit_all': dict(gsplit_all=True)}

# (Cin, Cout, K, stride, padding, groups, period, H): H input rows of `period` samples
MPD = [(ci, co, 5, 3, 2, 1, P, H) for P in (2, 3, 5, 7, 11) for ci, co, H in ((1, 32, 600 // P), (32, 128, 400 // P), (128, 512, 240 // P),
                                                                               (512, 1024, 150 // P))] + \
      [(1024, 1024, 5, 1, 2, 1, P, 12) for P in (2, 3, 5, 7, 11)] + [(1024, 1, 3, 1, 1, 1, P, 12) for P in (2, 3, 5, 7, 11)]
MSD = [(1, 128, 15, 1, 7, 1, 1, 700), (128, 128, 41, 2, 20, 4, 1, 500), (128, 256, 41, 2, 20, 16, 1, 400), (256, 512, 41, 4, 20, 16, 1, 300),
       (512, 1024, 41, 4, 20, 16, 1, 120), (1024, 1024, 41, 1, 20, 16, 1, 40), (1024, 1024, 5, 1, 2, 1, 1, 40), (1024, 1, 3, 1, 1, 1, 1, 40)]
OUT_OF_SUPPORT = [(16, 64, 5, 1, 2, 4, 1, 300), (64, 64, 43, 1, 21, 1, 1, 200)]   # Cin / groups < 8, K > 41


def _layer(Cin, Cout, K, s, p, G):
    from torch.nn.utils import weight_norm
    return weight_norm(nn.Conv1d(Cin, Cout, K, s, padding=p, groups=G)).cuda()


def _wn_vjp_S(v, g, Sdw):
    """absolute-value companion of weight_norm_vjp for an |dw| bound Sdw"""
    v, g = v.detach().double().cpu(), g.detach().double().cpu()
    R_ = v.shape[0]
    v2, s2 = v.reshape(R_, -1), Sdw.reshape(R_, -1)
    n = v2.norm(dim=1)
    dot = (s2 * v2.abs()).sum(dim=1)
    dv = (g.reshape(R_).abs() / n)[:, None] * (s2 + (dot / n ** 2)[:, None] * v2.abs())
    return dv.view(v.shape), (dot / n).view(g.shape)


@pytest.mark.parametrize('Cin,Cout,K,s,p,G,P,H', MPD + MSD + OUT_OF_SUPPORT)
def test_layer_against_float64_on_every_path(Cin, Cout, K, s, p, G, P, H):
    from ttscube_amd import _lib
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan.disc_hip import HipStridedConv
    from ttscube_amd.hifigan.wbank import WeightBank
    torch.manual_seed(Cin + Cout + K + P + H)
    N = 2
    layer = _layer(Cin, Cout, K, s, p, G)
    with torch.no_grad():
        layer.bias.normal_(0, 0.1)
    h = HipStridedConv(Cin, Cout, K, s, p, G, period=P)
    tc = h.tc
    supported = bool(_lib.lib().ttsc_conv_train_supported(tc.Cin, tc.Cout, tc.K, tc.dilation, tc.groups))
    assert supported == ((Cin, Cout, K, s, p, G, P, H) not in OUT_OF_SUPPORT)
    x = torch.randn(N, Cin, H * P).cuda()
    modes = ['split', 'exact'] + (['unfused'] if s > 1 else []) + (['gsplit_off', 'gsplit_all'] if G > 1 else [])
    bankable = supported and bool(_lib.lib().ttsc_conv_train_supported(tc.Cout, tc.Cin, tc.K, tc.dilation, tc.groups)) and \
        tc.dilation * (tc.K - 1) - tc.padding >= 0       # (the rule disc_hip._bank_of applies)
    if bankable and A.USE_BANK:
        modes.append('banked')
    for slope in (1.0, 0.1):
        w64 = R.weight_norm(layer.weight_v, layer.weight_g)
        w = (layer.weight_g * layer.weight_v / layer.weight_v.reshape(Cout, -1).norm(dim=1).view(-1, 1, 1)).detach()   # reference weight: fp32
        b = layer.bias.detach().clone()
        y_ref = R.conv_layer(x, w, b, s, p, G, P, slope)
        S_y = R.conv_layer(x, w, b, s, p, G, P, slope, absolute=True)
        dy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(K + H)).float()
        dx_ref, dw_ref, db_ref = R.conv_layer_vjp(x, w, dy, s, p, G, P, slope)
        S_dx, S_dw, S_db = R.conv_layer_vjp(x, w, dy, s, p, G, P, slope, absolute=True)
        for mode in modes:
            with _switches(**MODES[mode]):
                split = A._split_ok(tc.Cin, tc.Cout, tc.K, tc.dilation, tc.groups)
                assert split == (mode != 'exact' and supported), (mode, split)
                tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
                label = '%s %s:' % (mode if split or mode == 'exact' else 'fallback', 'K%d G%d s%d' % (K, G, s))
                xi = x.clone().requires_grad_(True)
                if mode == 'banked':
                    layer.weight_v.grad = layer.weight_g.grad = None
                    bank = WeightBank([(layer, Cin, Cout, K, G, s)])
                    bank.prepare()
                    wi = bank.weight(0)
                    assert wi._ttsc_pack is not None
                    _bound(label + ' w', bank.entries[0].w.view(Cout, Cin // G, K), w64, w64.abs(), R.TAU_EXACT)
                    bi = layer.bias
                    layer.bias.grad = None
                else:
                    wi = w.clone().requires_grad_(True)
                    bi = b.clone().requires_grad_(True)
                y = h(xi, wi, bi, in_slope=slope)
                _bound(label + ' y', y, y_ref, S_y, tau)
                gx, = torch.autograd.grad(y, xi, dy.cuda(), retain_graph=True)
                _bound(label + ' dx', gx, dx_ref, S_dx, tau)
                if mode == 'banked':
                    y.backward(dy.cuda())
                    dv_ref, dg_ref = R.weight_norm_vjp(layer.weight_v, layer.weight_g, dw_ref.view(layer.weight_v.shape))
                    S_dv, S_dg = _wn_vjp_S(layer.weight_v, layer.weight_g, S_dw.view(layer.weight_v.shape))
                    _bound(label + ' dv', layer.weight_v.grad, dv_ref, S_dv, tau)
                    _bound(label + ' dg', layer.weight_g.grad, dg_ref, S_dg, tau)
                    _bound(label + ' db', layer.bias.grad, db_ref, S_db, tau)
                else:
                    gw, gb = torch.autograd.grad(y, (wi, bi), dy.cuda())
                    _bound(label + ' dw', gw, dw_ref, S_dw, tau)
                    _bound(label + ' db', gb, db_ref, S_db, tau)


class _Tap(torch.autograd.Function):
    """identity whose backward records the gradient that flows through it"""

    @staticmethod
    def forward(ctx, t, rec, key):
        ctx.rec, ctx.key = rec, key
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        ctx.rec[ctx.key] = g.detach().clone()
        return g, None, None


def _capture(monkeypatch):
    """wraps HipStridedConv.__call__: every layer call's input, weight, bias, slope, output and (after backward) its upstream gradient and the
    gradients it produced for its own input / weight / bias"""
    from ttscube_amd.hifigan import disc_hip as DH
    from ttscube_amd.hifigan.wbank import pass_range
    calls = []
    orig = DH.HipStridedConv.__call__

    def call(self, x, w, b, in_slope=1.0):
        rec = dict(h=self, x=x.detach().clone(), slope=in_slope, banked=getattr(w, '_ttsc_pack', None) is not None, b=b.detach().clone())
        xi = pass_range(x, _Tap.apply(x, rec, 'dx')) if x.requires_grad else x
        wi = _Tap.apply(w, rec, 'dw') if w.requires_grad else w
        if rec['banked']:
            wi._ttsc_pack = w._ttsc_pack
        rec['w'] = w.detach().clone() if not rec['banked'] else None
        bi = _Tap.apply(b, rec, 'db') if b.requires_grad else b
        y = orig(self, xi, wi, bi, in_slope)
        rec['y'] = y.detach().clone()
        if y.requires_grad:
            y.register_hook(lambda g: rec.__setitem__('dy', g.detach().clone()))
        calls.append(rec)
        return y

    monkeypatch.setattr(DH.HipStridedConv, '__call__', call)
    return calls


def _check_calls(calls, layer_of, tag):
    """each captured call against the float64 layer at its own operands"""
    from ttscube_amd.hifigan import autograd as A
    assert calls
    for rec in calls:
        h = rec['h']
        l = layer_of[id(h)]
        tc = h.tc
        split = A._split_ok(tc.Cin, tc.Cout, tc.K, tc.dilation, tc.groups)
        tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
        if rec['banked']:
            w = l._wbank_w.detach().cpu()
        else:
            w = rec['w'].cpu().reshape(h.Cout, h.Cin // h.G, h.K)
        args = (h.s, h.p, h.G, h.P, rec['slope'])
        label = '%s %s %s:' % (tag, 'split' if split else 'exact', 'banked' if rec['banked'] else 'plain')
        x = rec['x'].cpu()
        _bound(label + ' y', rec['y'], R.conv_layer(x, w, rec['b'].cpu(), *args), R.conv_layer(x, w, rec['b'].cpu(), *args, absolute=True), tau)
        if 'dy' not in rec:
            continue
        dy = rec['dy'].cpu()
        ref = R.conv_layer_vjp(x, w, dy, *args)
        S = R.conv_layer_vjp(x, w, dy, *args, absolute=True)
        if 'dx' in rec:
            _bound(label + ' dx', rec['dx'], ref[0], S[0], tau)
        if 'dw' in rec:
            got = rec['dw'].cpu()
            if rec['banked'] and h.s > 1:      # the bank hands out the weight in the strided layer's de-interleaved layout; its backward drops
                got = R.deinterleave_w_adjoint(got, h.s, h.K)     # the slots of the zero taps beyond K
            _bound(label + ' dw', got, ref[1], S[1], tau)
        if 'db' in rec:
            _bound(label + ' db', rec['db'], ref[2], S[2], tau)


def _modules(which):
    from ttscube_amd.hifigan import discriminators as D
    from ttscube_amd.hifigan import disc_hip as DH
    torch.manual_seed(17)
    m = (D.MultiPeriodDiscriminator() if which == 'mpd' else D.MultiScaleDiscriminator()).cuda()
    layer_of = {}
    for d in m.discriminators:
        for l, h in zip(list(d.convs) + [d.conv_post], DH._layers(d, 'p' if which == 'mpd' else 's')):
            layer_of[id(h)] = l
    return m, layer_of


def _effective_weights(m, which):
    """the fp32 effective weight each banked layer's kernels used: the bank's buffer (original [Cout, Cg, K] layout)"""
    from ttscube_amd.hifigan import disc_hip as DH
    bank, index = DH._bank_of(m, 'p' if which == 'mpd' else 's')
    for d in m.discriminators:
        for l in list(d.convs) + [d.conv_post]:
            i = index.get(id(l)) if bank else None
            if i is not None:
                e = bank.entries[i]
                object.__setattr__(l, '_wbank_w', e.w.view(e.Cout, e.Cin // e.groups, e.K))
                w64 = R.weight_norm(l.weight_v, l.weight_g).reshape(e.Cout, e.Cin // e.groups, e.K)
                _bound('%s weight_norm:' % which, e.w, w64, w64.abs(), R.TAU_EXACT)


@pytest.mark.parametrize('which,B,T,disc_step', [('mpd', 4, 12000, False), ('msd', 4, 12000, False), ('mpd', 4, 12001, False),
                                                  ('mpd', 16, 12000, True), ('msd', 16, 12000, True)])
def test_module_teacher_forced_per_layer(monkeypatch, which, B, T, disc_step):
    """mpd_forward / msd_forward and the backward of a fixed random cotangent on scores and feature maps; T = 12 001 is a multiple of none of
    the periods (reflect fold); disc_step: generated audio without a graph, real + generated as one batch (the discriminator step's call)"""
    from ttscube_amd.hifigan import disc_hip as DH
    m, layer_of = _modules(which)
    g = torch.Generator().manual_seed(B + T)
    y = (torch.rand(B, 1, T, generator=g) - 0.5).cuda()
    yh = (torch.rand(B, 1, T, generator=g) - 0.5).cuda()
    if not disc_step:
        yh.requires_grad_(True)
    calls = _capture(monkeypatch)
    snap = None
    if which == 'msd':
        snap = [(l, l.weight_u.clone(), l.weight_v.clone()) for l in list(m.discriminators[0].convs) + [m.discriminators[0].conv_post]]
    out = (DH.mpd_forward if which == 'mpd' else DH.msd_forward)(m, y, yh)
    _effective_weights(m, which)
    tens = [t for t in out[0] + out[1]] + [f for fl in out[2] + out[3] for f in fl]
    cot = [torch.randn(t.shape, generator=g).cuda() for t in tens]
    torch.autograd.backward([t for t in tens if t.requires_grad], [c for t, c in zip(tens, cot) if t.requires_grad])
    _check_calls(calls, layer_of, which)
    if snap is not None:      # MSD 0 is spectrally normed: one power iteration per call (real, generated: two calls) on weight_u / weight_v
        ncalls = 2          # (MSD 0 never batches real and generated: disc_hip.msd_forward)
        for l, u0, v0 in snap:
            u, v = u0.double().cpu(), v0.double().cpu()
            for _ in range(ncalls):
                _, u, v, _ = R.spectral_norm(l.weight_orig, u, v, True)
            _bound('msd0 power iteration: u', l.weight_u, u, u.abs() + 1.0 / u.numel() ** 0.5, 2 ** -16)
            _bound('msd0 power iteration: v', l.weight_v, v, v.abs() + 1.0 / v.numel() ** 0.5, 2 ** -16)


@pytest.mark.parametrize('Cout,Cin,K,groups', [(128, 1, 15, 1), (128, 32, 41, 4), (256, 8, 41, 16), (1024, 32, 41, 16), (1024, 1024, 5, 1),
                                               (1, 1024, 3, 1)])
def test_spectral_norm_against_float64(Cout, Cin, K, groups):
    """HipSpectralNormFn (MSD 0's layers): the normalised weight, the power iteration, sigma and the gradient w.r.t. weight_orig with u, v
    held constant, against the float64 oracle per element (S = |W| / sigma and its companion)"""
    from torch.nn.utils import spectral_norm
    from ttscube_amd.hifigan.disc_hip import _weight
    torch.manual_seed(Cout + K)
    a = spectral_norm(nn.Conv1d(Cin * groups, Cout, K, groups=groups)).cuda()
    for training in (True, False):
        a.train(training)
        u0, v0 = a.weight_u.detach().clone().cpu(), a.weight_v.detach().clone().cpu()
        wn = _weight(a)
        wn_ref, u, v, sigma = R.spectral_norm(a.weight_orig, u0, v0, training)
        _bound('spectral_norm w:', wn, wn_ref, a.weight_orig.detach().double().cpu().abs() / float(sigma), 2 ** -20)
        _bound('spectral_norm u:', a.weight_u, u, u.abs() + 1.0 / u.numel() ** 0.5, 2 ** -20)
        _bound('spectral_norm v:', a.weight_v, v, v.abs() + 1.0 / v.numel() ** 0.5, 2 ** -20)
        dwn = torch.randn(wn.shape, generator=torch.Generator().manual_seed(K)).cuda()
        gw, = torch.autograd.grad(wn, a.weight_orig, dwn)
        ref = R.spectral_norm_vjp(a.weight_orig, u, v, sigma, dwn)
        W = a.weight_orig.detach().double().cpu()
        S = (dwn.double().cpu().abs() / float(sigma) + float((dwn.double().cpu() * W).abs().sum()) / float(sigma) ** 2
             * torch.outer(u.abs(), v.abs()).view(W.shape))
        _bound('spectral_norm dw:', gw, ref, S, 2 ** -20)


def _segments(B, with_msd=True):
    """the real step's feature-map / score shapes at B utterances of 12 000 samples: MPD 5 x (5 convs + conv_post), MSD 3 x (7 + 1)"""
    shapes = []
    for P in (2, 3, 5, 7, 11):
        Hh = -(-12000 // P)
        for co, st in ((32, 3), (128, 3), (512, 3), (1024, 3), (1024, 1), (1, 1)):
            Hh = (Hh + 4 - 5) // st + 1 if co != 1 else Hh
            shapes.append((B, co, Hh, P))
    if with_msd:
        for Ls in (12000, 6001, 3001):
            Lc = Ls
            for co, st in ((128, 1), (128, 2), (256, 2), (512, 4), (1024, 4), (1024, 1), (1024, 1), (1, 1)):
                Lc = (Lc - 1) // st + 1
                shapes.append((B, co, Lc))
    return shapes


@pytest.mark.parametrize('nseg', [54, 64, 65])
def test_gan_loss_kernel_against_float64(nseg):
    """gan_loss_kernel (losses_hip._ListLoss): kind 0 with and without the leaky-relu pre-activation variant, kind 1 at target 1 and 0, over the
    real step's 54 segments and exactly GAN_LOSS_MAX_SEG = 64; 65 segments must raise the ttsc_gan_loss argument error, not truncate"""
    from ttscube_amd import _lib
    from ttscube_amd.hifigan.losses_hip import _ListLoss
    shapes = _segments(1)
    while len(shapes) < nseg:
        shapes.append((1, 3, 17 + len(shapes)))
    shapes = shapes[:nseg]
    g = torch.Generator().manual_seed(nseg)
    a = [torch.randn(s, generator=g) for s in shapes]
    b = [torch.randn(s, generator=g) for s in shapes]
    slopes = [0.1 if i % 6 != 5 else 1.0 for i in range(nseg)]
    if nseg > 64:
        for kind, args in ((0, [t.cuda() for t in a + b]), (1, [t.cuda() for t in a])):
            with pytest.raises(_lib.TTSCError, match='ttsc_gan_loss'):
                _ListLoss.apply(kind, 0.0, 2.0, *[t.requires_grad_(True) for t in args])
        return
    for kind, target, weight, sl in ((0, 0.0, 2.0, None), (0, 0.0, 2.0, slopes), (1, 1.0, 1.0, None), (1, 0.0, 1.0, None)):
        ts = [t.cuda().requires_grad_(True) for t in (a + b if kind == 0 else a)]
        loss = _ListLoss.apply(kind, target, (weight, tuple(sl)) if sl else weight, *ts)
        grads = torch.autograd.grad(loss, ts)
        ref, ga, gb = R.gan_losses(kind, a, b if kind == 0 else None, target=target, weight=weight, slopes=sl)
        if kind == 0:
            S = sum(weight * (R.lrelu(p.double(), s_ if sl else 1.0).abs() + R.lrelu(q.double(), s_ if sl else 1.0).abs()).mean()
                    for p, q, s_ in zip(a, b, sl or [1.0] * nseg))
        else:
            S = sum(weight * ((p.double() - target) ** 2).mean() for p in a)
        label = 'gan_loss kind %d%s:' % (kind, ' lrelu' if sl else '')
        _bound(label + ' loss', loss, ref, S, R.TAU_EXACT)
        for i, (got, want) in enumerate(zip(grads, ga + gb)):
            _bound(label + ' grad', got, want, want.abs() + 1e-30, R.TAU_EXACT)


def test_zz_report_measured():
    """prints the worst measured err / S per path (units of 2^-24)"""
    for k in sorted(MEASURED):
        print('MEASURED %-40s %.3f' % (k, MEASURED[k]))
