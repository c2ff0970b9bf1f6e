"""GPU: the generator's training layers as autograd runs them — hifigan/autograd.py::hip_conv (HipConvFn forward, data gradient, weight
gradient, bias gradient, residual gradient; Conv1d and ConvTranspose1d) — held PER ELEMENT to the float64 statement of the layer
(tests/conv_train_reference.py) at the native operands, and every convolution call inside generator_forward_with_grad held the same way,
teacher-forced: each call's native input, weight, bias, residual and upstream gradient are captured and that call alone is checked, so
a leaky-relu gate that flips between native and float64 runs cannot fail a correct kernel, while a range word that is stale, too small or
shared across branch streams fails the layer it feeds (lost low halves, or an fp16 overflow).

Bound: |got - ref64| <= tau * S per element, S the absolute-value companion; tau = 2^-19 where split-precision kernels may run, 2^-21 with
SPLIT_TRAIN off (TAU_SPLIT / TAU_EXACT of tests/test_disc_f64_gpu.py: the same kernels, the same derivation).  Each single layer runs three
ways — per-launch weights, banked (a WeightBank over the layer, AmaxPool.reset() first), SPLIT_TRAIN off — and asserts which kernel every
leg reaches through _split_ok and the plan queries.  Measured on an MI355X, worst err / S in units of 2^-24 (test_zz_report_measured, DESIGN.md
section 2e): Conv1d layer per-launch 8.2, banked 8.2 (bound 32), SPLIT_TRAIN off 6.3 (bound 8); ConvTranspose1d 9.4 (32) and 7.1 (8); the
generator's 78 calls teacher-forced 5.5 (Conv1d) and 7.7 (ConvTranspose1d) in both modes."""
import contextlib

import pytest
import torch
import torch.nn as nn

from oracle import hifigan_ref
from tests import conv_train_reference as R
from tests.test_conv_train_f64_gpu import conv_plan, wgrad_plan

pytestmark = pytest.mark.gpu

MEASURED = {}
SCALE, SLOPE = 1.0 / 3.0, 0.1


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), v)


def _bound(label, got, ref, S, tau):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), label + ': non-finite'
    r = float(((got - ref).abs() / S.clamp(min=1e-300)).max()) if ref.numel() else 0.0
    _note(label.split(':')[0], r * 2 ** 24)
    assert r <= tau, '%s: max err / S = %.3g * 2^-24 > %.3g * 2^-24' % (label, r * 2 ** 24, tau * 2 ** 24)


@contextlib.contextmanager
def _switches(split=True, bank=True):
    from ttscube_amd.hifigan import autograd as A
    old = (A.SPLIT_TRAIN, A.USE_BANK)
    A.SPLIT_TRAIN, A.USE_BANK = split, bank
    try:
        yield
    finally:
        A.SPLIT_TRAIN, A.USE_BANK = old


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


# ---- single layers ---------------------------------------------------------------------------------------------------------------------------
# Conv1d: (Cin, Cout, K, dilation, weight gradient on the split kernel (A = Cout >= 64 rows and Bc = Cin >= 32 columns))
CONV1D = [(80, 512, 7, 1, True)] + [(C, C, K, d, C >= 64) for C in (256, 128, 64, 32) for K, d in ((3, 1), (7, 3), (11, 5))] + [(32, 1, 7, 1, False)]
CONV1D_L = (1, 50, 257)
# ConvTranspose1d: (Cin, Cout, K, u, p, m_lo, M, Lo(L), weight gradient on the split kernel (u Cout >= 64 rows, Cin >= 32 columns))
GEOMETRIES = [(16, 5, 5, -1, 4, lambda L: 5 * L + 1), (16, 3, 6, -2, 6, lambda L: 3 * L + 1), (4, 4, 0, 0, 1, lambda L: 4 * L)]
TRANSPOSED = []
for (_K, _u, _p, _mlo, _M, _Lo), (_ci, _co) in zip(GEOMETRIES, ((512, 256), (256, 128), (128, 64))):
    for _L in sorted({1, 2, max(_M - 1, 1), 7}):
        TRANSPOSED.append((_ci, _co, _K, _u, _p, _mlo, _M, 2, _L, _Lo(_L), True))            # the real channel counts; Lin < M among them
    for _L in (1, 33, 200):
        TRANSPOSED.append((32, 16, _K, _u, _p, _mlo, _M, 3, _L, _Lo(_L), _u * 16 >= 64))      # reduced channels, B = 3
K_BELOW_U = [(32, 16, 3, 4, 0, 0, 1, 3, _L, 4 * _L - 1, True) for _L in (1, 33)]               # K < u: phase 3 has no tap


def _wn_conv(Cin, Cout, K, d, seed):
    torch.manual_seed(seed)
    l = nn.utils.weight_norm(nn.Conv1d(Cin, Cout, K, padding=d * (K - 1) // 2, dilation=d)).cuda()
    with torch.no_grad():
        l.bias.normal_(0, 0.1)
    return l


@pytest.mark.parametrize('L', CONV1D_L)
@pytest.mark.parametrize('Cin,Cout,K,d,wg_split', CONV1D)
def test_conv1d_layer_three_ways(Cin, Cout, K, d, wg_split, L):
    from ttscube_amd import _lib
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan.wbank import AmaxPool, WeightBank
    B, p = 2, d * (K - 1) // 2
    layer = _wn_conv(Cin, Cout, K, d, Cin + Cout + K + L)
    tc = A.TrainConv(Cin, Cout, K, padding=p, dilation=d)
    g = torch.Generator().manual_seed(K * 100 + L)
    x = torch.randn(B, Cin, L, generator=g)
    r = torch.randn(B, Cout, L, generator=g)
    dy = torch.randn(B, Cout, L, generator=g)
    w = (layer.weight_g * layer.weight_v / layer.weight_v.reshape(Cout, -1).norm(dim=1).view(-1, 1, 1)).detach()
    b = layer.bias.detach().clone()
    # which kernels: both legs of every generator layer are taken by ttsc_conv_train, on the 128-column tile at these sizes
    pf, pd = conv_plan(B, Cin, Cout, K, L, p, d), conv_plan(B, Cout, Cin, K, L, d * (K - 1) - p, d)
    assert (pf['MI'], pf['NJ'], pf['bucket']) == (2 if Cout >= 64 else 1, 1, K) and (pd['MI'], pd['NJ'], pd['bucket']) == (2 if Cin >= 64 else 1, 1, K)
    assert bool(_lib.lib().ttsc_conv_wgrad_split_supported(Cout, Cin, K, d)) == wg_split
    if wg_split:
        assert wgrad_plan(B, Cout, Cin, L, K, d)['groups'] == {3: (3,), 7: (5, 2), 11: (5, 5, 1)}[K]
    from oracle import gan_step_ref
    bank = WeightBank([(layer, Cin, Cout, K, 1, 1)])
    bank.prepare()
    w_bank = bank.weight(0).detach().clone().cpu()      # the effective weight the banked launches use: the native operand of that mode
    w64 = gan_step_ref.weight_norm(layer.weight_v, layer.weight_g).reshape(w.shape)
    _bound('conv1d banked: weight norm', w_bank, w64, w64.abs(), R.TAU_EXACT)
    for resid in (True, False):
        rr = r if resid else None
        ref_of = {}
        for key, wk in (('plain', w), ('bank', w_bank)):
            ref_of[key] = (R.layer(x, wk, b, rr, p, d, in_scale=SCALE, in_slope=SLOPE), R.layer(x, wk, b, rr, p, d, in_scale=SCALE, in_slope=SLOPE, absolute=True),
                           R.layer_vjp(x, wk, dy, p, d, in_scale=SCALE, in_slope=SLOPE), R.layer_vjp(x, wk, dy, p, d, in_scale=SCALE, in_slope=SLOPE, absolute=True))
        for mode in ('split', 'banked', 'exact'):
            y_ref, S_y, refs, Ss = ref_of['bank' if mode == 'banked' else 'plain']
            with _switches(split=mode != 'exact'):
                assert A._split_ok(Cin, Cout, K, d) == (mode != 'exact') and A._split_ok(Cout, Cin, K, d) == (mode != 'exact')
                tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
                label = 'conv1d %s:' % mode
                # three requests: a first call, a second one that reuses the handles, the maps and the bank's buffers, and the no-input-gradient
                # call (conv_pre on a detached mel)
                for request in ('first', 'again', 'no dx'):
                    want_dx = request != 'no dx'
                    rec = {}
                    xi = x.cuda().requires_grad_(want_dx)
                    ri = r.cuda().requires_grad_(True) if resid else None
                    if mode == 'banked':
                        AmaxPool.of(xi.device).reset()
                        bank.invalidate()
                        bank.prepare()
                        wb = bank.weight(0)
                        assert wb._ttsc_pack is not None and torch.equal(wb.detach().cpu(), w_bank)
                        wi = _Tap.apply(wb, rec, 'dw')
                        wi._ttsc_pack = wb._ttsc_pack
                        bi = _Tap.apply(layer.bias, rec, 'db')
                        leaves = [layer.weight_v, layer.weight_g, layer.bias]
                    else:
                        wi = w.clone().requires_grad_(True)
                        bi = b.clone().requires_grad_(True)
                        leaves = [wi, bi]
                    y = A.hip_conv(tc, xi, wi, bi, resid=ri, in_scale=SCALE, in_slope=SLOPE)
                    _bound(label + ' y', y, y_ref, S_y, tau)
                    ins = ([xi] if want_dx else []) + ([ri] if resid else [])
                    gs = torch.autograd.grad(y, ins + leaves, dy.cuda())
                    gw, gb = (rec['dw'], rec['db']) if mode == 'banked' else gs[len(ins):]
                    if want_dx:
                        _bound(label + ' dx', gs[0], refs[0], Ss[0], tau)
                    _bound(label + (' dw' if want_dx else ' dw (no dx)'), gw, refs[1], Ss[1], tau)
                    _bound(label + (' db' if want_dx else ' db (no dx)'), gb, refs[2], Ss[2], tau)
                    if resid:
                        assert torch.equal(gs[len(ins) - 1].cpu(), dy)      # dresid = dy, untouched


@pytest.mark.parametrize('Cin,Cout,K,u,p,m_lo,M,B,L,Lo,wg_split', TRANSPOSED)
def test_transposed_layer(Cin, Cout, K, u, p, m_lo, M, B, L, Lo, wg_split):
    from ttscube_amd import _lib
    from ttscube_amd.hifigan import autograd as A
    tc = A.TrainConv(Cin, Cout, K, stride=u, padding=p, transposed=True)
    assert tc.taps_t() == (m_lo, m_lo + M - 1, M)
    g = torch.Generator().manual_seed(K * 100 + u * 10 + L + Cin)
    x = torch.randn(B, Cin, L, generator=g)
    w = torch.randn(Cin, Cout, K, generator=g) / (Cin * K / u) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    assert R.out_len(L, K, p, 1, u, True) == Lo
    dy = torch.randn(B, Cout, Lo, generator=g)
    y_ref = R.layer(x, w, b, None, p, 1, u, True, SCALE, SLOPE)
    S_y = R.layer(x, w, b, None, p, 1, u, True, SCALE, SLOPE, absolute=True)
    refs = R.layer_vjp(x, w, dy, p, 1, u, True, SCALE, SLOPE)
    Ss = R.layer_vjp(x, w, dy, p, 1, u, True, SCALE, SLOPE, absolute=True)
    # the data gradient: a dense stride-1 convolution over u Cout rows, M taps, padding 0; the weight gradient: taps run backwards
    pd = conv_plan(B, u * Cout, Cin, M, L + M - 1, 0, 1)
    assert (pd['MI'], pd['NJ'], pd['bucket']) == (2 if Cin >= 64 else 1, 1, 3 if M <= 3 else 7) and pd['S'] == L + M - 1
    assert bool(_lib.lib().ttsc_conv_wgrad_split_supported(u * Cout, Cin, M, -1)) == wg_split
    if wg_split:
        assert wgrad_plan(B, u * Cout, Cin, L + M - 1, M, -1)['groups'] == {1: (1,), 4: (4,), 6: (5, 1)}[M]
    for mode in ('split', 'exact'):
        with _switches(split=mode != 'exact'):
            assert A._split_ok(u * Cout, Cin, M, 1) == (mode != 'exact')
            tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
            label = 'transposed %s:' % mode
            for _ in range(2):          # the second call reuses the handles and the index maps
                xi = x.cuda().requires_grad_(True)
                wi = w.cuda().requires_grad_(True)
                bi = b.cuda().requires_grad_(True)
                y = A.hip_conv(tc, xi, wi, bi, in_scale=SCALE, in_slope=SLOPE)
                _bound(label + ' y', y, y_ref, S_y, tau)
                gx, gw, gb = torch.autograd.grad(y, (xi, wi, bi), dy.cuda())
                _bound(label + ' dx', gx, refs[0], Ss[0], tau)
                _bound(label + ' dw', gw, refs[1], Ss[1], tau)
                _bound(label + ' db', gb, refs[2], Ss[2], tau)


@pytest.mark.parametrize('Cin,Cout,K,u,p,m_lo,M,B,L,Lo,wg_split', K_BELOW_U)
def test_transposed_backward_with_a_phase_without_taps(Cin, Cout, K, u, p, m_lo, M, B, L, Lo, wg_split):
    """K 3, u 4 (outside the config): the forward kernel refuses kernel_size < stride, loudly; the backward route (deinterleave, w_map, the dense
    data gradient, the backwards weight gradient, g_map) takes it — HipConvFn.backward is run on the context a forward call would have saved"""
    from ttscube_amd import _lib
    from ttscube_amd.hifigan import autograd as A
    tc = A.TrainConv(Cin, Cout, K, stride=u, padding=p, transposed=True)
    assert tc.taps_t() == (m_lo, m_lo + M - 1, M) and R.out_len(L, K, p, 1, u, True) == Lo
    g = torch.Generator().manual_seed(K * 100 + u * 10 + L + Cin)
    x = torch.randn(B, Cin, L, generator=g)
    w = torch.randn(Cin, Cout, K, generator=g) / (Cin * K / u) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(B, Cout, Lo, generator=g)
    with pytest.raises(_lib.TTSCError, match='kernel_size < stride'):
        A.hip_conv(tc, x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True), in_scale=SCALE, in_slope=SLOPE)
    refs = R.layer_vjp(x, w, dy, p, 1, u, True, SCALE, SLOPE)
    Ss = R.layer_vjp(x, w, dy, p, 1, u, True, SCALE, SLOPE, absolute=True)
    assert bool(_lib.lib().ttsc_conv_wgrad_split_supported(u * Cout, Cin, M, -1)) == wg_split
    for mode in ('split', 'exact'):
        with _switches(split=mode != 'exact'):
            assert A._split_ok(u * Cout, Cin, M, 1) == (mode != 'exact')
            tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
            ctx = A.backward_context(tc, x.cuda(), w.cuda(), SCALE, SLOPE)
            gx, gw, gb = A.HipConvFn.backward(ctx, dy.cuda())[:3]
            label = 'transposed K < u %s:' % mode
            _bound(label + ' dx', gx, refs[0], Ss[0], tau)
            _bound(label + ' dw', gw, refs[1], Ss[1], tau)
            _bound(label + ' db', gb, refs[2], Ss[2], tau)


def test_banked_chain_does_not_trust_a_range_word_after_a_write_or_a_reset():
    """two banked layers in a row.  The first leaves max |y1| in a pool word and tags y1 with it (tag_range); the second takes the word instead of
    reducing y1 (range_of) — unless y1 was written since (version rule) or the pool was reset (epoch rule).  Checked by VALUE: y1 is scaled by
    4096 in place (a stale word would put the fp16 range 12 bits too low: overflow), then the pool is reset (the word reads zero, or another
    call's maximum); and in the backward pass a second, 4096 times larger gradient is accumulated onto the data gradient the second layer
    tagged.  Every result is held to float64 at the operands the launches really read."""
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan.wbank import AmaxPool, WeightBank, range_of
    C_, L, B = 64, 300, 2
    l1, l2 = _wn_conv(C_, C_, 3, 1, 1), _wn_conv(C_, C_, 7, 3, 2)
    t1, t2 = A.TrainConv(C_, C_, 3, padding=1), A.TrainConv(C_, C_, 7, padding=9, dilation=3)
    bank = WeightBank([(l1, C_, C_, 3, 1, 1), (l2, C_, C_, 7, 1, 1)])
    pool = AmaxPool.of(torch.device('cuda', 0))
    pool.reset()
    bank.prepare()
    w1, w2 = bank.weight(0).detach().clone().cpu(), bank.weight(1).detach().clone().cpu()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C_, L, generator=g)
    kw1, kw2 = dict(padding=1, dilation=1), dict(padding=9, dilation=3, in_slope=SLOPE)
    xi = x.cuda().requires_grad_(True)
    y1 = A.hip_conv(t1, xi, bank.weight(0), l1.bias)
    assert range_of(y1) is not None
    _bound('banked chain: y1', y1, R.layer(x, w1, l1.bias, None, **kw1), R.layer(x, w1, l1.bias, None, absolute=True, **kw1), R.TAU_SPLIT)
    with torch.no_grad():
        y1.mul_(4096.0)
    y1c = y1.detach().clone().cpu()
    y2 = A.hip_conv(t2, y1, bank.weight(1), l2.bias, in_slope=SLOPE)
    _bound('banked chain: y2 after a write', y2, R.layer(y1c, w2, l2.bias, None, **kw2), R.layer(y1c, w2, l2.bias, None, absolute=True, **kw2), R.TAU_SPLIT)
    # backward: y1 receives the second layer's data gradient (tagged) and a second, much larger gradient
    seen = {}
    y1.register_hook(lambda g_: seen.__setitem__('dy1', g_.detach().clone()))
    dy2 = torch.randn(y2.shape, generator=g)
    big = torch.randn(y1.shape, generator=g) * 4096.0
    grads = torch.autograd.grad([y2, y1], [xi, l1.weight_v, l1.weight_g, l1.bias], [dy2.cuda(), big.cuda()])
    dy1 = seen['dy1'].cpu()
    ref2 = R.layer_vjp(y1c, w2, dy2, **kw2)
    S2 = R.layer_vjp(y1c, w2, dy2, absolute=True, **kw2)
    _bound('banked chain: accumulated dy1', dy1, ref2[0] + big.double(), S2[0] + big.double().abs(), R.TAU_SPLIT)
    ref1, S1 = R.layer_vjp(x, w1, dy1, **kw1), R.layer_vjp(x, w1, dy1, absolute=True, **kw1)
    _bound('banked chain: dx1 from the accumulated gradient', grads[0], ref1[0], S1[0], R.TAU_SPLIT)
    _bound('banked chain: db1 from the accumulated gradient', grads[3], ref1[2], S1[2], R.TAU_SPLIT)
    # epoch rule: after a reset y1's word belongs to the pool again (zeroed, then handed to the next call)
    pool.reset()
    assert range_of(y1) is None
    filler = A.hip_conv(t1, (x * 1e-3).cuda(), bank.weight(0), l1.bias)          # takes the first words of the fresh pool
    y2b = A.hip_conv(t2, y1.detach(), bank.weight(1), l2.bias, in_slope=SLOPE)
    y2c = A.hip_conv(t2, y1, bank.weight(1), l2.bias, in_slope=SLOPE)
    for name, t in (('detached', y2b), ('tagged in an earlier epoch', y2c)):
        _bound('banked chain: y2 after a reset, %s' % name, t, R.layer(y1c, w2, l2.bias, None, **kw2), R.layer(y1c, w2, l2.bias, None, absolute=True, **kw2), R.TAU_SPLIT)
    assert bool(torch.isfinite(filler).all())


# ---- the generator, teacher-forced per layer call ----------------------------------------------------------------------------------------------
def _capture(monkeypatch):
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan.wbank import pass_range
    calls = []
    orig = A.hip_conv

    def call(tc, x, w, b=None, resid=None, in_scale=1.0, in_slope=1.0):
        rec = dict(tc=tc, x=x.detach().clone(), w=w.detach().clone(), b=b.detach().clone(), resid=None if resid is None else resid.detach().clone(),
                   scale=in_scale, slope=in_slope, banked=getattr(w, '_ttsc_pack', None) is not None)
        xi = pass_range(x, _Tap.apply(x, rec, 'dx')) if x.requires_grad else x
        wi = _Tap.apply(w, rec, 'dw')
        if rec['banked']:
            wi._ttsc_pack = w._ttsc_pack
        bi = _Tap.apply(b, rec, 'db')
        y = orig(tc, xi, wi, bi, resid=resid, in_scale=in_scale, in_slope=in_slope)
        rec['y'] = y.detach().clone()
        y.register_hook(lambda g_: rec.__setitem__('dy', g_.detach().clone()))
        calls.append(rec)
        return y

    monkeypatch.setattr(A, 'hip_conv', call)
    return calls


def _check_calls(calls, tag, banked):
    from ttscube_amd.hifigan import autograd as A
    assert len(calls) == 78 and sum(c['banked'] for c in calls) == (74 if banked else 0)      # 74 stride-1 convolutions + 4 upsamplers
    tau = R.TAU_SPLIT if A.SPLIT_TRAIN else R.TAU_EXACT
    for rec in calls:
        tc = rec['tc']
        kw = dict(padding=tc.padding, dilation=tc.dilation, stride=tc.stride, transposed=tc.transposed, in_scale=rec['scale'], in_slope=rec['slope'])
        label = '%s %s %s:' % (tag, 'transposed' if tc.transposed else 'conv1d', 'banked' if rec['banked'] else 'plain')
        x, w, b, r = rec['x'].cpu(), rec['w'].cpu(), rec['b'].cpu(), None if rec['resid'] is None else rec['resid'].cpu()
        _bound(label + ' y', rec['y'], R.layer(x, w, b, r, **kw), R.layer(x, w, b, r, absolute=True, **kw), tau)
        assert 'dy' in rec and 'dw' in rec and 'db' in rec
        dy = rec['dy'].cpu()
        ref, S = R.layer_vjp(x, w, dy, **kw), R.layer_vjp(x, w, dy, absolute=True, **kw)
        if 'dx' in rec:
            _bound(label + ' dx', rec['dx'], ref[0], S[0], tau)
        _bound(label + ' dw', rec['dw'], ref[1], S[1], tau)
        _bound(label + ' db', rec['db'], ref[2], S[2], tau)


@pytest.mark.parametrize('use_bank', [True, False])
def test_generator_teacher_forced_per_layer_call(monkeypatch, use_bank):
    """one generator_forward_with_grad + backward per pass: two consecutive passes without AmaxPool.reset() (the words of the first pass are
    still tagged on nothing the second reads; the pool hands out fresh ones), then one more after a reset (epoch rule of range_of); the
    parameters move between the passes, as an optimizer would move them (version rule of the bank)"""
    from ttscube_amd.hifigan import autograd as A
    from ttscube_amd.hifigan.env import AttrDict
    from ttscube_amd.hifigan.models import Generator
    from ttscube_amd.hifigan.wbank import AmaxPool
    h = dict(hifigan_ref.CONFIG_V1, upsample_initial_channel=128)
    gen = Generator(AttrDict(h))
    gen.load_state_dict(hifigan_ref.synthetic_state_dict(h, seed=4))
    gen = gen.cuda()
    params = [p_ for p_ in gen.parameters() if p_.requires_grad]
    calls = _capture(monkeypatch)
    AmaxPool.of(torch.device('cuda', 0)).reset()
    with _switches(bank=use_bank):
        for step in range(3):
            if step == 2:
                AmaxPool.of(torch.device('cuda', 0)).reset()
            del calls[:]
            mel = hifigan_ref.synthetic_mel(2, 8, seed=6 + step).cuda()
            y = A.generator_forward_with_grad(gen, mel)
            tgt = torch.randn(y.shape, generator=torch.Generator().manual_seed(step)).cuda() * 0.3
            grads = torch.autograd.grad((y - tgt).abs().mean(), params)
            assert all(bool(torch.isfinite(g_).all()) for g_ in grads)
            _check_calls(calls, 'generator %s' % ('banked' if use_bank else 'per-launch'), use_bank)
            with torch.no_grad():        # the next pass sees other weights and, through them, other ranges in every layer
                for p_, g_ in zip(params, grads):
                    p_.add_(g_.sign() * (1e-3 * float(p_.abs().mean())))


def test_zz_report_measured():
    """prints the worst measured err / S per path (units of 2^-24)"""
    for k in sorted(MEASURED):
        print('MEASURED %-40s %.3f' % (k, MEASURED[k]))
