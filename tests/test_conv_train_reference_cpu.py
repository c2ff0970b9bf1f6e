"""CPU: the float64 statement of the training convolutions (tests/conv_train_reference.py) against torch autograd in float64; its float32
restatement (one term at a time) against the bounds the GPU tests assert, on every shape they use; the sensitivity of those bounds to the
mistakes such kernels make; and the index maps of the ConvTranspose1d backward (TrainConv.taps_t / maps_t / deinterleave) by brute force.

Measured here, worst float32 err / S per family in units of 2^-24 (bound 32 for the split kernels): see test_zz_report."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_train_reference as R
from oracle import hifigan_ref
from tests import test_conv_train_f64_gpu as G
from tests import test_gen_train_f64_gpu as GL

WORST = {}


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _ratio(got, ref, S):
    return float(((got.double() - ref).abs() / S.clamp(min=1e-300)).max())


CONV1D = [(3, 1, 1), (7, 3, 9), (11, 5, 25), (7, 3, 4), (7, 3, 14), (16, 1, 8), (1, 1, 0), (4, 1, 0)]       # K, dilation, padding
TRANSPOSED = [(16, 5, 5), (16, 3, 6), (4, 4, 0), (3, 4, 0)]                                                  # K, u, p  (the last: K < u)


@pytest.mark.parametrize('K,d,p', CONV1D)
@pytest.mark.parametrize('sc,sl,resid', [(1.0, 1.0, False), (1.0 / 3.0, 0.1, True)])
def test_conv1d_statement_equals_autograd(K, d, p, sc, sl, resid):
    g = torch.Generator().manual_seed(K * 10 + d)
    N, Ci, Co, L = 3, 5, 4, 70
    x = torch.randn(N, Ci, L, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(Co, Ci, K, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64).requires_grad_(True)
    Lo = R.out_len(L, K, p, d)
    r = torch.randn(N, Co, Lo, generator=g, dtype=torch.float64).requires_grad_(True) if resid else None
    scf, slf = R.f32(sc), R.f32(sl)
    y = F.conv1d(F.leaky_relu(x * scf, slf), w, b, padding=p, dilation=d)
    if resid:
        y = y + r
    assert _rel(R.layer(x, w, b, r, p, d, in_scale=sc, in_slope=sl), y.detach()) <= 1e-12
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad(y, [x, w, b] + ([r] if resid else []), dy)
    got = R.layer_vjp(x, w, dy, p, d, in_scale=sc, in_slope=sl)
    for a, want in zip(got, grads):
        assert _rel(a, want) <= 1e-12
    # the bare launches and the weight-gradient contract are the same statement in the kernels' terms
    assert _rel(R.launch_fwd(x, w, b, r, p, d, sc, sl), y.detach()) <= 1e-12
    if d * (K - 1) - p >= 0:
        assert _rel(R.launch_dgrad(dy, w, x, d * (K - 1) - p, d, sc, sl), grads[0]) <= 1e-12
    assert _rel(R.wgrad(dy, x, K, -p, d, sc, sl), grads[1]) <= 1e-12


@pytest.mark.parametrize('K,u,p', TRANSPOSED)
@pytest.mark.parametrize('L', [1, 2, 7, 33])
def test_transposed_statement_equals_autograd(K, u, p, L):
    g = torch.Generator().manual_seed(K * 10 + u + L)
    N, Ci, Co = 3, 5, 4
    x = torch.randn(N, Ci, L, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(Ci, Co, K, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64).requires_grad_(True)
    sc, sl = R.f32(1.0 / 3.0), R.f32(0.1)
    y = F.conv_transpose1d(F.leaky_relu(x * sc, sl), w, b, stride=u, padding=p)
    assert _rel(R.layer(x, w, b, None, p, 1, u, True, 1.0 / 3.0, 0.1), y.detach()) <= 1e-12
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad(y, [x, w, b], dy)
    for a, want in zip(R.layer_vjp(x, w, dy, p, 1, u, True, 1.0 / 3.0, 0.1), grads):
        assert _rel(a, want) <= 1e-12


def test_absolute_companion_dominates():
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.randn(2, 6, 40, generator=g), torch.randn(5, 6, 7, generator=g), torch.randn(5, generator=g)
    r = torch.randn(2, 5, 40, generator=g)
    assert bool((R.layer(x, w, b, r, 9, 3, absolute=True) >= R.layer(x, w, b, r, 9, 3).abs()).all())
    dy = torch.randn(2, 5, 40, generator=g)
    for s, v in zip(R.layer_vjp(x, w, dy, 9, 3, in_slope=0.1, absolute=True), R.layer_vjp(x, w, dy, 9, 3, in_slope=0.1)):
        assert bool((s >= v.abs() - 1e-15).all())


# ---- the float32 restatement stays inside the bounds of the GPU tests, on their shapes ------------------------------------------------------
@pytest.mark.parametrize('cid', G.CONV_IDS)
def test_float32_restatement_inside_the_bound_forward_and_data_gradient(cid):
    _, B, Cin, Cout, K, d, pad, Lin, expect = G.conv_case(cid)
    x, w, b, r = G.fwd_inputs(cid)
    ref = R.launch_fwd(x, w, b, r, pad, d, G.SCALE, G.SLOPE)
    S = R.launch_fwd(x, w, b, r, pad, d, G.SCALE, G.SLOPE, absolute=True)
    q = _ratio(R.launch_fwd_f32(x, w, b, r, pad, d, G.SCALE, G.SLOPE), ref, S)
    fam = '<%d,%d>' % expect[:2]
    WORST['forward ' + fam] = max(WORST.get('forward ' + fam, 0.0), q * 2 ** 24)
    assert q <= R.TAU_SPLIT / 2, q * 2 ** 24
    dy, wt, gate = G.dgrad_inputs(cid)
    ref = R.launch_dgrad(dy, wt, gate, pad, d, G.SCALE, G.SLOPE)
    S = R.launch_dgrad(dy, wt, gate, pad, d, G.SCALE, G.SLOPE, absolute=True)
    q = _ratio(R.launch_dgrad_f32(dy, wt, gate, pad, d, G.SCALE, G.SLOPE), ref, S)
    WORST['dgrad ' + fam] = max(WORST.get('dgrad ' + fam, 0.0), q * 2 ** 24)
    assert q <= R.TAU_SPLIT / 2, q * 2 ** 24


@pytest.mark.parametrize('wid', G.WG_IDS)
def test_float32_restatement_inside_the_bound_weight_gradient(wid):
    """strictly sequential over all N * LP positions of an element (the longest chain: 33 000 terms) — inside the split bound and, for the
    exact-fp32 kernel's bound 2^-21, the 64-position blocked order the tile kernels have"""
    _, N, A, Bc, LP, LQ, J, base, step, _ = G.WG_CASES[G.WG_IDS.index(wid)]
    P, Q = G.wg_inputs(wid)
    ref = R.wgrad(P, Q, J, base, step, G.SCALE, G.SLOPE)
    S = R.wgrad(P, Q, J, base, step, G.SCALE, G.SLOPE, absolute=True)
    q = _ratio(R.wgrad_f32(P, Q, J, base, step, G.SCALE, G.SLOPE), ref, S)
    WORST['wgrad sequential'] = max(WORST.get('wgrad sequential', 0.0), q * 2 ** 24)
    assert q <= R.TAU_SPLIT / 2, q * 2 ** 24
    if N * LP <= 3000:
        qb = _ratio(R.wgrad_f32(P, Q, J, base, step, G.SCALE, G.SLOPE, block=64), ref, S)
        WORST['wgrad blocked'] = max(WORST.get('wgrad blocked', 0.0), qb * 2 ** 24)
        assert qb <= R.TAU_EXACT, qb * 2 ** 24


# ---- ... and of the layer-level tests: hip_conv's layers and the reduced generator's, against the tau of EACH mode (2^-21 with SPLIT_TRAIN off) --
def _generator_layers(B=2, frames=8):
    """(Cin, Cout, K, dilation, u, p, transposed, B, L) of every convolution of the generator tests/test_gen_train_f64_gpu.py runs teacher-forced"""
    h = dict(hifigan_ref.CONFIG_V1, upsample_initial_channel=128)
    ch, L = h['upsample_initial_channel'], frames
    out = [(h['num_mels'], ch, 7, 1, 1, 3, False, B, L)]
    for u, k in zip(h['upsample_rates'], h['upsample_kernel_sizes']):
        out.append((ch, ch // 2, k, 1, u, (k - u) // 2, True, B, L))
        ch, L = ch // 2, R.out_len(L, k, (k - u) // 2, 1, u, True)
        for kr, ds in zip(h['resblock_kernel_sizes'], h['resblock_dilation_sizes']):
            out += [(ch, ch, kr, d, 1, d * (kr - 1) // 2, False, B, L) for d in sorted(set(ds) | {1})]
    out.append((ch, 1, 7, 1, 1, 3, False, B, L))
    return out


LAYER_SHAPES = sorted(set(
    [(Cin, Cout, K, d, 1, d * (K - 1) // 2, False, 2, L) for Cin, Cout, K, d, _ in GL.CONV1D for L in GL.CONV1D_L] +
    [(Cin, Cout, K, 1, u, p, True, B, L) for Cin, Cout, K, u, p, _, _, B, L, _, _ in GL.TRANSPOSED + GL.K_BELOW_U] + _generator_layers()))


@pytest.mark.parametrize('Cin,Cout,K,d,u,p,transposed,B,L', LAYER_SHAPES)
def test_float32_restatement_inside_the_bound_layers(Cin, Cout, K, d, u, p, transposed, B, L):
    """y, dx, dw of one layer in float32, one term at a time, on the shapes of the layer-level GPU tests: inside 2^-21 S, the bound of the
    exact-fp32 kernels (SPLIT_TRAIN off), hence inside 2^-19 S.  The Conv1d weight gradient is the long sum (B L positions): strictly
    sequential it is held to 2^-19 S (it measures up to 9.2 * 2^-24 S at 514 positions), and to 2^-21 S in the 64-position blocked order
    the weight-gradient kernels have (conv_wgrad.hip: partial sums per chunk, added in order)"""
    g = torch.Generator().manual_seed(Cin + 3 * Cout + K + L)
    x = torch.randn(B, Cin, L, generator=g)
    w = torch.randn((Cin, Cout, K) if transposed else (Cout, Cin, K), generator=g) / (Cin * K / u) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    Lo = R.out_len(L, K, p, d, u, transposed)
    r = torch.randn(B, Cout, Lo, generator=g) if not transposed else None
    dy = torch.randn(B, Cout, Lo, generator=g)
    kw = dict(padding=p, dilation=d, stride=u, transposed=transposed, in_scale=G.SCALE, in_slope=G.SLOPE)
    fam = 'layer transposed' if transposed else 'layer conv1d'
    qs = {'y': _ratio(R.layer_f32(x, w, b, r, **kw), R.layer(x, w, b, r, **kw), R.layer(x, w, b, r, absolute=True, **kw))}
    ref, S = R.layer_vjp(x, w, dy, **kw), R.layer_vjp(x, w, dy, absolute=True, **kw)
    got = R.layer_vjp_f32(x, w, dy, **kw)
    qs['dx'], qs['dw'] = _ratio(got[0], ref[0], S[0]), _ratio(got[1], ref[1], S[1])
    for k_, q in qs.items():
        WORST['%s %s' % (fam, k_)] = max(WORST.get('%s %s' % (fam, k_), 0.0), q * 2 ** 24)
    if not transposed:
        qs['dw blocked'] = _ratio(R.wgrad_f32(dy, x, K, -p, d, G.SCALE, G.SLOPE, block=64), ref[1], S[1])
        WORST[fam + ' dw blocked'] = max(WORST.get(fam + ' dw blocked', 0.0), qs['dw blocked'] * 2 ** 24)
    for k_, q in qs.items():
        assert q <= (R.TAU_SPLIT if (k_ == 'dw' and not transposed) else R.TAU_EXACT), (k_, q * 2 ** 24)


# ---- what the bounds catch ------------------------------------------------------------------------------------------------------------------
def _case():
    g = torch.Generator().manual_seed(11)
    N, Ci, Co, L, K, d = 3, 32, 48, 300, 7, 3
    p = d * (K - 1) // 2
    return dict(x=torch.randn(N, Ci, L, generator=g), w=torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5, b=torch.randn(Co, generator=g),
                r=torch.randn(N, Co, L, generator=g), dy=torch.randn(N, Co, L, generator=g), K=K, d=d, p=p)


def _caught(label, mutant, ref, S, tau=R.TAU_SPLIT):
    q = _ratio(mutant, ref, S)
    print('%-60s err / S = %.3g = %.0f x bound' % (label, q, q / tau))
    assert q >= 100 * tau, (label, q / tau)


def test_bounds_catch_a_dropped_tap_a_padding_shift_and_a_missing_bias():
    c = _case()
    x, w, b, r, dy, K, d, p = (c[k] for k in ('x', 'w', 'b', 'r', 'dy', 'K', 'd', 'p'))
    y = R.layer(x, w, b, r, p, d, in_scale=G.SCALE, in_slope=G.SLOPE)
    S = R.layer(x, w, b, r, p, d, in_scale=G.SCALE, in_slope=G.SLOPE, absolute=True)
    dx, dw, db, _ = R.layer_vjp(x, w, dy, p, d, in_scale=G.SCALE, in_slope=G.SLOPE)
    Sx, Sw, Sb, _ = R.layer_vjp(x, w, dy, p, d, in_scale=G.SCALE, in_slope=G.SLOPE, absolute=True)
    w0 = w.clone()
    w0[:, :, K - 1] = 0
    _caught('y: last tap dropped', R.layer(x, w0, b, r, p, d, in_scale=G.SCALE, in_slope=G.SLOPE), y, S)
    _caught('dx: last tap dropped', R.layer_vjp(x, w0, dy, p, d, in_scale=G.SCALE, in_slope=G.SLOPE)[0], dx, Sx)
    dw0 = dw.clone()
    dw0[:, :, K - 1] = 0
    _caught('dw: last tap dropped', dw0, dw, Sw)
    xs = torch.zeros_like(x)
    xs[:, :, 1:] = x[:, :, :-1]
    _caught('y: padding shifted by one sample', R.layer(xs, w, b, r, p, d, in_scale=G.SCALE, in_slope=G.SLOPE), y, S)
    _caught('dw: padding shifted by one sample', R.layer_vjp(xs, w, dy, p, d, in_scale=G.SCALE, in_slope=G.SLOPE)[1], dw, Sw)
    _caught('y: bias missing', R.layer(x, w, None, r, p, d, in_scale=G.SCALE, in_slope=G.SLOPE), y, S)
    _caught('y: residual missing', R.layer(x, w, b, None, p, d, in_scale=G.SCALE, in_slope=G.SLOPE), y, S)
    # the leaky-relu gate taken from the wrong side: slope where x > 0, one elsewhere
    gate = R.lrelu_grad(x.double(), R.f32(G.SLOPE))
    wrong = R.lrelu_grad(-x.double(), R.f32(G.SLOPE))
    _caught('dx: gate from the wrong side', dx / gate * wrong, dx, Sx)
    # the last position of batch item n read as the position before item n + 1 (a fold without the gap)
    a = R.lrelu(x.double() * R.f32(G.SCALE), R.f32(G.SLOPE))
    ap = R._pad(a, p, p)
    ap[1:, :, p - 1] = a[:-1, :, -1]
    leak = R._corr(ap, w.double(), d, x.shape[2]) + b.double().view(1, -1, 1) + r.double()
    _caught('y: last position of item n leaks into item n + 1', leak, y, S)
    _caught('dw: ... the same leak', R._corr_w(ap, dy.double(), K, d), dw, Sw)
    # two columns of one tile swapped
    ysw = y.clone()
    ysw[0, :, [4, 5]] = y[0, :, [5, 4]]
    _caught('y: two columns swapped', ysw, y, S)


def test_bounds_catch_swapped_phases_and_a_shifted_tap_map():
    g = torch.Generator().manual_seed(12)
    Ci, Co, K, u, p, L = 8, 6, 16, 5, 5, 40
    x = torch.randn(2, Ci, L, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, K, generator=g, dtype=torch.float64) / (Ci * K) ** 0.5
    dy = torch.randn(2, Co, R.out_len(L, K, p, 1, u, True), generator=g, dtype=torch.float64)
    dx, dw, _, _ = R.layer_vjp(x, w, dy, p, 1, u, True)
    Sx, Sw, _, _ = R.layer_vjp(x, w, dy, p, 1, u, True, absolute=True)
    tc = R.bare_train_conv(Ci, Co, K, u, p)
    gx, gw = R.transposed_backward_by_maps(tc, x, w, dy)
    assert _rel(gx, dx) <= 1e-12 and _rel(gw, dw) <= 1e-12
    orig = tc.deinterleave

    def swapped(dy_, Lin):
        out = orig(dy_, Lin)
        out[:, :2 * Co] = torch.cat([out[:, Co:2 * Co], out[:, :Co]], dim=1)
        return out
    tc.deinterleave = swapped
    gx, gw = R.transposed_backward_by_maps(tc, x, w, dy)
    _caught('transposed dx: phases 0 and 1 swapped', gx, dx, Sx)
    _caught('transposed dw: phases 0 and 1 swapped', gw, dw, Sw)
    tc = R.bare_train_conv(Ci, Co, K, u, p)
    w_map, g_map = tc.maps_t(torch.device('cpu'))
    m_lo, _, M = tc.taps_t()
    k = torch.arange(K)
    jj = (k - p - (k - p) % u) // u - (m_lo + 1)                       # g_map with m_lo off by one
    bad = g_map - ((k - p - (k - p) % u) // u - m_lo).view(1, 1, K) + jj.clamp(min=0).view(1, 1, K)
    tc._maps = (w_map, bad)
    _caught('transposed dw: g_map with m_lo off by one', R.transposed_backward_by_maps(tc, x, w, dy)[1], dw, Sw)


# ---- the index maps by brute force ----------------------------------------------------------------------------------------------------------
def test_transposed_index_maps_by_brute_force():
    """K 1..17, u 1..8, p 0..K-1, Lin 1, 2, 3, 7: deinterleave + w_map as a dense stride-1 convolution give torch's dx, the correlation
    G[r Co + co, ci, j] = sum_i x[ci, i] dyP[r Co + co, i + j] through g_map gives torch's dw, in float64 to 1e-10"""
    g = torch.Generator().manual_seed(5)
    Ci, Co, N = 3, 2, 2
    n = 0
    for K in range(1, 18):
        for u in range(1, 9):
            for p in range(0, K):
                tc = R.bare_train_conv(Ci, Co, K, u, p)
                for L in (1, 2, 3, 7):
                    Lo = R.out_len(L, K, p, 1, u, True)
                    if Lo < 1:
                        continue
                    x = torch.randn(N, Ci, L, generator=g, dtype=torch.float64).requires_grad_(True)
                    w = torch.randn(Ci, Co, K, generator=g, dtype=torch.float64).requires_grad_(True)
                    dy = torch.randn(N, Co, Lo, generator=g, dtype=torch.float64)
                    dx, dw = torch.autograd.grad(F.conv_transpose1d(x, w, stride=u, padding=p), (x, w), dy)
                    gx, gw = R.transposed_backward_by_maps(tc, x.detach(), w.detach(), dy)
                    assert float((gx - dx).abs().max()) <= 1e-10 and float((gw - dw).abs().max()) <= 1e-10, (K, u, p, L)
                    n += 1
    assert n == 3794, n


def test_zz_report():
    for k in sorted(WORST):
        print('WORST float32 %-28s %.2f * 2^-24 S' % (k, WORST[k]))
