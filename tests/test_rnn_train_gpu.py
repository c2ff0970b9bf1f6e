"""GPU: the GRU and LSTM training recurrences (gru.hip; lstm.hip ttsc_lstm_seq_forward_train / ttsc_lstm_seq_backward) against the float64
oracle (oracle/rnn_train_ref.py) on every dispatch path, at the production horizons.

Every case asks the dispatch query (ttsc_gru_train_path / ttsc_lstm_train_path) which kernels it reaches and asserts the intended path; the
batch sizes are derived from the device's CU count.  Two levels of check:
  kernel level  the C entry points on identical xg rows, every output buffer NaN-filled before the launch; y, the saved activations and the
                gate gradients of chosen utterances against the oracle per window of <= 1 000 steps
  layer level   gru_forward_train / lstm_forward_train + autograd: y, dx and every parameter gradient against the oracle
Bound: err_kernel <= 4 * err_yardstick + 1e-6 * max|ref| + ACT_ABS, both max-abs errors against the float64 oracle per (utterance, window) or
per weight tensor; the yardstick is the same oracle run in float32.  ACT_ABS = 2^-23: ttsc_tanhf (include/ttscube_math.h) evaluates
1 - 2/(exp(2|x|) + 1) for |x| >= 1/16, so its error is ~1 ulp of 1.0 in ABSOLUTE terms; where outputs are << 1 (a one-step sequence of the
H = 512 stack: |y| ~ 0.03) that alone is ~2e-6 relative, above the 1e-6 * max|ref| term (measured: 6.1e-8 against a 3.1e-8 floor)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import rnn_train_ref as R

FACTOR, FLOOR, WIN = 4.0, 1e-6, 1000
ACT_ABS = 2.0 ** -23
RATIOS = {}    # path label -> worst err_kernel / err_yardstick seen
TIMINGS = {}

GRU_SEQ, GRU_SPLIT, GRU_SPLIT_RES = 0, 1, 2                                                   # include/ttscube_hip.h TTSC_GRU_PATH_*
L_SEQ, L_SPLIT, L_SPLIT_RES, L_SPLIT_RES_NB, L_RESIDENT = 0, 1, 2, 3, 4                       # TTSC_LSTM_PATH_*
GRU_NAMES = {GRU_SEQ: 'seq', GRU_SPLIT: 'split', GRU_SPLIT_RES: 'split_res'}
LSTM_NAMES = {L_SEQ: 'seq', L_SPLIT: 'split', L_SPLIT_RES: 'split_res', L_SPLIT_RES_NB: 'split_res_nb', L_RESIDENT: 'resident'}


def _L():
    from ttscube_amd import _lib
    return _lib.lib()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def gru_path(B, H, backward=0):
    info = (C.c_int32 * 3)()
    p = _L().ttsc_gru_train_path(B, H, backward, info)
    assert p >= 0
    return p, tuple(info)


def lstm_path(B, ndir, H, backward=0):
    info = (C.c_int32 * 3)()
    p = _L().ttsc_lstm_train_path(B, ndir, H, backward, info)
    assert p >= 0
    return p, tuple(info)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(b) else 0.0


def _bound(label, what, got, ref, yard):
    """one (utterance, window) or one tensor: returns a failure string or None, records the kernel / yardstick ratio"""
    ek, ey = _err(got, ref), _err(yard, ref)
    scale = float(np.abs(ref).max()) if np.size(ref) else 0.0
    floor = FLOOR * scale + ACT_ABS
    ok = np.all(np.isfinite(got)) and ek <= FACTOR * ey + floor
    ratio = ek / max(ey, FLOOR * scale, 1e-30)
    RATIOS[label] = max(RATIOS.get(label, 0.0), ratio)
    return None if ok else '%s %s: err %.3e > 4 * yardstick %.3e + %.3e' % (label, what, ek, ey, floor)


def _windows(label, what, got, ref, yard, fails):
    """got / ref / yard: [T, ...] of one utterance, checked per window of WIN steps"""
    for t0 in range(0, ref.shape[0], WIN):
        f = _bound(label, '%s[t %d:%d]' % (what, t0, t0 + WIN), got[t0:t0 + WIN], ref[t0:t0 + WIN], yard[t0:t0 + WIN])
        if f:
            fails.append(f)


def _pick(B, extra=()):
    return sorted({i for i in (0, 1, 3, B // 2, B - 2, B - 1) + tuple(extra) if 0 <= i < B})


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    if RATIOS:
        print('\nkernel / float32-yardstick max-abs error ratio per path (bound: 4):')
        for k in sorted(RATIOS):
            print('  %-48s %.3f' % (k, RATIOS[k]))
    for k, v in TIMINGS.items():
        print('  timing %-40s %s' % (k, v))


# ---------------------------------------------------------------------------------------------------------------------------- GRU
def _gru_inputs(B, T, H, seed, h0=False):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    k = H ** -0.5
    whh = (torch.rand(3 * H, H, device='cuda', generator=g) * 2 - 1) * k
    bhh = (torch.rand(3 * H, device='cuda', generator=g) * 2 - 1) * k
    xg = torch.randn(B, T, 3 * H, device='cuda', generator=g) * 0.8
    dy = torch.randn(B, T, H, device='cuda', generator=g) * 0.1
    h0t = (torch.rand(B, H, device='cuda', generator=g) * 2 - 1) * 0.9 if h0 else None
    return xg, whh, bhh, dy, h0t


def _gru_pack(whh, transpose):
    from ttscube_amd import _lib
    H = whh.shape[1]
    out = torch.empty(3 * H * H, device='cuda')
    _lib.check(_L().ttsc_gru_pack_whh_device(_lib.dev_ptr(whh), H, transpose, _lib.dev_ptr(out), None), 'pack')
    return out


def gru_kernel_run(xg, whh, bhh, dy, h0=None):
    """ttsc_gru_seq_forward + ttsc_gru_seq_backward on NaN-filled outputs -> y, saved, dgi, dgh (device)"""
    from ttscube_amd import _lib
    B, T, H3 = xg.shape
    H = H3 // 3
    nan = float('nan')
    y = torch.full((B, T, H), nan, device='cuda')
    saved = torch.full((B, T, 4 * H), nan, device='cuda')
    dgi = torch.full((B, T, 3 * H), nan, device='cuda')
    dgh = torch.full((B, T, 3 * H), nan, device='cuda')
    h0p = _lib.dev_ptr(h0) if h0 is not None else None
    _lib.check(_L().ttsc_gru_seq_forward(_lib.dev_ptr(xg), _lib.dev_ptr(_gru_pack(whh, 0)), _lib.dev_ptr(bhh), _lib.dev_ptr(y), _lib.dev_ptr(saved),
                                         h0p, B, T, H, None), 'ttsc_gru_seq_forward')
    assert _L().ttsc_gru_split_status() == 0
    _lib.check(_L().ttsc_gru_seq_backward(_lib.dev_ptr(dy), _lib.dev_ptr(saved), _lib.dev_ptr(y), h0p, _lib.dev_ptr(_gru_pack(whh, 1)),
                                          _lib.dev_ptr(dgi), _lib.dev_ptr(dgh), B, T, H, None), 'ttsc_gru_seq_backward')
    assert _L().ttsc_gru_split_status() == 0
    torch.cuda.synchronize()
    for name, t in (('y', y), ('saved', saved), ('dgi', dgi), ('dgh', dgh)):   # every element written (NaN fill)
        assert bool(torch.isfinite(t).all()), '%s has unwritten / non-finite elements' % name
    return y, saved, dgi, dgh


def gru_check_against_oracle(label, xg, whh, bhh, dy, h0, outs, sel, w_ih=None, dx=None, chain=False):
    """per selected utterance and window: y, saved, dgi, dgh (and dx = dgi W_ih) against the float64 oracle with the float32 yardstick
    (chain: the yardstick sums W_hh products as one k-ordered chain, as the single-workgroup kernels do)"""
    y, saved, dgi, dgh = outs
    idx = torch.tensor(sel, device='cuda')
    a = [t.index_select(0, idx).cpu().numpy() for t in (xg, dy)]
    g = {k: t.index_select(0, idx).cpu().numpy() for k, t in (('y', y), ('saved', saved), ('dgi', dgi), ('dgh', dgh))}
    if dx is not None:
        g['dx'] = dx.index_select(0, idx).cpu().numpy()
        wih = w_ih.cpu().numpy()
    h0n = h0.index_select(0, idx).cpu().numpy() if h0 is not None else None
    W, Bh = whh.cpu().numpy(), bhh.cpu().numpy()
    fails = []
    it64 = R.gru_windows(a[0], W, Bh, a[1], h0n, np.float64, WIN)
    it32 = R.gru_windows(a[0], W, Bh, a[1], h0n, np.float32, WIN, chain=chain)
    for e64, e32 in zip(it64, it32):
        if e64[0] == 'fwd':
            _, t0, t1, y64, s64 = e64
            parts = (('y', y64, e32[3]), ('saved', s64, e32[4]))
        elif e64[0] == 'bwd':
            _, t0, t1, gi64, gh64, _ = e64
            parts = (('dgi', gi64, e32[3]), ('dgh', gh64, e32[4]))
            if dx is not None:
                parts += (('dx', gi64 @ wih.astype(np.float64), e32[3] @ wih),)
        else:
            continue
        for name, r64, r32 in parts:
            for i, u in enumerate(sel):
                f = _bound(label + (' fwd' if name in ('y', 'saved') else ' bwd'), '%s u%d [t %d:%d]' % (name, u, t0, t1),
                           g[name][i, t0:t1], r64[i], r32[i])
                if f:
                    fails.append(f)
    assert not fails, fails[:6]


def _gru_cases():
    c = _cus()
    return [
        # label, H, B, T, h0, path, G
        ('seq H64', 64, 4, 500, True, GRU_SEQ, 1),
        ('seq H36', 36, 3, 200, False, GRU_SEQ, 1),
        ('seq H100', 100, 3, 200, False, GRU_SEQ, 1),
        ('seq H512 many', 512, c * 25 // 32, 50, False, GRU_SEQ, 1),
        ('split G2 H128', 128, 8, 300, False, GRU_SPLIT, 2),
        ('split G2 H256', 256, c * 25 // 64, 100, False, GRU_SPLIT, 2),
        ('split G4 H512 B17', 512, c // 16 + 1, 100, False, GRU_SPLIT, 4),
        ('split G4 H512 B40', 512, c * 5 // 32, 100, False, GRU_SPLIT, 4),
        ('split_res G4 H256 B8', 256, 8, 300, False, GRU_SPLIT_RES, 4),
        ('split_res G4 H256 Bmax', 256, c // 4, 100, False, GRU_SPLIT_RES, 4),
        ('split_res G16 H512 B1', 512, 1, 500, True, GRU_SPLIT_RES, 16),
        ('split_res G16 H512 Bmax', 512, c // 16, 300, False, GRU_SPLIT_RES, 16),
    ]


_GRU_IDS = ['seq H64', 'seq H36', 'seq H100', 'seq H512 many', 'split G2 H128', 'split G2 H256', 'split G4 H512 B17', 'split G4 H512 B40',
            'split_res G4 H256 B8', 'split_res G4 H256 Bmax', 'split_res G16 H512 B1', 'split_res G16 H512 Bmax']


@pytest.mark.gpu
@pytest.mark.parametrize('tsel', ['long', 1, 2])
@pytest.mark.parametrize('case', _GRU_IDS)
def test_gru_kernels_match_float64_oracle(case, tsel):
    label, H, B, T, h0, path, G = [c for c in _gru_cases() if c[0] == case][0]
    T = T if tsel == 'long' else tsel
    for bwd in (0, 1):
        assert gru_path(B, H, bwd) == (path, (G, 1, 1)), (case, B, H, gru_path(B, H, bwd))
    xg, whh, bhh, dy, h0t = _gru_inputs(B, T, H, seed=H * 7 + B, h0=h0)
    outs = gru_kernel_run(xg, whh, bhh, dy, h0t)
    # gru_seq_kernel / gru_bwd_kernel sum W_hh h and W_hh^T dGh as ONE fma chain of H / 3H terms per unit: at H = 512 that rounds up to 13x more
    # than numpy's blocked float32 product (measured, T = 50), so their yardstick is float32 with the same k-ordered chain
    chain = path == GRU_SEQ
    gru_check_against_oracle('gru %s G=%d H=%d%s' % (GRU_NAMES[path], G, H, ' (chain yardstick)' if chain else ''), xg, whh, bhh, dy, h0t, outs,
                             _pick(B), chain=chain)


@pytest.mark.gpu
def test_gru_same_path_launches_are_bit_identical():
    """the same G on the same path gives the same bits per utterance whatever the batch: resident B = 1 vs cus/16, split G = 4 B = cus/16 + 1 vs
    5 cus / 32 (forward and backward)"""
    c = _cus()
    for H, Ba, Bb, path, G, T in ((512, 1, c // 16, GRU_SPLIT_RES, 16, 200), (512, c // 16 + 1, c * 5 // 32, GRU_SPLIT, 4, 120)):
        assert gru_path(Ba, H) == (path, (G, 1, 1)) and gru_path(Bb, H) == (path, (G, 1, 1))
        xg, whh, bhh, dy, _ = _gru_inputs(Bb, T, H, seed=99 + Bb)
        big = gru_kernel_run(xg, whh, bhh, dy)
        small = gru_kernel_run(xg[:Ba].contiguous(), whh, bhh, dy[:Ba].contiguous())
        for name, s_, b_ in zip(('y', 'saved', 'dgi', 'dgh'), small, big):
            assert torch.equal(s_, b_[:Ba]), (H, Ba, Bb, name)


def _gru_layer_check(label, H, B, T, I, seed):
    """gru_forward_train + autograd against the oracle: y, dx per (utterance, window); weight / bias gradients per tensor"""
    from ttscube_amd.networks.gru_autograd import gru_forward_train
    torch.manual_seed(seed)
    m = torch.nn.GRU(I, H, batch_first=True).cuda()
    x = torch.randn(B, T, I, device='cuda', requires_grad=True)
    dy = torch.randn(B, T, H, device='cuda') * 0.1
    y = gru_forward_train(m, x)
    assert _L().ttsc_gru_split_status() == 0
    (y * dy).sum().backward()
    assert _L().ttsc_gru_split_status() == 0
    p = {k: v.detach().cpu().numpy() for k, v in m.named_parameters()}
    args = (x.detach().cpu().numpy(), p['weight_ih_l0'], p['weight_hh_l0'], p['bias_ih_l0'], p['bias_hh_l0'], dy.cpu().numpy())
    t0 = time.time()
    r64 = R.gru_layer_grads(*args, dtype=np.float64)
    r32 = R.gru_layer_grads(*args, dtype=np.float32)
    TIMINGS['oracle %s' % label] = '%.1f s (float64 + float32, %d x %d steps)' % (time.time() - t0, B, T)
    fails = []
    yk, dxk = y.detach().cpu().numpy(), x.grad.cpu().numpy()
    for u in range(B):
        _windows(label + ' layer', 'y u%d' % u, yk[u], r64['y'][u], r32['y'][u], fails)
        _windows(label + ' layer', 'dx u%d' % u, dxk[u], r64['dx'][u], r32['dx'][u], fails)
    for k, v in m.named_parameters():
        f = _bound(label + ' layer weights', k, v.grad.cpu().numpy(), r64[k], r32[k])
        if f:
            fails.append(f)
    assert not fails, fails[:6]


@pytest.mark.gpu
@pytest.mark.parametrize('tsel', ['long', 1])
@pytest.mark.parametrize('case', ['seq', 'split G2', 'split G4', 'split_res G4'])
def test_gru_layer_gradients_match_float64_oracle(case, tsel):
    """T = 1 is a regression case: the dW_hh GEMM's row shift needs a period above 1, so one-step sequences raised in the backward"""
    c = _cus()
    H, B, T, path, G = {'seq': (64, 4, 500, GRU_SEQ, 1), 'split G2': (256, c * 25 // 64, 60, GRU_SPLIT, 2),
                        'split G4': (512, c // 16 + 1, 60, GRU_SPLIT, 4), 'split_res G4': (256, 8, 200, GRU_SPLIT_RES, 4)}[case]
    T = T if tsel == 'long' else 1
    assert gru_path(B, H) == (path, (G, 1, 1))
    _gru_layer_check('gru %s G=%d H=%d' % (GRU_NAMES[path], G, H), H, B, T, 32, seed=11)


@pytest.mark.gpu
def test_gru_lr_net_horizon_2400_steps():
    """the vocoder's lr net: H = 512, B = 16, T = 2 400 on the resident path — y, dx and the weight gradients (split-K GEMM over 38 400 rows)"""
    c = _cus()
    B = min(16, c // 16)
    assert gru_path(B, 512) == (GRU_SPLIT_RES, (16, 1, 1))
    t0 = time.time()
    _gru_layer_check('gru split_res G=16 H=512 lr', 512, B, 2400, 32, seed=5)
    TIMINGS['lr net B=%d T=2400 total' % B] = '%.1f s' % (time.time() - t0)


@pytest.mark.gpu
def test_gru_hr_net_horizon_24000_steps():
    """the vocoder's hr net: H = 512, B = 16, T = 24 000 with real dy, all 16 utterances launched; y, saved, dgi, dgh and dx = dgi W_ih of
    utterances 0, 9, 15 against the oracle per 1 000-step window"""
    from ttscube_amd.hip_layers import gemm_hip
    c = _cus()
    B, T, H, I = min(16, c // 16), 24000, 512, 32
    assert gru_path(B, H) == (GRU_SPLIT_RES, (16, 1, 1)) and gru_path(B, H, 1) == (GRU_SPLIT_RES, (16, 1, 1))
    xg, whh, bhh, dy, _ = _gru_inputs(B, T, H, seed=2024)
    w_ih = torch.randn(3 * H, I, device='cuda') * (H ** -0.5)
    t0 = time.time()
    outs = gru_kernel_run(xg, whh, bhh, dy)
    dx = gemm_hip(outs[2].reshape(B * T, 3 * H), w_ih).reshape(B, T, I)
    torch.cuda.synchronize()
    t1 = time.time()
    gru_check_against_oracle('gru split_res G=16 H=512 hr', xg, whh, bhh, dy, None, outs, [u for u in (0, 9, 15) if u < B], w_ih=w_ih, dx=dx)
    TIMINGS['hr net B=%d T=24000' % B] = 'GPU %.1f s, oracle + compare %.1f s' % (t1 - t0, time.time() - t1)


# ---------------------------------------------------------------------------------------------------------------------------- LSTM
def _lstm_cases():
    c = _cus()
    return {
        # label: H, ndir, B, T, group size, (fwd path, (G, NB, launches)), (bwd path, G)
        'resident H64': (64, 2, c // 2, 600, 0, (L_RESIDENT, (1, 1, 1)), (L_RESIDENT, 1)),
        'resident H128': (128, 2, c // 2, 600, 0, (L_RESIDENT, (1, 1, 1)), (L_RESIDENT, 1)),
        'split_res H256 b16': (256, 2, c // 16, 300, 0, (L_SPLIT_RES, (4, 1, 1)), (L_SPLIT_RES, 4)),
        'nb4 H256 b128': (256, 2, c // 2, 200, 0, (L_SPLIT_RES_NB, (4, 4, 1)), (L_SEQ, 1)),
        'nb2 H256': (256, 2, c * 3 // 16, 200, 0, (L_SPLIT_RES_NB, (4, 2, 1)), (L_SPLIT, 2)),
        'nb4 2 launches H512': (512, 1, c * 25 // 64, 100, 0, (L_SPLIT_RES_NB, (16, 4, 2)), (L_SPLIT, 2)),
        'nb8 H512': (512, 1, c // 16, 100, 8, (L_SPLIT_RES_NB, (16, 8, 1)), (L_SPLIT, 4)),
        'seq2 H256': (256, 2, max(400, 3 * c // 2 + 4), 20, 0, (L_SEQ, (1, 2, 1)), (L_SEQ, 1)),
    }


class _group_size:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        if self.n:
            from ttscube_amd import _lib
            self.cm = _lib.lstm_group_size(self.n)
            self.cm.__enter__()

    def __exit__(self, *e):
        if self.n:
            self.cm.__exit__(*e)


def _lstm_inputs(B, T, H, nd, seed):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    k = H ** -0.5
    whh = (torch.rand(nd, 4 * H, H, device='cuda', generator=g) * 2 - 1) * k
    xg = torch.randn(B, T, nd * 4 * H, device='cuda', generator=g) * 0.8
    dy = torch.randn(B, T, nd * H, device='cuda', generator=g) * 0.1
    return xg, whh, dy


def _lstm_pack(whh, transpose):
    from ttscube_amd import _lib
    nd, H4, H = whh.shape
    out = torch.empty(nd * H4 * H, device='cuda')
    _lib.check(_L().ttsc_lstm_pack_whh_device(_lib.dev_ptr(whh), nd, H, transpose, _lib.dev_ptr(out), None), 'pack')
    return out


def lstm_kernel_run(xg, whh, dy, backward=True):
    """ttsc_lstm_seq_forward_train (+ ttsc_lstm_seq_backward) on NaN-filled outputs -> y, gates, c, dG (device)"""
    from ttscube_amd import _lib
    B, T, _ = xg.shape
    nd, H4, H = whh.shape
    nan = float('nan')
    y = torch.full((B, T, nd * H), nan, device='cuda')
    gates = torch.full((B, T, nd * H4), nan, device='cuda')
    cs = torch.full((B, T, nd * H), nan, device='cuda')
    _lib.check(_L().ttsc_lstm_seq_forward_train(_lib.dev_ptr(xg), _lib.dev_ptr(_lstm_pack(whh, 0)), _lib.dev_ptr(y), None, B, T, H, nd, nd * H, 0,
                                                _lib.dev_ptr(gates), _lib.dev_ptr(cs), None), 'ttsc_lstm_seq_forward_train')
    assert _L().ttsc_lstm_split_status() == 0
    outs = [y, gates, cs]
    if backward:
        dG = torch.full((B, T, nd * H4), nan, device='cuda')
        _lib.check(_L().ttsc_lstm_seq_backward(_lib.dev_ptr(dy), _lib.dev_ptr(gates), _lib.dev_ptr(cs), _lib.dev_ptr(_lstm_pack(whh, 1)),
                                               _lib.dev_ptr(dG), None, B, T, H, nd, nd * H, 0, None), 'ttsc_lstm_seq_backward')
        assert _L().ttsc_lstm_split_status() == 0
        outs.append(dG)
    torch.cuda.synchronize()
    for name, t in zip(('y', 'gates', 'c', 'dG'), outs):
        assert bool(torch.isfinite(t).all()), '%s has unwritten / non-finite elements' % name
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('tsel', ['long', 1])
@pytest.mark.parametrize('case', list(['resident H64', 'resident H128', 'split_res H256 b16', 'nb4 H256 b128', 'nb2 H256', 'nb4 2 launches H512',
                                       'nb8 H512', 'seq2 H256']))
def test_lstm_kernels_match_float64_oracle(case, tsel):
    H, nd, B, T, gs, fwd, bwd = _lstm_cases()[case]
    T = T if tsel == 'long' else 1
    with _group_size(gs):
        assert lstm_path(B, nd, H, 0) == fwd, (case, lstm_path(B, nd, H, 0))
        assert lstm_path(B, nd, H, 1)[0] == bwd[0] and lstm_path(B, nd, H, 1)[1][0] == bwd[1], (case, lstm_path(B, nd, H, 1))
        xg, whh, dy = _lstm_inputs(B, T, H, nd, seed=H + B + T)
        y, gates, cs, dG = lstm_kernel_run(xg, whh, dy)
    lf = 'lstm fwd %s G=%d NB=%d H=%d' % (LSTM_NAMES[fwd[0]], fwd[1][0], fwd[1][1], H)
    lb = 'lstm bwd %s G=%d H=%d' % (LSTM_NAMES[bwd[0]], bwd[1], H)
    sel = _pick(B, (B // 4, 3 * B // 4))
    idx = torch.tensor(sel, device='cuda')
    xs, ds = xg.index_select(0, idx).cpu().numpy(), dy.index_select(0, idx).cpu().numpy()
    W = whh.cpu().numpy()
    got = [t.index_select(0, idx).cpu().numpy() for t in (y, gates, cs, dG)]
    ref, yard = {}, {}
    for dt, out in ((np.float64, ref), (np.float32, yard)):
        out['y'], out['gates'], out['c'] = R.lstm_layer_forward(xs, W, dt)
        out['dG'] = R.lstm_layer_backward(ds, out['gates'], out['c'], W, dt)
    fails = []
    for i, u in enumerate(sel):
        for name, g_ in zip(('y', 'gates', 'c', 'dG'), got):
            _windows(lb if name == 'dG' else lf, '%s u%d' % (name, u), g_[i], ref[name][i], yard[name][i], fails)
    assert not fails, fails[:6]


@pytest.mark.gpu
def test_lstm_nb_forward_is_bit_identical_to_nb1():
    """lstm_forward_impl: the nb kernels do per utterance the NB = 1 arithmetic — utterances 0..3 of a B = 4 launch (split_res, NB = 1) and of a
    B = cus/2 launch (nb<4>) have the same bits (forward only: the two backward launches take different paths)"""
    c = _cus()
    H, nd, T = 256, 2, 150
    Bb = c // 2
    assert lstm_path(4, nd, H) == (L_SPLIT_RES, (4, 1, 1))
    assert lstm_path(Bb, nd, H) == (L_SPLIT_RES_NB, (4, 4, 1))
    xg, whh, dy = _lstm_inputs(Bb, T, H, nd, seed=77)
    big = lstm_kernel_run(xg, whh, dy, backward=False)
    small = lstm_kernel_run(xg[:4].contiguous(), whh, dy[:4].contiguous(), backward=False)
    for name, s_, b_ in zip(('y', 'gates', 'c'), small, big):
        assert torch.equal(s_, b_[:4]), name


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1, 24])
@pytest.mark.parametrize('case', ['resident H64', 'resident H128', 'split_res H256 b16', 'nb4 H256 b128', 'nb2 H256', 'nb4 2 launches H512',
                                  'nb8 H512', 'seq2 H256'])
def test_lstm_two_layer_stack_gradients_match_float64_oracle(case, T):
    """lstm_forward_train over a 2-layer stack + autograd: y, dx and every parameter gradient against the oracle (layer 1 reaches the case's
    path; layer 2 takes ndir*H inputs).  T = 1 is a regression case: the dW_hh GEMM's row shift needs a period above 1, so one-step sequences
    raised in the backward"""
    from ttscube_amd.networks.lstm_autograd import lstm_forward_train
    H, nd, B, _, gs, fwd, bwd = _lstm_cases()[case]
    I = 32
    torch.manual_seed(B + T)
    m = torch.nn.LSTM(I, H, num_layers=2, bidirectional=nd == 2, batch_first=True).cuda()
    x = torch.randn(B, T, I, device='cuda', requires_grad=True)
    dy = torch.randn(B, T, nd * H, device='cuda') * 0.1
    with _group_size(gs):
        assert lstm_path(B, nd, H, 0) == fwd and lstm_path(B, nd, H, 1)[0] == bwd[0]
        y = lstm_forward_train(m, x)
        assert _L().ttsc_lstm_split_status() == 0
        (y * dy).sum().backward()
        assert _L().ttsc_lstm_split_status() == 0
    p = {k: v.detach().cpu().numpy() for k, v in m.named_parameters()}
    xs, ds = x.detach().cpu().numpy(), dy.cpu().numpy()
    r64 = R.lstm_stack_grads(xs, p, ds, np.float64)
    r32 = R.lstm_stack_grads(xs, p, ds, np.float32)
    label = 'lstm layer %s/%s H=%d' % (LSTM_NAMES[fwd[0]], LSTM_NAMES[bwd[0]], H)
    fails = []
    for name, got in (('y', y.detach().cpu().numpy()), ('dx', x.grad.cpu().numpy())):
        for u in range(B):
            _windows(label, '%s u%d' % (name, u), got[u], r64[name][u], r32[name][u], fails)
    for k, v in m.named_parameters():
        f = _bound(label + ' weights', k, v.grad.cpu().numpy(), r64[k], r32[k])
        if f:
            fails.append(f)
    assert not fails, fails[:6]


# ---------------------------------------------------------------------------------------------------------------------------- dispatch
def _rule_gru(B, H, cus):
    """the GRU selection as written in gru.hip before the path query existed (gru_resident_members, gru_split_members)"""
    G = 16 if H == 512 else (4 if H == 256 else 0)
    if G and G * B <= cus and B <= 4096:
        return GRU_SPLIT_RES, G
    G = 1
    while G * 2 <= 4 and G * 2 * B <= cus and H % (G * 2) == 0 and H // (G * 2) >= 32 and 512 % (H // (G * 2)) == 0:
        HU = H // (G * 2)
        KS = 512 // HU
        if H % KS or (H // KS) % 8 or (3 * H // KS) % 16:
            break
        G *= 2
    return (GRU_SPLIT if G > 1 else GRU_SEQ), G


def _lstm_split_members(B, nd, H, cus):
    G = 1
    while G * 2 <= 4 and G * 2 * B * nd <= cus and H % (G * 2) == 0 and H // (G * 2) >= 32 and 512 % (H // (G * 2)) == 0:
        HU = H // (G * 2)
        KS = 512 // HU
        if H % KS or (H // KS) % 8 or (4 * H // KS) % 16:
            break
        G *= 2
    return G


def _rule_lstm_fwd(B, nd, H, cus):
    """lstm_forward_impl's selection for a training launch (gates saved), as written before the path query existed"""
    if H in (64, 128):
        return L_RESIDENT, (1, 1, 1)
    if H in (256, 512) and cus >= 4:
        Gm = 4 if H == 256 else 16
        cap = cus // Gm
        NB = 1
        while NB < 4 and -(-B // NB) * nd > cap:
            NB *= 2
        groups = -(-B // NB) * nd
        if cap >= 1 and groups <= 3 * cap and B * nd <= 16384:
            return (L_SPLIT_RES if NB == 1 else L_SPLIT_RES_NB), (Gm, NB, -(-groups // cap))
    G = _lstm_split_members(B, nd, H, cus)
    if G > 1:
        return L_SPLIT, (G, 1, 1)
    return L_SEQ, (1, 2 if B * nd > 512 else 1, 1)


def _rule_lstm_bwd(B, nd, H, cus):
    G = _lstm_split_members(B, nd, H, cus)
    if G > 1:
        return (L_SPLIT_RES if 4 * H // (512 // (H // G)) == 128 else L_SPLIT), (G, 1, 1)
    return (L_RESIDENT if H in (64, 128) else L_SEQ), (1, 1, 1)


@pytest.mark.gpu
def test_dispatch_query_follows_the_selection_rules():
    """the path query (the launchers' own selection) against a restatement of the selection rules over a grid of (B, ndir, H); prints the table"""
    c = _cus()
    rows, bad = [], []
    for H in (36, 64, 100, 128, 192, 256, 384, 512):
        for B in (1, 2, 4, 8, 16, 17, 32, 33, 40, 48, 64, 65, 100, 128, 129, 200, 256, 300, 400, 1024):
            g = gru_path(B, H)
            if g != (lambda p: (p[0], (p[1], 1, 1)))(_rule_gru(B, H, c)) or gru_path(B, H, 1) != g:
                bad.append(('gru', B, H, g))
            rows.append('gru  B=%4d H=%3d          fwd/bwd %s G=%d' % (B, H, GRU_NAMES[g[0]], g[1][0]))
            for nd in (1, 2):
                f, b = lstm_path(B, nd, H, 0), lstm_path(B, nd, H, 1)
                if f != _rule_lstm_fwd(B, nd, H, c) or b != _rule_lstm_bwd(B, nd, H, c):
                    bad.append(('lstm', B, nd, H, f, b))
                rows.append('lstm B=%4d H=%3d ndir=%d   fwd %s G=%d NB=%d launches=%d   bwd %s G=%d' % (
                    B, H, nd, LSTM_NAMES[f[0]], f[1][0], f[1][1], f[1][2], LSTM_NAMES[b[0]], b[1][0]))
    print('\n%d CUs\n' % c + '\n'.join(rows))
    assert not bad, bad[:8]
