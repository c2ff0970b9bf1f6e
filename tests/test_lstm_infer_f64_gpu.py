"""GPU: the LSTM inference recurrence (lstm.hip ttsc_lstm_seq_forward, hip_layers.LSTMHip) against the float64 oracle
(oracle/rnn_train_ref.py lstm_layer_forward with lengths / h0 / c0 / final states) on every kernel the entry point dispatches to:
lstm_seq_kernel<1> / <2>, lstm_seq_resident_kernel<64> / <128>, lstm_seq_split_res_kernel, lstm_seq_split_res_nb_kernel<2> / <4> / <8>.

Every case asks the dispatch query (ttsc_lstm_train_path) which kernel it reaches and asserts the intended path; the batch sizes are the smallest
that reach each kernel, derived from the device's CU count.  The query equals the inference dispatch only while TTSC_LSTM_SPLIT_INFER,
TTSC_LSTM_RESIDENT, TTSC_LSTM_SPLIT and TTSC_LSTM_NB are unset: the file is skipped otherwise.

  kernel level  ttsc_lstm_seq_forward on a ragged batch with initial states, an output pitch wider than the layer (ldy = ndir*H + 24, yoff = 8),
                y / h_n / c_n NaN-filled before the launch and every xg row at t >= len NaN-filled (linear_hip leaves whole padding tiles of xg
                unwritten, so they may hold anything).  y at t < len, h_n and c_n of chosen utterances against the oracle; zeros at t >= len; the
                columns outside [yoff, yoff + ndir*H) untouched; nothing non-finite; each utterance run alone gives the same bits; the plain launch
                (no lengths, no states, dense y) gives the same bits for the full-length zero-state utterances.  Plus a zero-length utterance and
                T chained one-step calls against one T-step call.
  layer level   LSTMHip over a 2-layer module with lengths, hx and return_state against torch.nn.LSTM(...).double() on packed sequences.

Bound (tests/test_rnn_train_gpu.py, unchanged): err_kernel <= 4 * err_yardstick + 1e-6 * max|ref| + 2^-23, max-abs errors against float64 per
(utterance, window of <= 1 000 steps) or per state vector.  Kernel-level yardstick: the same oracle in float32, with the W_hh products as one
k-ordered chain for lstm_seq_kernel.  Layer-level yardstick: the same torch module in float32 on the CPU.

Layer level, worst kernel / yardstick ratio per case, measured on 256 CUs with the hoisted projection on the split-precision GEMM and on the
exact fp32 GEMM (hip_layers.SPLIT_GEMM = False):
    case                 path        split GEMM   exact GEMM
    in641 H64 bi         resident    0.982        1.036
    in256 H256 bi        split_res   1.045        0.449
    in256 H200 bi        seq         1.137        0.693
    in1280 H512 uni      split_res   1.214        1.061
Neither exceeds 4, so the layer level keeps the kernel-level bound with its factor 4 for both GEMMs."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import rnn_train_ref as R
from tests.test_rnn_train_gpu import (L_RESIDENT, L_SEQ, L_SPLIT_RES, L_SPLIT_RES_NB, LSTM_NAMES, RATIOS, _L, _bound, _cus, _group_size, _lstm_pack,
                                      _pick, _windows, lstm_path)

_SWITCHES = [k for k in ('TTSC_LSTM_SPLIT_INFER', 'TTSC_LSTM_RESIDENT', 'TTSC_LSTM_SPLIT', 'TTSC_LSTM_NB') if k in os.environ]
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(_SWITCHES), reason='%s set: ttsc_lstm_train_path no longer equals the inference dispatch' % ', '.join(_SWITCHES))]

PAD, YOFF = 24, 8
PREFIX = 'lstm infer '


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    mine = sorted(k for k in RATIOS if k.startswith(PREFIX))
    if mine:
        print('\nLSTM inference: kernel / float32-yardstick max-abs error ratio per path (bound: 4):')
        for k in mine:
            print('  %-64s %.3f' % (k, RATIOS.pop(k)))


def _cases():
    c = _cus()
    return {
        # label: H, ndir, B, T, group size, (path, (G, NB, launches))
        'resident H64': (64, 2, 5, 700, 0, (L_RESIDENT, (1, 1, 1))),
        'resident H128': (128, 1, 3, 40, 0, (L_RESIDENT, (1, 1, 1))),
        'split_res H256': (256, 2, 3, 300, 0, (L_SPLIT_RES, (4, 1, 1))),
        'split_res H512': (512, 1, 2, 120, 0, (L_SPLIT_RES, (16, 1, 1))),
        'nb2 H256': (256, 2, 3 * c // 16 - 1, 60, 0, (L_SPLIT_RES_NB, (4, 2, 1))),
        'nb4 H256': (256, 2, c // 2 - 3, 40, 0, (L_SPLIT_RES_NB, (4, 4, 1))),
        'nb4 two launches': (512, 1, 25 * c // 64 - 1, 30, 0, (L_SPLIT_RES_NB, (16, 4, 2))),
        'nb8': (512, 1, c // 16 + 3, 30, 8, (L_SPLIT_RES_NB, (16, 8, 1))),
        'seq1 H200': (200, 2, 3, 50, 0, (L_SEQ, (1, 1, 1))),
        'seq1 H36': (36, 1, 2, 50, 0, (L_SEQ, (1, 1, 1))),
        'seq1 H384': (384, 2, 2, 20, 0, (L_SEQ, (1, 1, 1))),
        'seq1 H512 big': (512, 2, 3 * c // 8 + 4, 12, 0, (L_SEQ, (1, 1, 1))),
        'seq2 H96': (96, 2, 261, 9, 0, (L_SEQ, (1, 2, 1))),
    }


_IDS = ['resident H64', 'resident H128', 'split_res H256', 'split_res H512', 'nb2 H256', 'nb4 H256', 'nb4 two launches', 'nb8', 'seq1 H200',
        'seq1 H36', 'seq1 H384', 'seq1 H512 big', 'seq2 H96']


def _lengths(B, T):
    """ragged lengths with T (utterance 0, and B - 2 from four utterances on) and 1 (utterance 1); the batch sizes of the NB / seq<2> cases
    leave the last member group / workgroup partly empty, and its members end early"""
    lens = [(7 * b) % T + 1 for b in range(B)]
    lens[0] = T
    lens[1] = 1
    if B >= 4:
        lens[B - 2] = T
        lens[B - 1] = max(1, (2 * T) // 3)
    return lens


def _zero_state_utt(B):
    """the full-length utterance that starts from h0 = c0 = 0 (what the plain launch is compared on)"""
    return B - 2 if B >= 4 else 0


def _inputs(B, T, H, nd, seed, lens=None):
    """xg ~ 0.8 N(0,1) with NaN rows at t >= len, whh uniform +-H^-1/2, h0 uniform +-0.9, c0 uniform +-1.5 (zero for _zero_state_utt)"""
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    whh = (torch.rand(nd, 4 * H, H, device='cuda', generator=g) * 2 - 1) * H ** -0.5
    xg = torch.randn(B, T, nd * 4 * H, device='cuda', generator=g) * 0.8
    h0 = (torch.rand(nd, B, H, device='cuda', generator=g) * 2 - 1) * 0.9
    c0 = (torch.rand(nd, B, H, device='cuda', generator=g) * 2 - 1) * 1.5
    if lens is not None:
        z = _zero_state_utt(B)
        h0[:, z] = 0
        c0[:, z] = 0
        for b, n in enumerate(lens):
            xg[b, n:] = float('nan')
    return xg, whh, h0, c0


def _run(xg, wp, H, nd, lens=None, h0=None, c0=None, pad=0, yoff=0, state=True):
    """ttsc_lstm_seq_forward on NaN-filled y [B,T,nd*H + pad] / h_n / c_n -> y, h_n, c_n (device)"""
    from ttscube_amd import _lib
    B, T, _ = xg.shape
    nan = float('nan')
    ldy = nd * H + pad
    y = torch.full((B, T, ldy), nan, device='cuda')
    hn = torch.full((nd, B, H), nan, device='cuda') if state else None
    cn = torch.full((nd, B, H), nan, device='cuda') if state else None
    ld = torch.tensor(lens, dtype=torch.int32, device='cuda') if lens is not None else None
    P = lambda t: _lib.dev_ptr(t) if t is not None else None
    _lib.check(_L().ttsc_lstm_seq_forward(P(xg), P(wp), P(y), P(ld), B, T, H, nd, ldy, yoff, P(h0), P(c0), P(hn), P(cn), None),
               'ttsc_lstm_seq_forward')
    assert _L().ttsc_lstm_split_status() == 0
    torch.cuda.synchronize()
    return y, hn, cn


def _check_layout(y, hn, cn, lens, H, nd, pad, yoff):
    """the whole batch: zeros at t >= len, finite at t < len, finite states, untouched columns still NaN"""
    B, T, _ = y.shape
    valid = torch.arange(T, device='cuda')[None, :] < torch.tensor(lens, device='cuda')[:, None]
    core = y[:, :, yoff:yoff + nd * H]
    assert bool(torch.isfinite(core[valid]).all()), 'non-finite y at t < len (a NaN xg row consumed, or an element not written)'
    assert bool((core[~valid] == 0).all()), 'y at t >= len is not exactly zero'
    assert bool(torch.isfinite(hn).all()) and bool(torch.isfinite(cn).all()), 'non-finite / unwritten final state'
    if pad:
        assert bool(torch.isnan(y[:, :, :yoff]).all()) and bool(torch.isnan(y[:, :, yoff + nd * H:]).all()), 'columns outside the layer written'


def _oracle(xg, whh, h0, c0, lens, sel, chain):
    """float64 reference and float32 yardstick of the selected utterances -> two dicts y [n,T,nd*H], h, c [nd,n,H]"""
    idx = torch.tensor(sel, device='cuda')
    xs = xg.index_select(0, idx).cpu().numpy()
    hs, cs = (t.index_select(1, idx).cpu().numpy() for t in (h0, c0))
    W = whh.cpu().numpy()
    ls = [lens[u] for u in sel]
    out = []
    for dt, ch in ((np.float64, False), (np.float32, chain)):
        y, _, _, hn, cn = R.lstm_layer_forward(xs, W, dt, lengths=ls, h0=hs, c0=cs, return_state=True, chain=ch)
        out.append({'y': y, 'h': hn, 'c': cn})
    return out


def _check_accuracy(label, sel, lens, y, hn, cn, ref, yard, fails):
    """y [n,T,nd*H], hn / cn [nd,n,H] (numpy, the selected utterances) against the oracle per utterance"""
    for i, u in enumerate(sel):
        n = lens[u]
        _windows(label, 'y u%d' % u, y[i, :n], ref['y'][i, :n], yard['y'][i, :n], fails)
        for name, got in (('h', hn), ('c', cn)):
            f = _bound(label, '%s_n u%d' % (name, u), got[:, i], ref[name][:, i], yard[name][:, i])
            if f:
                fails.append(f)


@pytest.mark.parametrize('case', _IDS)
def test_lstm_inference_kernels_match_float64_oracle(case):
    H, nd, B, T, gs, path = _cases()[case]
    lens = _lengths(B, T)
    seq = path[0] == L_SEQ
    label = PREFIX + '%s (%s G=%d NB=%d x%d%s)' % (case, LSTM_NAMES[path[0]], path[1][0], path[1][1], path[1][2], ', chain yardstick' if seq else '')
    xg, whh, h0, c0 = _inputs(B, T, H, nd, seed=H + B + T, lens=lens)
    wp = _lstm_pack(whh, 0)
    with _group_size(gs):
        assert lstm_path(B, nd, H, 0) == path, (case, B, lstm_path(B, nd, H, 0))
        y, hn, cn = _run(xg, wp, H, nd, lens, h0, c0, PAD, YOFF)
        # plain: no lengths, no states, dense y — the same bits for the full-length utterance that started from zero
        yp, _, _ = _run(torch.nan_to_num(xg, nan=0.25), wp, H, nd, state=False)
    _check_layout(y, hn, cn, lens, H, nd, PAD, YOFF)
    core = y[:, :, YOFF:YOFF + nd * H]
    z = _zero_state_utt(B)
    assert lens[z] == T and not bool(h0[:, z].any()) and not bool(c0[:, z].any())
    assert bool(torch.isfinite(yp).all())
    assert torch.equal(yp[z], core[z]), 'the plain launch differs from the ragged / offset launch'

    sel = sorted(set(_pick(B)) | {0, 1, z})
    assert {lens[u] for u in sel} >= {1, T}
    idx = torch.tensor(sel, device='cuda')
    ref, yard = _oracle(xg, whh, h0, c0, lens, sel, chain=seq)
    fails = []
    _check_accuracy(label, sel, lens, core.index_select(0, idx).cpu().numpy(), hn.index_select(1, idx).cpu().numpy(),
                    cn.index_select(1, idx).cpu().numpy(), ref, yard, fails)

    # batch independence: each chosen utterance alone, its length as T, its own initial state
    big = case == 'seq1 H512 big'      # its solo run takes split_res: another summation order, compared to rounding
    solo_path = {L_SPLIT_RES_NB: L_SPLIT_RES}.get(path[0], path[0]) if not big else L_SPLIT_RES
    assert lstm_path(1, nd, H, 0)[0] == solo_path, (case, lstm_path(1, nd, H, 0))
    if big:
        yard_solo = _oracle(xg, whh, h0, c0, lens, sel, chain=False)[1]
    for i, u in enumerate(sel):
        n = lens[u]
        ys, hs, cs = _run(xg[u:u + 1, :n].contiguous(), wp, H, nd, None, h0[:, u:u + 1].contiguous(), c0[:, u:u + 1].contiguous())
        if big:
            one = lambda a: {k: v[i:i + 1] if k == 'y' else v[:, i:i + 1] for k, v in a.items()}
            _check_accuracy(label + ' solo split_res', [u], lens, ys.cpu().numpy(), hs.cpu().numpy(), cs.cpu().numpy(), one(ref), one(yard_solo),
                            fails)
        else:
            assert torch.equal(ys[0], core[u, :n]), (case, 'y of utterance %d alone differs from its rows in the batch' % u)
            assert torch.equal(hs[:, 0], hn[:, u]) and torch.equal(cs[:, 0], cn[:, u]), (case, 'final state of utterance %d alone differs' % u)
    assert not fails, fails[:6]


@pytest.mark.parametrize('case', ['split_res H256', 'nb2 H256'])
def test_lstm_zero_length_utterance(case):
    """one utterance of length 0: its y row is all zeros, its final state is its initial state bit for bit, and the other utterances keep the
    bits they have when it is one step long (the kernels neither poll nor publish for such a row)"""
    H, nd, B, T, gs, path = _cases()[case]
    lens = _lengths(B, T)
    zu = 2 if B == 3 else 3            # nb2: the second member of group 1, whose partner keeps running
    assert lens[zu] > 0
    xg, whh, h0, c0 = _inputs(B, T, H, nd, seed=H + B + T, lens=lens)
    wp = _lstm_pack(whh, 0)
    lens0 = list(lens)
    lens0[zu] = 0
    xg0 = xg.clone()
    xg0[zu] = float('nan')
    with _group_size(gs):
        assert lstm_path(B, nd, H, 0) == path
        y, hn, cn = _run(xg, wp, H, nd, lens, h0, c0, PAD, YOFF)
        y0, hn0, cn0 = _run(xg0, wp, H, nd, lens0, h0, c0, PAD, YOFF)
    _check_layout(y0, hn0, cn0, lens0, H, nd, PAD, YOFF)
    assert bool((y0[zu, :, YOFF:YOFF + nd * H] == 0).all())
    assert torch.equal(hn0[:, zu], h0[:, zu]) and torch.equal(cn0[:, zu], c0[:, zu])
    others = torch.tensor([b for b in range(B) if b != zu], device='cuda')
    for a, b, dim in ((y0, y, 0), (hn0, hn, 1), (cn0, cn, 1)):
        a, b = a.index_select(dim, others), b.index_select(dim, others)
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))   # (the untouched columns are NaN in both)


@pytest.mark.parametrize('H,path', [(512, (L_SPLIT_RES, (16, 1, 1))), (200, (L_SEQ, (1, 1, 1))), (128, (L_RESIDENT, (1, 1, 1)))],
                         ids=['split_res H512', 'seq H200', 'resident H128'])
def test_lstm_one_call_equals_chained_one_step_calls(H, path):
    """one call over T steps == T one-step calls that pass (h_n, c_n) on as (h_0, c_0), bit for bit (y, h_n, c_n): the pattern of the stepwise AR
    decoder, at H = 512 on split_res G = 16"""
    B, T, nd = 1, 40, 1
    assert lstm_path(B, nd, H, 0) == path
    xg, whh, h0, c0 = _inputs(B, T, H, nd, seed=H + 17)
    wp = _lstm_pack(whh, 0)
    y, hn, cn = _run(xg, wp, H, nd, None, h0, c0)
    h, c, ys = h0, c0, []
    for t in range(T):
        yt, h, c = _run(xg[:, t:t + 1].contiguous(), wp, H, nd, None, h, c)
        ys.append(yt)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(torch.cat(ys, 1), y) and torch.equal(h, hn) and torch.equal(c, cn)


# ---------------------------------------------------------------------------------------------------------------------------- layer level
_LAYER = {
    # label: in, H, bidirectional, B, T, lengths, path of the recurrence
    'in641 H64 bi': (641, 64, True, 3, 90, [90, 1, 37], (L_RESIDENT, (1, 1, 1))),
    'in256 H256 bi': (256, 256, True, 5, 37, [37, 1, 20, 9, 30], (L_SPLIT_RES, (4, 1, 1))),
    'in256 H200 bi': (256, 200, True, 4, 30, [30, 7, 1, 18], (L_SEQ, (1, 1, 1))),
    'in1280 H512 uni': (1280, 512, False, 2, 12, None, (L_SPLIT_RES, (16, 1, 1))),
}


def _layer_bound(label, what, got, ref, yard, fails):
    f = _bound(label, what, got, ref, yard)
    if f:
        fails.append(f)


@pytest.mark.parametrize('gemm', ['split', 'exact'])
@pytest.mark.parametrize('case', list(_LAYER))
def test_lstm_layer_with_lengths_and_states_matches_float64(case, gemm, monkeypatch):
    """LSTMHip(m)(x, lengths, hx, return_state=True) over two layers against the float64 module on packed sequences; yardstick: the float32
    module on the CPU.  gemm = exact runs the hoisted projection on the exact fp32 GEMM: its ratios must stay within 4 (the recurrence)."""
    from ttscube_amd import hip_layers
    I, H, bi, B, T, lens, path = _LAYER[case]
    nd = 2 if bi else 1
    assert lstm_path(B, nd, H, 0) == path
    if gemm == 'exact':
        monkeypatch.setattr(hip_layers, 'SPLIT_GEMM', False)
    assert hip_layers.SPLIT_GEMM == (gemm == 'split')
    torch.manual_seed(I + H + T)
    m32 = torch.nn.LSTM(I, H, num_layers=2, bidirectional=bi, batch_first=True)
    m64 = torch.nn.LSTM(I, H, num_layers=2, bidirectional=bi, batch_first=True).double()
    m64.load_state_dict({k: v.double() for k, v in m32.state_dict().items()})
    x = torch.randn(B, T, I)
    hx = ((torch.rand(2 * nd, B, H) * 2 - 1) * 0.9, (torch.rand(2 * nd, B, H) * 2 - 1) * 1.5)
    full = lens if lens is not None else [T] * B

    def cpu(m, dt):
        with torch.no_grad():
            packed = torch.nn.utils.rnn.pack_padded_sequence(x.to(dt), full, batch_first=True, enforce_sorted=False)
            out, (h, c) = m(packed, (hx[0].to(dt), hx[1].to(dt)))
            y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
        return y.numpy(), h.numpy(), c.numpy()

    ref, yard = cpu(m64, torch.float64), cpu(m32, torch.float32)
    h = hip_layers.LSTMHip(copy.deepcopy(m32).cuda())
    xd = x.cuda()
    y, (hn, cn) = h(xd, lens, (hx[0].cuda(), hx[1].cuda()), return_state=True)
    assert _L().ttsc_lstm_split_status() == 0
    label = PREFIX + 'layer %s (%s), %s GEMM' % (case, LSTM_NAMES[path[0]], gemm)
    fails = []
    yk, hk, ck = y.cpu().numpy(), hn.cpu().numpy(), cn.cpu().numpy()
    for u in range(B):
        n = full[u]
        assert not yk[u, n:].any(), 'y at t >= len is not zero'
        _layer_bound(label, 'y u%d' % u, yk[u, :n], ref[0][u, :n], yard[0][u, :n], fails)
        _layer_bound(label, 'h_n u%d' % u, hk[:, u], ref[1][:, u], yard[1][:, u], fails)
        _layer_bound(label, 'c_n u%d' % u, ck[:, u], ref[2][:, u], yard[2][:, u], fails)
    # no hx == explicit zeros, bit for bit
    za, (zh, zc) = h(xd, lens, None, return_state=True)
    zeros = torch.zeros(2 * nd, B, H, device='cuda')
    ea, (eh, ec) = h(xd, lens, (zeros, zeros.clone()), return_state=True)
    assert _L().ttsc_lstm_split_status() == 0
    assert torch.equal(za, ea) and torch.equal(zh, eh) and torch.equal(zc, ec)
    assert not fails, fails[:6]
