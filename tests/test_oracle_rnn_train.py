"""CPU: the float64 GRU / LSTM training oracle (oracle/rnn_train_ref.py) against torch float64 autograd over nn.GRU / nn.LSTM."""
import numpy as np
import pytest
import torch

from oracle import rnn_train_ref as R

TOL = 1e-12


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize('B,T,I,H,with_h0', [(3, 1, 5, 8, False), (2, 7, 4, 12, True), (3, 40, 6, 16, False), (1, 2, 3, 4, True)])
def test_gru_oracle_matches_torch_float64(B, T, I, H, with_h0):
    torch.manual_seed(B * 100 + T)
    m = torch.nn.GRU(I, H, batch_first=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    h0 = (0.5 * torch.randn(1, B, H, dtype=torch.float64)).requires_grad_() if with_h0 else None
    dy = torch.randn(B, T, H, dtype=torch.float64)
    y, _ = m(x, h0)
    (y * dy).sum().backward()
    p = {k: v.detach().numpy() for k, v in m.named_parameters()}
    h0n = h0.detach()[0].numpy() if with_h0 else None
    for window in (1000, 3):   # one window, and windows that cut the sequence (checkpointed recompute)
        g = R.gru_layer_grads(x.detach().numpy(), p['weight_ih_l0'], p['weight_hh_l0'], p['bias_ih_l0'], p['bias_hh_l0'], dy.numpy(), h0n,
                              window=window)
        assert _rel(g['y'], y.detach().numpy()) < TOL
        assert _rel(g['dx'], x.grad.numpy()) < TOL
        for k, v in m.named_parameters():
            assert _rel(g[k], v.grad.numpy()) < TOL, k
        if with_h0:
            assert _rel(g['dh0'], h0.grad[0].numpy()) < TOL


def test_gru_oracle_saved_and_gate_gradients():
    """saved (r, z, n, W_hn h + b_hn) restated from the torch weights; dgi / dgh against autograd on the pre-activations"""
    torch.manual_seed(7)
    B, T, H = 2, 6, 8
    xg = torch.randn(B, T, 3 * H, dtype=torch.float64, requires_grad=True)
    whh = 0.4 * torch.randn(3 * H, H, dtype=torch.float64)
    bhh = (0.3 * torch.randn(3 * H, dtype=torch.float64)).requires_grad_()
    h0 = 0.5 * torch.randn(B, H, dtype=torch.float64)
    dy = torch.randn(B, T, H, dtype=torch.float64)
    h, ys, hns, rs, zs, ns = h0, [], [], [], [], []
    for t in range(T):
        gh = h @ whh.T + bhh
        r = torch.sigmoid(xg[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(xg[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(xg[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        ys.append(h)
        rs.append(r), zs.append(z), ns.append(n), hns.append(gh[:, 2 * H:])
    y = torch.stack(ys, 1)
    (y * dy).sum().backward()
    yo, saved = R.gru_forward(xg.detach().numpy(), whh.numpy(), bhh.detach().numpy(), h0.numpy())
    assert _rel(yo, y.detach().numpy()) < TOL
    want = torch.cat([torch.stack(v, 1) for v in (rs, zs, ns, hns)], dim=2).detach().numpy()
    assert _rel(saved, want) < TOL
    dgi, dgh, _ = R.gru_backward(xg.detach().numpy(), whh.numpy(), bhh.detach().numpy(), dy.numpy(), h0.numpy())
    assert _rel(dgi, xg.grad.numpy()) < TOL
    # the hidden-side gradient summed over steps is the b_hh gradient
    assert _rel(dgh.sum(axis=(0, 1)), bhh.grad.numpy()) < TOL


@pytest.mark.parametrize('B,T,I,H,layers,bi', [(3, 1, 5, 8, 1, False), (2, 1, 4, 8, 2, True), (2, 9, 6, 12, 2, True), (3, 30, 4, 8, 1, True),
                                               (1, 5, 3, 4, 3, False)])
def test_lstm_oracle_matches_torch_float64(B, T, I, H, layers, bi):
    torch.manual_seed(B * 1000 + T * 10 + layers)
    m = torch.nn.LSTM(I, H, num_layers=layers, bidirectional=bi, batch_first=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    y, _ = m(x)
    dy = torch.randn(*y.shape, dtype=torch.float64)
    (y * dy).sum().backward()
    p = {k: v.detach().numpy() for k, v in m.named_parameters()}
    g = R.lstm_stack_grads(x.detach().numpy(), p, dy.numpy())
    assert _rel(g['y'], y.detach().numpy()) < TOL
    assert _rel(g['dx'], x.grad.numpy()) < TOL
    for k, v in m.named_parameters():
        assert _rel(g[k], v.grad.numpy()) < TOL, k


def test_lstm_oracle_gates_cells_and_gate_gradients():
    """the saved gates / cell states and dG of one bidirectional layer against autograd on the pre-activations"""
    torch.manual_seed(3)
    B, T, H, nd = 2, 5, 6, 2
    xg = torch.randn(B, T, nd * 4 * H, dtype=torch.float64, requires_grad=True)
    whh = 0.4 * torch.randn(nd, 4 * H, H, dtype=torch.float64)
    dy = torch.randn(B, T, nd * H, dtype=torch.float64)
    ys = torch.zeros(B, T, nd * H, dtype=torch.float64)
    gts = torch.zeros(B, T, nd * 4 * H, dtype=torch.float64)
    cs = torch.zeros(B, T, nd * H, dtype=torch.float64)
    ys, gts, cs = list(ys.unbind(1)), list(gts.unbind(1)), list(cs.unbind(1))
    yd = [[None] * T for _ in range(nd)]
    for d in range(nd):
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        for t in (range(T) if d == 0 else reversed(range(T))):
            pre = xg[:, t, d * 4 * H:(d + 1) * 4 * H] + h @ whh[d].T
            i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            yd[d][t] = h
            gts[t] = torch.cat([gts[t][:, :d * 4 * H], i, f, g, o, gts[t][:, (d + 1) * 4 * H:]], dim=1)
            cs[t] = torch.cat([cs[t][:, :d * H], c, cs[t][:, (d + 1) * H:]], dim=1)
    y = torch.stack([torch.cat([yd[d][t] for d in range(nd)], dim=1) for t in range(T)], 1)
    (y * dy).sum().backward()
    yo, gates, cst = R.lstm_layer_forward(xg.detach().numpy(), whh.numpy())
    assert _rel(yo, y.detach().numpy()) < TOL
    assert _rel(gates, torch.stack(gts, 1).detach().numpy()) < TOL
    assert _rel(cst, torch.stack(cs, 1).detach().numpy()) < TOL
    dG = R.lstm_layer_backward(dy.numpy(), gates, cst, whh.numpy())
    assert _rel(dG, xg.grad.numpy()) < TOL


def _lstm_old_forward(xg, whh):
    """lstm_layer_forward as it stood before it took lengths / states (zero state, full length), kept here to pin the defaults bit for bit"""
    B, T, _ = xg.shape
    nd, H4, H = whh.shape
    y, gates, cs = np.empty((B, T, nd * H)), np.empty((B, T, nd * H4)), np.empty((B, T, nd * H))
    for d in range(nd):
        whhT = np.ascontiguousarray(whh[d].T)
        h, c = np.zeros((B, H)), np.zeros((B, H))
        for t in (range(T) if d == 0 else reversed(range(T))):
            pre = xg[:, t, d * H4:(d + 1) * H4] + h @ whhT
            i, f, g, o = R._sig(pre[:, :H]), R._sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), R._sig(pre[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            y[:, t, d * H:(d + 1) * H], cs[:, t, d * H:(d + 1) * H] = h, c
            gates[:, t, d * H4:(d + 1) * H4] = np.concatenate([i, f, g, o], axis=1)
    return y, gates, cs


def test_lstm_oracle_defaults_are_unchanged():
    rng = np.random.default_rng(4)
    B, T, H, nd = 3, 11, 12, 2
    xg, whh = rng.standard_normal((B, T, nd * 4 * H)), 0.3 * rng.standard_normal((nd, 4 * H, H))
    want = _lstm_old_forward(xg, whh)
    got = R.lstm_layer_forward(xg, whh)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    z = np.zeros((nd, B, H))
    full = R.lstm_layer_forward(xg, whh, lengths=[T] * B, h0=z, c0=z, return_state=True)   # the ragged walk at full length: the same recurrence
    assert all(_rel(a, b) < TOL for a, b in zip(full[:3], want))
    assert _rel(full[3][0], want[0][:, -1, :H]) < TOL and _rel(full[3][1], want[0][:, 0, H:]) < TOL
    assert _rel(full[4][0], want[2][:, -1, :H]) < TOL and _rel(full[4][1], want[2][:, 0, H:]) < TOL


@pytest.mark.parametrize('chain', [False, True])
@pytest.mark.parametrize('bi', [False, True])
@pytest.mark.parametrize('lens', [[9, 1, 4, 9, 7], [1, 6], [5]])
def test_lstm_oracle_ragged_with_states_matches_torch_float64(lens, bi, chain):
    """lengths (including 1 and T), non-zero hx, final states: against torch.nn.LSTM in float64 on a packed batch"""
    torch.manual_seed(len(lens) * 10 + bi)
    B, T, I, H, nd = len(lens), max(lens), 5, 8, 2 if bi else 1
    m = torch.nn.LSTM(I, H, bidirectional=bi, batch_first=True).double()
    x = torch.randn(B, T, I, dtype=torch.float64)
    h0 = 0.7 * torch.randn(nd, B, H, dtype=torch.float64)
    c0 = 1.2 * torch.randn(nd, B, H, dtype=torch.float64)
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False)
        out, (hn, cn) = m(packed, (h0, c0))
        y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    p = {k: v.detach().numpy() for k, v in m.named_parameters()}
    sfx = ['', '_reverse'][:nd]
    wih = np.concatenate([p['weight_ih_l0' + s] for s in sfx])
    bias = np.concatenate([p['bias_ih_l0' + s] + p['bias_hh_l0' + s] for s in sfx])
    whh = np.stack([p['weight_hh_l0' + s] for s in sfx])
    xg = x.numpy() @ wih.T + bias
    for b, n in enumerate(lens):
        xg[b, n:] = np.nan                     # rows beyond the length are never read
    yo, gates, cs, ho, co = R.lstm_layer_forward(xg, whh, lengths=lens, h0=h0.numpy(), c0=c0.numpy(), return_state=True, chain=chain)
    assert ho.shape == (nd, B, H) and co.shape == (nd, B, H)
    assert _rel(yo, y.numpy()) < TOL and _rel(ho, hn.numpy()) < TOL and _rel(co, cn.numpy()) < TOL
    for b, n in enumerate(lens):
        assert not yo[b, n:].any() and not gates[b, n:].any() and not cs[b, n:].any()
        assert np.isfinite(gates[b, :n]).all() and np.isfinite(cs[b, :n]).all()


@pytest.mark.parametrize('nd', [1, 2])
def test_lstm_oracle_zero_length_row(nd):
    """torch refuses a length of 0: the row is all zeros, its final state is its initial state, the other rows do not notice"""
    rng = np.random.default_rng(nd)
    B, T, H = 4, 6, 8
    lens = [6, 0, 1, 3]
    xg, whh = rng.standard_normal((B, T, nd * 4 * H)), 0.3 * rng.standard_normal((nd, 4 * H, H))
    h0, c0 = 0.5 * rng.standard_normal((nd, B, H)), rng.standard_normal((nd, B, H))
    xg[1] = np.nan
    y, gates, cs, hn, cn = R.lstm_layer_forward(xg, whh, lengths=lens, h0=h0, c0=c0, return_state=True)
    assert not y[1].any() and not gates[1].any() and not cs[1].any()
    assert np.array_equal(hn[:, 1], h0[:, 1]) and np.array_equal(cn[:, 1], c0[:, 1])
    keep = [0, 2, 3]
    o = R.lstm_layer_forward(xg[keep], whh, lengths=[lens[b] for b in keep], h0=h0[:, keep], c0=c0[:, keep], return_state=True)
    for a, b in zip((y[keep], gates[keep], cs[keep], hn[:, keep], cn[:, keep]), o):
        assert np.isfinite(b).all() and _rel(a, b) < TOL


def test_chain_summation_order_is_the_same_recurrence():
    """chain=True only changes the order of the W_hh sums: the same answer in float64"""
    rng = np.random.default_rng(1)
    B, T, H = 2, 9, 8
    args = (rng.standard_normal((B, T, 3 * H)), 0.3 * rng.standard_normal((3 * H, H)), 0.1 * rng.standard_normal(3 * H), rng.standard_normal((B, T, H)),
            0.5 * rng.standard_normal((B, H)))
    a = [ev for ev in R.gru_windows(*args, window=4)]
    b = [ev for ev in R.gru_windows(*args, window=4, chain=True)]
    for ea, eb in zip(a, b):
        for va, vb in zip(ea[1:], eb[1:]):
            if isinstance(va, np.ndarray):
                assert _rel(vb, va) < TOL


def test_float32_yardstick_runs_in_float32():
    rng = np.random.default_rng(0)
    xg = rng.standard_normal((1, 4, 12)).astype(np.float32)
    y, saved = R.gru_forward(xg, 0.3 * rng.standard_normal((12, 4)), np.zeros(12), dtype=np.float32)
    assert y.dtype == np.float32 and saved.dtype == np.float32
    y64, _ = R.gru_forward(xg, 0.3 * rng.standard_normal((12, 4)), np.zeros(12))
    assert y64.dtype == np.float64
