"""ORACLE (test infrastructure): numpy restatement of the GRU and LSTM training recurrences of gru.hip / lstm.hip, forward and
backward through time, for tests only.

torch.nn.GRU (gate order r, z, n):   r = s(xr + W_hr h + b_hr),  z = s(xz + W_hz h + b_hz),  hn = W_hn h + b_hn,
                                     n = tanh(xn + r * hn),      h' = (1 - z) * n + z * h        with xg = W_ih x + b_ih
torch.nn.LSTM (gate order i, f, g, o): gates = xg + W_hh h,  i, f, o = s(.), g = tanh(.),  c' = f c + i g,  h' = o tanh(c')
                                     with xg = W_ih x + b_ih + b_hh; the reverse direction walks the steps from T-1 down to 0
                                     (from len_b - 1 with ragged `lengths`: lstm_layer_forward, also the inference oracle of
                                     ttsc_lstm_seq_forward with initial and final states).

Every function takes `dtype`: float64 is the reference, float32 of the same code is the yardstick (what plain fp32 arithmetic makes of
the same problem).  The outputs are the quantities the kernels save or produce:
  GRU   saved [B,T,4H] = r, z, n, hn;   dgi [B,T,3H] = d(r_pre, z_pre, n_pre);   dgh [B,T,3H] = d(r_pre, z_pre), dn_pre * r
  LSTM  gates [B,T,ndir*4H] = post-activation i, f, g, o;   c [B,T,ndir*H];   dG [B,T,ndir*4H] = pre-activation gate gradients
Long GRU sequences run in windows: the forward keeps h only at the window starts and the backward recomputes each window
(`gru_windows`), so T = 24 000 at H = 512 stays well under 1 GB per utterance."""
import numpy as np


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _a(v, dtype):
    return None if v is None else np.asarray(v).astype(dtype, copy=False)


def _chain(init, v, M):
    """init + v @ M as ONE k-ordered sum per output (k = 0, 1, ...): the summation order of a single-workgroup recurrence kernel's fma chain,
    for the yardstick of those kernels (a BLAS product sums in blocks and rounds less)"""
    acc = np.array(np.broadcast_to(init, (v.shape[0], M.shape[1])), dtype=v.dtype)
    for k in range(M.shape[0]):
        acc += v[:, k:k + 1] * M[k]
    return acc


# ---------------------------------------------------------------------------------------------------------------------------- GRU
def _gru_fwd_window(xg_w, h, whh, bhh, chain=False):
    """steps of one window from state h [B,H] -> y [B,W,H], saved [B,W,4H], last h"""
    B, W, H3 = xg_w.shape
    H = H3 // 3
    y = np.empty((B, W, H), dtype=xg_w.dtype)
    saved = np.empty((B, W, 4 * H), dtype=xg_w.dtype)
    whhT = np.ascontiguousarray(whh.T)
    for t in range(W):
        gh = _chain(bhh, h, whhT) if chain else h @ whhT + bhh
        x = xg_w[:, t]
        r = _sig(x[:, :H] + gh[:, :H])
        z = _sig(x[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = np.tanh(x[:, 2 * H:] + r * hn)
        h = (1 - z) * n + z * h
        y[:, t] = h
        saved[:, t, :H], saved[:, t, H:2 * H], saved[:, t, 2 * H:3 * H], saved[:, t, 3 * H:] = r, z, n, hn
    return y, saved, h


def gru_windows(xg, whh, bhh, dy=None, h0=None, dtype=np.float64, window=1000, chain=False):
    """Generator over one GRU layer's training recurrence in windows of <= `window` steps.

    xg [B,T,3H] (W_ih x + b_ih), whh [3H,H], bhh [3H], dy [B,T,H] or None, h0 [B,H] or None.
    Yields ('fwd', t0, t1, y, saved) for the windows in ascending order; then, if dy is given, ('bwd', t0, t1, dgi, dgh, h_prev) in
    descending order (h_prev [B,t1-t0,H]: the state each step started from) and finally ('dh0', dh0).  Only the window-start states are
    kept between the two passes: the backward recomputes each window's forward from its start state.  chain=True: the W_hh products are
    k-ordered chains (`_chain`), the summation order of gru_seq_kernel / gru_bwd_kernel."""
    whh, bhh = _a(whh, dtype), _a(bhh, dtype)   # xg / dy are converted window by window
    B, T, H3 = xg.shape
    H = H3 // 3
    h = np.zeros((B, H), dtype=dtype) if h0 is None else _a(h0, dtype).copy()
    starts = list(range(0, T, window))
    ckpt = []
    for t0 in starts:
        t1 = min(t0 + window, T)
        ckpt.append(h)
        y, saved, h = _gru_fwd_window(_a(xg[:, t0:t1], dtype), h, whh, bhh, chain)
        yield ('fwd', t0, t1, y, saved)
    if dy is None:
        return
    dh_rec = np.zeros((B, H), dtype=dtype)
    for wi in reversed(range(len(starts))):
        t0 = starts[wi]
        t1 = min(t0 + window, T)
        y, saved, _ = _gru_fwd_window(_a(xg[:, t0:t1], dtype), ckpt[wi], whh, bhh, chain)
        dyw = _a(dy[:, t0:t1], dtype)
        hprev = np.concatenate([ckpt[wi][:, None], y[:, :-1]], axis=1)
        dgi = np.empty((B, t1 - t0, 3 * H), dtype=dtype)
        dgh = np.empty_like(dgi)
        for s in reversed(range(t1 - t0)):
            r, z, n, hn = saved[:, s, :H], saved[:, s, H:2 * H], saved[:, s, 2 * H:3 * H], saved[:, s, 3 * H:]
            dh = dyw[:, s] + dh_rec
            dn = dh * (1 - z) * (1 - n * n)
            dz = dh * (hprev[:, s] - n) * z * (1 - z)
            dr = dn * hn * r * (1 - r)
            dgi[:, s, :H], dgi[:, s, H:2 * H], dgi[:, s, 2 * H:] = dr, dz, dn
            dgh[:, s, :H], dgh[:, s, H:2 * H], dgh[:, s, 2 * H:] = dr, dz, dn * r
            dh_rec = _chain(dh * z, dgh[:, s], whh) if chain else dh * z + dgh[:, s] @ whh
        yield ('bwd', t0, t1, dgi, dgh, hprev)
    yield ('dh0', dh_rec)


def gru_forward(xg, whh, bhh, h0=None, dtype=np.float64):
    """-> y [B,T,H], saved [B,T,4H] (r, z, n, W_hn h + b_hn)"""
    ys, ss = [], []
    for _, _, _, y, saved in gru_windows(xg, whh, bhh, None, h0, dtype, window=1 << 30):
        ys.append(y)
        ss.append(saved)
    return np.concatenate(ys, axis=1), np.concatenate(ss, axis=1)


def gru_backward(xg, whh, bhh, dy, h0=None, dtype=np.float64):
    """-> dgi [B,T,3H], dgh [B,T,3H], dh0 [B,H]"""
    out = {}
    for ev in gru_windows(xg, whh, bhh, dy, h0, dtype, window=1 << 30):
        if ev[0] == 'bwd':
            out['dgi'], out['dgh'] = ev[3], ev[4]
        elif ev[0] == 'dh0':
            out['dh0'] = ev[1]
    return out['dgi'], out['dgh'], out['dh0']


def gru_layer_grads(x, w_ih, w_hh, b_ih, b_hh, dy, h0=None, dtype=np.float64, window=1000):
    """One unidirectional torch.nn.GRU layer (batch_first) with loss sum(y * dy) -> dict y, dx, dh0 and the gradients of
    weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0 (torch names).  Weight gradients are accumulated window by window."""
    x, w_ih, w_hh, b_ih, b_hh = (_a(v, dtype) for v in (x, w_ih, w_hh, b_ih, b_hh))
    xg = x @ w_ih.T + b_ih
    g = {'weight_ih_l0': np.zeros_like(w_ih), 'weight_hh_l0': np.zeros_like(w_hh), 'bias_ih_l0': np.zeros_like(b_ih),
         'bias_hh_l0': np.zeros_like(b_hh)}
    ys, dx = [], np.empty_like(x)
    for ev in gru_windows(xg, w_hh, b_hh, dy, h0, dtype, window):
        if ev[0] == 'fwd':
            ys.append(ev[3])
        elif ev[0] == 'bwd':
            _, t0, t1, dgi, dgh, hprev = ev
            H3 = dgi.shape[2]
            gi2, gh2 = dgi.reshape(-1, H3), dgh.reshape(-1, H3)
            dx[:, t0:t1] = dgi @ w_ih
            g['weight_ih_l0'] += gi2.T @ x[:, t0:t1].reshape(-1, x.shape[2])
            g['weight_hh_l0'] += gh2.T @ hprev.reshape(-1, hprev.shape[2])
            g['bias_ih_l0'] += gi2.sum(axis=0)
            g['bias_hh_l0'] += gh2.sum(axis=0)
        else:
            g['dh0'] = ev[1]
    g['y'] = np.concatenate(ys, axis=1)
    g['dx'] = dx
    return g


# ---------------------------------------------------------------------------------------------------------------------------- LSTM
def _lstm_cell(x, h, c, whhT, H, chain):
    """one step: x [n,4H] (the xg rows), state h, c [n,H] -> post-activation gates [n,4H], c', h'"""
    pre = _chain(x, h, whhT) if chain else x + h @ whhT
    i, f, g, o = _sig(pre[:, :H]), _sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), _sig(pre[:, 3 * H:])
    c = f * c + i * g
    h = o * np.tanh(c)
    return np.concatenate([i, f, g, o], axis=1), c, h


def lstm_layer_forward(xg, whh, dtype=np.float64, lengths=None, h0=None, c0=None, return_state=False, chain=False):
    """xg [B,T,ndir*4H] (W_ih x + b_ih + b_hh), whh [ndir,4H,H] -> y [B,T,ndir*H], gates [B,T,ndir*4H] (post-activation i,f,g,o),
    c [B,T,ndir*H]; with return_state also h_n, c_n [ndir,B,H].  h0 / c0 [ndir,B,H]: the initial state (None: zeros).
    lengths [B] (None: all T): pack_padded_sequence semantics — direction 1 of utterance b walks len_b - 1 .. 0, y / gates / c are zero at
    t >= len_b and never read there (those xg rows may hold anything), the final state is the state after the utterance's own last step; a
    length of 0 gives an all-zero row with h_n = h0, c_n = c0.  chain=True: the W_hh h product is one k-ordered sum starting from the xg
    value (`_chain`), the summation order of lstm_seq_kernel."""
    whh = _a(whh, dtype)
    B, T, _ = xg.shape
    nd, H4, H = whh.shape
    lens = None if lengths is None else np.asarray(lengths).astype(np.int64)
    if lens is None:
        xg = _a(xg, dtype)
    alloc = np.empty if lens is None else np.zeros
    y = alloc((B, T, nd * H), dtype=dtype)
    gates = alloc((B, T, nd * H4), dtype=dtype)
    cs = alloc((B, T, nd * H), dtype=dtype)
    h_n = np.empty((nd, B, H), dtype=dtype)
    c_n = np.empty((nd, B, H), dtype=dtype)
    for d in range(nd):
        whhT = np.ascontiguousarray(whh[d].T)
        h = np.zeros((B, H), dtype=dtype) if h0 is None else _a(h0[d], dtype).copy()
        c = np.zeros((B, H), dtype=dtype) if c0 is None else _a(c0[d], dtype).copy()
        if lens is None:
            for t in (range(T) if d == 0 else reversed(range(T))):
                gt, c, h = _lstm_cell(xg[:, t, d * H4:(d + 1) * H4], h, c, whhT, H, chain)
                y[:, t, d * H:(d + 1) * H] = h
                cs[:, t, d * H:(d + 1) * H] = c
                gates[:, t, d * H4:(d + 1) * H4] = gt
        else:
            assert lens.shape == (B,) and lens.min(initial=0) >= 0 and lens.max(initial=0) <= T
            for s in range(int(lens.max(initial=0))):
                a = np.nonzero(lens > s)[0]   # the utterances still running; only their own rows of xg are read
                t = np.full(a.shape, s) if d == 0 else lens[a] - 1 - s
                gt, ca, ha = _lstm_cell(_a(xg[a, t, d * H4:(d + 1) * H4], dtype), h[a], c[a], whhT, H, chain)
                h[a], c[a] = ha, ca
                y[a, t, d * H:(d + 1) * H] = ha
                cs[a, t, d * H:(d + 1) * H] = ca
                gates[a, t, d * H4:(d + 1) * H4] = gt
        h_n[d], c_n[d] = h, c
    return (y, gates, cs, h_n, c_n) if return_state else (y, gates, cs)


def lstm_layer_backward(dy, gates, cs, whh, dtype=np.float64):
    """dy [B,T,ndir*H] -> dG [B,T,ndir*4H], the gradient wrt the pre-activation gates (zero final-state gradients)"""
    dy, gates, cs, whh = (_a(v, dtype) for v in (dy, gates, cs, whh))
    B, T, _ = dy.shape
    nd, H4, H = whh.shape
    dG = np.empty((B, T, nd * H4), dtype=dtype)
    for d in range(nd):
        dh_rec = np.zeros((B, H), dtype=dtype)
        dc_next = np.zeros((B, H), dtype=dtype)
        order = list(range(T)) if d == 0 else list(reversed(range(T)))
        for s in reversed(range(T)):
            t = order[s]
            gt = gates[:, t, d * H4:(d + 1) * H4]
            i, f, g, o = gt[:, :H], gt[:, H:2 * H], gt[:, 2 * H:3 * H], gt[:, 3 * H:]
            c = cs[:, t, d * H:(d + 1) * H]
            cp = cs[:, order[s - 1], d * H:(d + 1) * H] if s > 0 else np.zeros_like(c)
            dh = dy[:, t, d * H:(d + 1) * H] + dh_rec
            tc = np.tanh(c)
            do = dh * tc * o * (1 - o)
            dc = dc_next + dh * o * (1 - tc * tc)
            di = dc * g * i * (1 - i)
            dg = dc * i * (1 - g * g)
            df = dc * cp * f * (1 - f)
            dc_next = dc * f
            dGt = np.concatenate([di, df, dg, do], axis=1)
            dG[:, t, d * H4:(d + 1) * H4] = dGt
            dh_rec = dGt @ whh[d]
    return dG


def lstm_stack_grads(x, params, dy, dtype=np.float64):
    """A torch.nn.LSTM stack (batch_first, zero initial state) with loss sum(y * dy).  params: {torch parameter name: array} of
    weight_ih_l{k}[_reverse], weight_hh_l{k}[_reverse], bias_ih_l{k}[_reverse], bias_hh_l{k}[_reverse].
    -> dict y, dx, per layer 'layers': [(y, gates, c, dG)], and the gradient of every parameter under its torch name"""
    nd = 2 if any(k.endswith('_reverse') for k in params) else 1
    L = 1 + max(int(k.split('_l')[1].split('_')[0]) for k in params)
    sfx = ['', '_reverse'][:nd]
    p = {k: _a(v, dtype) for k, v in params.items()}
    h = _a(x, dtype)
    inputs, layers = [], []
    for l in range(L):
        wih = np.concatenate([p['weight_ih_l%d%s' % (l, s)] for s in sfx], axis=0)
        bias = np.concatenate([p['bias_ih_l%d%s' % (l, s)] + p['bias_hh_l%d%s' % (l, s)] for s in sfx])
        whh = np.stack([p['weight_hh_l%d%s' % (l, s)] for s in sfx])
        inputs.append(h)
        y, gates, cs = lstm_layer_forward(h @ wih.T + bias, whh, dtype)
        layers.append([y, gates, cs, None])
        h = y
    out = {'y': h}
    g = _a(dy, dtype)
    for l in reversed(range(L)):
        y, gates, cs, _ = layers[l]
        whh = np.stack([p['weight_hh_l%d%s' % (l, s)] for s in sfx])
        dG = lstm_layer_backward(g, gates, cs, whh, dtype)
        layers[l][3] = dG
        xin = inputs[l]
        B, T, _ = xin.shape
        H4 = whh.shape[1]
        H = H4 // 4
        x2 = xin.reshape(B * T, -1)
        gin = np.zeros_like(xin)
        for d, s in enumerate(sfx):
            dGd = dG[:, :, d * H4:(d + 1) * H4]
            g2 = dGd.reshape(B * T, H4)
            yd = y[:, :, d * H:(d + 1) * H]
            hprev = np.zeros_like(yd)
            if d == 0:
                hprev[:, 1:] = yd[:, :-1]
            else:
                hprev[:, :-1] = yd[:, 1:]
            out['weight_ih_l%d%s' % (l, s)] = g2.T @ x2
            out['weight_hh_l%d%s' % (l, s)] = g2.T @ hprev.reshape(B * T, H)
            out['bias_ih_l%d%s' % (l, s)] = g2.sum(axis=0)
            out['bias_hh_l%d%s' % (l, s)] = g2.sum(axis=0)
            gin += dGd @ p['weight_ih_l%d%s' % (l, s)]
        g = gin
    out['dx'] = g
    out['layers'] = [tuple(v) for v in layers]
    return out
