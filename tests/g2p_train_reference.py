"""Test helper: the teacher-forced G2P training forward (Seq2Seq.forward(x, gs_output=y) in train mode) in plain torch ops, at any dtype and on
any device, with INJECTED dropout masks — differentiable by autograd.  Written from the description of the computation, not from the
reference's code:

  emb = input_emb[x]                                        (PAD row: no gradient)
  encoder: 2-layer BiLSTM over all N positions, zero initial state; the whole layer-0 output [B, N, 2H] times mask / (1 - p_enc)
  start state: one decoder step on a zero input from a zero state, layer 0's h times mask / (1 - p_dec) on its way into layer 1
  per step t: q = CELL state of the top decoder layer; energy_j = tanh(W_att [q; enc_j] + b) times mask / (1 - p_att);
              a = softmax_j(v . energy_j) over all N; ctx = sum_j a_j enc_j; decoder input [ctx; emb_prev] (emb_prev = 0 at t = 0, else
              output_emb[y[:, t - 1]]); two LSTM layers, one step, a fresh mask on layer 0's h; logits_t = W_out h2 + b
  loss = mean over the targets != 0 of the cross-entropy

`P` maps the Seq2Seq state_dict keys to tensors (leaves that require grad, for the gradient checks).  masks = {'enc': [B, N, 2H], 'init':
[B, 1, D], 'att': T x [B, N, A], 'dec': T x [B, 1, D]}; a missing entry (or masks=None) means "nothing dropped, no scaling"."""
import torch
import torch.nn.functional as F

P_ENC, P_DEC, P_ATT = 0.33, 0.33, 0.1


def _cell(x_gates, h, c, w_hh):
    """one LSTM step from the input's share of the gates (biases included); gate order i, f, g, o"""
    g = x_gates + h @ w_hh.t()
    i, f, gg, o = g.chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, N, _ = x.shape
    H = w_hh.shape[1]
    xg = x @ w_ih.t() + (b_ih + b_hh)
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    out = [None] * N
    for t in (range(N - 1, -1, -1) if reverse else range(N)):
        h, c = _cell(xg[:, t], h, c, w_hh)
        out[t] = h
    return torch.stack(out, dim=1)


def _drop(t, mask, p):
    if mask is None:
        return t
    return t * (mask.to(t.device).to(t.dtype).reshape(t.shape) / (1.0 - p))


def bilstm_reference(P, prefix, x, layers=2, masks=None, p=P_ENC):
    """stacked BiLSTM `prefix` ('encoder.') over x [B, N, in]; masks: one per layer but the last, or None"""
    h = x
    for l in range(layers):
        outs = []
        for sfx, rev in (('', False), ('_reverse', True)):
            k = lambda n: P['%s%s_l%d%s' % (prefix, n, l, sfx)]
            outs.append(_lstm_direction(h, k('weight_ih'), k('weight_hh'), k('bias_ih'), k('bias_hh'), rev))
        h = torch.cat(outs, dim=-1)
        if l < layers - 1 and masks is not None and masks[l] is not None:
            h = _drop(h, masks[l], p)
    return h


def _decoder_step(P, inp, state, mask, p_dec):
    (h1, c1), (h2, c2) = state
    k = lambda n: P['decoder.' + n]
    h1, c1 = _cell(inp @ k('weight_ih_l0').t() + (k('bias_ih_l0') + k('bias_hh_l0')), h1, c1, k('weight_hh_l0'))
    h1d = _drop(h1, mask, p_dec)
    h2, c2 = _cell(h1d @ k('weight_ih_l1').t() + (k('bias_ih_l1') + k('bias_hh_l1')), h2, c2, k('weight_hh_l1'))
    return (h1, c1), (h2, c2)


def decoder_reference(P, enc, y, masks=None, p_att=P_ATT, p_dec=P_DEC):
    """encoder states [B, N, E], labels int64 [B, T] -> logits [B, T, L]"""
    masks = masks or {}
    B, N, E = enc.shape
    T = y.shape[1]
    D = P['decoder.weight_hh_l0'].shape[1]
    Em = P['output_emb.weight'].shape[1]
    w_att = P['attention.attn.conv.weight'][:, :, 0]                # [A, D + E]: query columns first
    z = lambda n: enc.new_zeros(B, n)
    state = _decoder_step(P, z(E + Em), ((z(D), z(D)), (z(D), z(D))), masks.get('init'), p_dec)
    pe = enc @ w_att[:, D:].t() + P['attention.attn.conv.bias']      # [B, N, A]
    emb_prev = z(Em)
    logits = []
    for t in range(T):
        q = state[1][1]                                              # the CELL state of the top layer
        energy = torch.tanh((q @ w_att[:, :D].t())[:, None, :] + pe)
        energy = _drop(energy, masks['att'][t] if masks.get('att') is not None else None, p_att)
        a = torch.softmax(energy @ P['attention.v'], dim=1)          # over all N positions
        ctx = (a[:, :, None] * enc).sum(dim=1)
        state = _decoder_step(P, torch.cat([ctx, emb_prev], dim=1), state, masks['dec'][t] if masks.get('dec') is not None else None, p_dec)
        logits.append(state[1][0] @ P['output.weight'].t() + P['output.bias'])
        emb_prev = F.embedding(y[:, t], P['output_emb.weight'], padding_idx=0)
    return torch.stack(logits, dim=1)


def seq2seq_reference(P, x, y, masks=None, p_enc=P_ENC, p_att=P_ATT, p_dec=P_DEC):
    """token ids [B, N], labels [B, T] -> logits [B, T, L]"""
    masks = masks or {}
    emb = F.embedding(x, P['input_emb.weight'], padding_idx=0)
    enc = bilstm_reference(P, 'encoder.', emb, 2, [masks.get('enc')], p_enc)
    return decoder_reference(P, enc, y, masks, p_att, p_dec)


def loss_reference(logits, y):
    """mean cross-entropy over the targets != 0"""
    return F.cross_entropy(logits.reshape(-1, logits.shape[-1]), y.reshape(-1), ignore_index=0)


def leaves(sd, dtype=torch.float64, device='cpu'):
    """state_dict -> {key: leaf tensor that requires grad} at `dtype`"""
    return {k: v.detach().to(device).to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
