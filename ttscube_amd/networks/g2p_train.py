"""Training path of the word-level G2P (cube/networks/g2p.py:91-121 learn_batch, 296-351 the loop; modules.py:258-297 Seq2Seq.forward with
gs_output in train mode) on the HIP kernels.

  embeddings      HipEmbeddingFn (padding_idx = 0: the PAD row gets no gradient)
  encoder         lstm_autograd.lstm_forward_train over ALL N positions of the padded batch (no lengths, as the reference), dropout 0.33 on the
                  whole layer-0 output (ttsc_dropout_scale)
  decoder         G2pDecoderFn, ONE autograd.Function: ttsc_g2p_train_forward (the start step and all T teacher-forced steps in one launch) and
                  ttsc_g2p_train_backward (the whole backward-through-time loop in one launch); the weight gradients are GEMMs over the per-step
                  rows the backward kernel leaves (gemm_hip TN split-K, the row shift for h_prev, colsum_hip for the biases)
  logits          one hip_linear over the B * T rows of h2 (teacher forcing: the logits do not feed back)
  loss            ttsc_masked_ce(ignore_index = 0): mean over the non-PAD targets
  update          optim.FlatAdamW(weight_decay=0, betas=(0.9, 0.999)) = torch.optim.Adam's update; torch.optim.Adam itself works too
                  (`learn_batch` returns a differentiable scalar, so the reference's loop `loss.backward(); optim.step()` runs unchanged)

Dropout masks are injected (`masks`, parity tests) or drawn in the kernels from Philox, keyed by one seed per step taken from torch's CPU generator
(`torch.manual_seed` makes a run repeatable).  `Seq2Seq.forward` itself stays inference only."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..hip_layers import colsum_hip, gemm_hip, linear_hip
from .lstm_autograd import lstm_forward_train
from .phonemizer import masked_ce
from .seq2seq import pack4
from .training import StepLosses

# Philox stream id of the decoder kernels' masks (they add a tag per family: attention / inter-layer); the encoder's inter-layer dropout is another
# kernel with a tag of its own and draws stream l for layer l (lstm_autograd.lstm_forward_train)
STREAM_DEC = 2


def _seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())     # (torch's CPU generator: no device round trip)


class G2pDecoderFn(torch.autograd.Function):
    """enc [B, N, E], labels int32 [B, T] -> h2 [B, T, D] of the teacher-forced attention decoder (start step included).
    att_mask [B, T, N, A] / dec_mask [B, T + 1, D]: {0,1} floats or None (Philox(seed) when the probability is above 0)."""

    @staticmethod
    def forward(ctx, enc, y, att_mask, dec_mask, seed, p_att, p_dec, w_att, b_att, v, out_emb, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1):
        dev = enc.device
        g = lambda t: t.detach().float()
        enc = g(enc).contiguous()
        B, N, E = enc.shape
        T = y.shape[1]
        D = w_hh0.shape[1]
        w_att2 = g(w_att)[:, :, 0]                                   # [A, D + E], hidden columns first
        A = w_att2.shape[0]
        L, Em = out_emb.shape
        if w_att.shape[2] != 1 or w_att2.shape[1] != D + E or w_ih0.shape[1] != E + Em or D % 4 or E % 4 or A % 4:
            raise _lib.TTSCError('G2pDecoderFn: sizes do not fit (attention [A, D + E, 1], decoder input E + Em; D, E, A multiples of 4)')
        w_ih0, w_hh0, w_ih1, w_hh1, v, out_emb = g(w_ih0), g(w_hh0), g(w_ih1), g(w_hh1), g(v).contiguous(), g(out_emb).contiguous()
        w_pe = w_att2[:, D:].contiguous()
        pe = linear_hip(enc, w_pe, g(b_att))                         # hoisted: does not depend on the recurrence
        tab = linear_hip(out_emb, w_ih0[:, E:].contiguous())         # the fed-back embedding as one row lookup
        R = T + 1
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        x0 = torch.zeros((B, R, E + Em), dtype=torch.float32, device=dev)
        L_ = _lib.lib()
        if T > 1:                                                    # row t + 1 takes output_emb(y[:, t - 1]); an id outside the table gives zeros
            yp = y[:, :T - 1].contiguous()
            emb = f(B * (T - 1), Em)
            with _lib.on_device(dev):
                _lib.check(L_.ttsc_rows_gather(_lib.dev_ptr(out_emb), _lib.dev_ptr(yp), _lib.dev_ptr(emb), B * (T - 1), Em, L, _lib.current_stream()),
                           'ttsc_rows_gather')
            x0[:, 2:, E:] = emb.view(B, T - 1, Em)
        sv = dict(gates0=f(B, R, 4 * D), cells0=f(B, R, D), h1=f(B, R, D), h1m=f(B, R, D), gates1=f(B, R, 4 * D), cells1=f(B, R, D), h2=f(B, R, D),
                  aq=f(B, T, A), att=f(B, T, N))
        scratch = f(B, 2, N)
        b0, b1 = (g(b_ih0) + g(b_hh0)).contiguous(), (g(b_ih1) + g(b_hh1)).contiguous()
        am = att_mask.float().contiguous() if att_mask is not None else None
        dm = dec_mask.float().contiguous() if dec_mask is not None else None
        if am is not None and tuple(am.shape) != (B, T, N, A) or dm is not None and tuple(dm.shape) != (B, R, D):
            raise _lib.TTSCError('G2pDecoderFn: attention masks must be [B, T, N, A] and decoder masks [B, T + 1, D]')
        fw = dict(w_aq=pack4(w_att2[:, :D]), w_ic=pack4(w_ih0[:, :E]), w_hh0=pack4(w_hh0), w_ih1=pack4(w_ih1), w_hh1=pack4(w_hh1))
        a = _lib.G2pTrainArgs()
        P = lambda t: t.data_ptr() if t is not None else None
        for k, t in dict(enc_dev=enc, pe_dev=pe, y_dev=y, v=v, tab=tab, b0=b0, b1=b1, att_mask_dev=am, dec_mask_dev=dm, x0_dev=x0, scratch_dev=scratch,
                         **fw, **{k + '_dev': t for k, t in sv.items()}).items():
            setattr(a, k, P(t))
        a.seed, a.stream_id = int(seed), STREAM_DEC
        a.B, a.N, a.T, a.E, a.A, a.D, a.L, a.Em = B, N, T, E, A, D, L, Em
        a.p_att, a.p_dec = float(p_att), float(p_dec)
        with _lib.on_device(dev):
            _lib.check(L_.ttsc_g2p_train_forward(C.byref(a), _lib.current_stream()), 'ttsc_g2p_train_forward')
        ctx.save_for_backward(enc, pe, y, v, tab, b0, b1, x0, w_att2, w_ih0, w_hh0, w_ih1, w_hh1, *[sv[k] for k in sorted(sv)])
        ctx.masks = (am, dm)
        ctx.fw = fw
        ctx.dims = (B, N, T, E, A, D, L, Em, int(seed), float(p_att), float(p_dec))
        return sv['h2'][:, 1:].contiguous()

    @staticmethod
    def backward(ctx, dh2):
        enc, pe, y, v, tab, b0, b1, x0, w_att2, w_ih0, w_hh0, w_ih1, w_hh1, *rest = ctx.saved_tensors
        B, N, T, E, A, D, L, Em, seed, p_att, p_dec = ctx.dims
        sv = dict(zip(sorted(['gates0', 'cells0', 'h1', 'h1m', 'gates1', 'cells1', 'h2', 'aq', 'att']), rest))
        am, dm = ctx.masks
        dev = enc.device
        R = T + 1
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        dh2 = dh2.contiguous().float()
        dG0, dG1, denc, dpe, dvp, scratch = f(B, R, 4 * D), f(B, R, 4 * D), f(B, N, E), f(B, N, A), f(B, A), f(B, 2, N)
        dq = torch.zeros((B, R, A), dtype=torch.float32, device=dev)
        bw = dict(w_l1t=pack4(torch.cat([w_ih1.t(), w_hh1.t()], dim=0)), w_l0t=pack4(torch.cat([w_hh0.t(), w_ih0[:, :E].t()], dim=0)),
                  w_aqt=pack4(w_att2[:, :D].t()))
        a = _lib.G2pTrainArgs()
        P = lambda t: t.data_ptr() if t is not None else None
        for k, t in dict(enc_dev=enc, pe_dev=pe, y_dev=y, v=v, tab=tab, b0=b0, b1=b1, att_mask_dev=am, dec_mask_dev=dm, x0_dev=x0, scratch_dev=scratch,
                         dh2_dev=dh2, dgates0_dev=dG0, dgates1_dev=dG1, dq_dev=dq, denc_dev=denc, dpe_dev=dpe, dv_dev=dvp,
                         **ctx.fw, **bw, **{k + '_dev': t for k, t in sv.items()}).items():
            setattr(a, k, P(t))
        a.seed, a.stream_id = seed, STREAM_DEC
        a.B, a.N, a.T, a.E, a.A, a.D, a.L, a.Em = B, N, T, E, A, D, L, Em
        a.p_att, a.p_dec = p_att, p_dec
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ttsc_g2p_train_backward(C.byref(a), _lib.current_stream()), 'ttsc_g2p_train_backward')
        g0, g1 = dG0.view(B * R, 4 * D), dG1.view(B * R, 4 * D)
        # the start step is row 0 of a period-(T + 1) sequence: its predecessor is the zero state (the row shift reads zeros there)
        tn = lambda dg, rows, shift=0: gemm_hip(dg, rows, trans_a=True, b_row_shift=shift, b_period=R if shift else 0)
        d_wih0 = tn(g0, x0.view(B * R, E + Em))
        d_whh0 = tn(g0, sv['h1'].view(B * R, D), -1)
        d_wih1 = tn(g1, sv['h1m'].view(B * R, D))
        d_whh1 = tn(g1, sv['h2'].view(B * R, D), -1)
        d_b0, d_b1 = colsum_hip(g0), colsum_hip(g1)
        # attention: the query of step t is the CELL state of row t (= step t - 1); pe = enc . W_pe^T + b
        d_waq = tn(dq.view(B * R, A), sv['cells1'].view(B * R, D), -1)
        dpe2, enc2 = dpe.view(B * N, A), enc.view(B * N, E)
        d_wpe = tn(dpe2, enc2)
        d_watt = torch.cat([d_waq, d_wpe], dim=1).unsqueeze(2)
        d_batt = colsum_hip(dpe2)
        gemm_hip(dpe2, w_att2[:, D:], out=denc.view(B * N, E), accumulate=True)             # d enc += d pe . W_pe
        d_v = colsum_hip(dvp)
        # the fed-back embedding: d emb = d g0 . W_ih0[:, E:], then the gather's adjoint on y shifted by one step (PAD excluded)
        if T > 1:
            demb = gemm_hip(g0, w_ih0[:, E:]).view(B, R, Em)[:, 2:].contiguous()
            d_emb = f(L, Em)
            yp = y[:, :T - 1].contiguous()
            with _lib.on_device(dev):
                _lib.check(_lib.lib().ttsc_rows_scatter_add(_lib.dev_ptr(demb), _lib.dev_ptr(yp), _lib.dev_ptr(d_emb), B * (T - 1), Em, L, 0,
                                                            _lib.current_stream()), 'ttsc_rows_scatter_add')
        else:
            d_emb = torch.zeros((L, Em), dtype=torch.float32, device=dev)
        return (denc if ctx.needs_input_grad[0] else None, None, None, None, None, None, None, d_watt, d_batt, d_v, d_emb, d_wih0, d_whh0, d_b0,
                d_b0.clone(), d_wih1, d_whh1, d_b1, d_b1.clone())


def _decoder_masks(masks, B, T, dev):
    """{'init': [B, 1, D], 'att': T x [B, N, A], 'dec': T x [B, 1, D]} -> ([B, T, N, A], [B, T + 1, D]) on the device"""
    if masks is None:
        return None, None
    am = dm = None
    if masks.get('att') is not None:
        am = torch.stack([m.to(dev).float() for m in masks['att']], dim=1).contiguous()
    if masks.get('dec') is not None:
        rows = [masks['init']] + list(masks['dec'])
        dm = torch.cat([m.to(dev).float().reshape(B, 1, -1) for m in rows], dim=1).contiguous()
    return am, dm


def decoder_forward_train(net, enc, y, masks=None, seed=None):
    """encoder states [B, N, E] (differentiable), labels [B, T] -> differentiable logits [B, T, L]"""
    from .text_autograd import hip_linear
    if not enc.is_cuda:
        raise _lib.TTSCError('G2P training needs a HIP device; no CPU path')
    if net.decoder.num_layers != 2:
        raise _lib.TTSCError('G2P training runs a 2-layer decoder (got %d layers)' % net.decoder.num_layers)
    B, T = y.shape
    y32 = y.to(enc.device).to(torch.int32).contiguous()
    am, dm = _decoder_masks(masks, B, T, enc.device)
    on = net.training
    d = net.decoder
    h2 = G2pDecoderFn.apply(enc, y32, am, dm, _seed() if seed is None else seed, float(net.attention.dropout_prob) if on else 0.0,
                            float(d.dropout) if on else 0.0, net.attention.attn.conv.weight, net.attention.attn.conv.bias, net.attention.v,
                            net.output_emb.weight, d.weight_ih_l0, d.weight_hh_l0, d.bias_ih_l0, d.bias_hh_l0, d.weight_ih_l1, d.weight_hh_l1,
                            d.bias_ih_l1, d.bias_hh_l1)
    return hip_linear(h2, net.output.weight, net.output.bias)


def seq2seq_forward_train(net, x, y, masks=None):
    """Differentiable Seq2Seq.forward(x, gs_output=y) (modules.py:258-297): token ids [B, N], labels [B, T] -> logits [B, T, L].
    masks: optional dict {'enc': [B, N, 2H], 'init': [B, 1, D], 'att': T x [B, N, A], 'dec': T x [B, 1, D]} of {0,1} tensors (parity tests);
    without it the masks are drawn in the kernels.  In eval mode nothing drops out."""
    from .text_autograd import hip_embedding
    dev = net._get_device()
    if not x.is_cuda or not y.is_cuda:
        raise _lib.TTSCError('seq2seq_forward_train: token ids and labels must live on a HIP device; no CPU path')
    seed = _seed()
    emb = hip_embedding(net.input_emb, x)
    enc_masks = [masks['enc'].to(dev)] if masks is not None and masks.get('enc') is not None else None
    enc = lstm_forward_train(net.encoder, emb, dropout_masks=enc_masks, dropout_seed=seed)
    return decoder_forward_train(net, enc, y, masks, seed)


def g2p_loss(logits, y):
    """CrossEntropyLoss(ignore_index=0) of g2p.py:32,121 over [B * T, L] on ttsc_masked_ce: mean over the non-PAD targets (0 when there is none)"""
    return masked_ce(logits.reshape(logits.shape[0] * logits.shape[1], -1), y.reshape(-1), 0)[0]


def make_batch(g2p, batch):
    """g2p.py:92-119: x padded to the longest word + 1, y to the longest transcription + 1, <EOS> then <PAD> -> int64 arrays"""
    t2i, l2i = g2p.token2int, g2p.label2int
    x = np.full((len(batch), max(len(ex[0]) for ex in batch) + 1), t2i['<PAD>'], dtype=np.int64)
    y = np.full((len(batch), max(len(ex[1]) for ex in batch) + 1), l2i['<PAD>'], dtype=np.int64)
    for i, (word, trans) in enumerate(batch):
        for j, ch in enumerate(word):
            x[i, j] = t2i.get(ch.lower(), t2i['<UNK>'])
        x[i, len(word)] = t2i['<EOS>']
        for j, ph in enumerate(trans):
            y[i, j] = l2i.get(ph, l2i['<UNK>'])
        y[i, len(trans)] = l2i['<EOS>']
    return x, y


def learn_batch(g2p, batch, masks=None):
    """G2P.learn_batch (g2p.py:91-121): a list of (word, phones) -> the scalar loss tensor; `loss.backward()` fills every Seq2Seq parameter's
    gradient, so the reference's own loop with torch.optim.Adam works on it"""
    dev = g2p._get_device()
    x, y = make_batch(g2p, batch)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    return g2p_loss(seq2seq_forward_train(g2p.seq2seq, x, y, masks), y)


def g2p_configure_optimizer(g2p, lr=1e-3):
    """g2p.py:312: Adam(lr) over every Seq2Seq parameter, as optim.FlatAdamW(weight_decay=0, betas=(0.9, 0.999)) — torch.optim.Adam's update"""
    from ..optim import FlatAdamW
    g2p._get_device()
    return FlatAdamW(list(g2p.seq2seq.parameters()), lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


def g2p_training_step(g2p, batch, opt, masks=None):
    """forward, loss, backward and the Adam update of one batch -> training.StepLosses {'loss'}; the value is read back when somebody looks.
    Labels outside the table are reported by seq2seq.check_status (the trainer asks once per epoch)."""
    opt.zero_grad()
    loss = learn_batch(g2p, batch, masks)
    loss.backward()
    opt.step()
    val = loss.detach()
    return StepLosses(lambda: {'loss': float(val)})
