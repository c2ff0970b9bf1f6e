"""Training path of `CubenetTextcoder` (cube/networks/textcoder.py:101-138, 191-270) on the HIP kernels.

  teacher-forced forward    embeddings / char-CNN / Linears (text_autograd.py), the five LSTMs over the padded batch WITHOUT lengths
                            (lstm_autograd.py, as torch.nn.LSTM runs them in the reference), the `_expand` row gather (HipEmbeddingFn on a
                            non-decreasing flat index: ordered backward), PreNet = hip_linear -> relu -> x 2 mask, PostNet = 4 x [TrainConv k5 ->
                            ttsc_bn_tanh_dropout_train_forward] + TrainConv k5 (BatchNorm batch statistics, running statistics, dropout 0.1)
  losses                    ttsc_textcoder_loss: two cross-entropies with ignore_index + two mel L1 terms, values and gradients in one launch
  update                    optim.FlatAdamW(weight_decay=0, betas=(0.9, 0.999)): torch.optim.Adam's update (what configure_optimizers returns)

The step returns training.StepLosses: the values (and the loss kernel's target-range status) travel to page-locked memory in one asynchronous copy
and are read when first looked at."""
import torch

from .. import _lib
from .lstm_autograd import lstm_forward_train
from .training import StepLosses, _h2d, _require_device


# ---- PostNet in training mode -----------------------------------------------------------------------------------------------------
class BnTanhDropoutFn(torch.autograd.Function):
    """y = dropout(tanh(BatchNorm1d(x))) over x [B, C, F] in training mode (modules.py:121-140): batch statistics, running statistics updated in
    place, dropout mask injected ({0,1}, same shape as x) or drawn in-kernel from Philox (seed, layer)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, mask, seed, layer, momentum, eps, p):
        x = x.contiguous()
        B, C_, F_ = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(C_, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        m = mask.contiguous().float() if mask is not None else None
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_bn_tanh_dropout_train_forward(
                _lib.dev_ptr(x), _lib.dev_ptr(g), _lib.dev_ptr(b), _lib.dev_ptr(running_mean), _lib.dev_ptr(running_var), B, C_, F_, float(momentum),
                float(eps), float(p), _lib.dev_ptr(m) if m is not None else None, int(seed), int(layer), _lib.dev_ptr(y), _lib.dev_ptr(mean),
                _lib.dev_ptr(invstd), _lib.current_stream()), 'ttsc_bn_tanh_dropout_train_forward')
        ctx.save_for_backward(x, g, b, mean, invstd, m)
        ctx.seed, ctx.layer, ctx.p = int(seed), int(layer), float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, b, mean, invstd, m = ctx.saved_tensors
        B, C_, F_ = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg = torch.empty_like(g)
        db = torch.empty_like(b)
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_bn_tanh_dropout_train_backward(
                _lib.dev_ptr(dy), _lib.dev_ptr(x), _lib.dev_ptr(g), _lib.dev_ptr(b), _lib.dev_ptr(mean), _lib.dev_ptr(invstd), B, C_, F_, ctx.p,
                _lib.dev_ptr(m) if m is not None else None, ctx.seed, ctx.layer, _lib.dev_ptr(dx), _lib.dev_ptr(dg), _lib.dev_ptr(db),
                _lib.current_stream()), 'ttsc_bn_tanh_dropout_train_backward')
        return dx, dg, db, None, None, None, None, None, None, None, None


def _seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())     # (torch's CPU generator: no device round trip)


def postnet_train(net, mel, masks=None):
    """mel [B, F, 80] -> mel + PostNet(mel) (textcoder.py:135-136) with BatchNorm in training mode.  masks: optional list of four {0,1} tensors
    [B, 512, F] (the Dropout(0.1) masks, parity tests); otherwise drawn in-kernel."""
    from ..hifigan.autograd import TrainConv, hip_conv
    pn = net._postnet
    cache = net.__dict__.setdefault('_train_postnet', {})
    h = mel.permute(0, 2, 1).contiguous()
    for i in range(5):
        c = pn.network[4 * i].conv
        tc = cache.get(i)
        if tc is None:
            tc = cache[i] = TrainConv(c.in_channels, c.out_channels, c.kernel_size[0], padding=c.padding[0], dilation=c.dilation[0])
        h = hip_conv(tc, h, c.weight, c.bias)
        if i == 4:
            break
        bn, drop = pn.network[4 * i + 1], pn.network[4 * i + 3]
        h = BnTanhDropoutFn.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, None if masks is None else masks[i], _seed(), i,
                                  bn.momentum, bn.eps, drop.p)
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
    return mel + h.permute(0, 2, 1)


def prenet_train(net, x, masks=None):
    """PreNet (modules.py:148-164): 2 x [Linear -> relu -> dropout(0.5, always on)]; masks: optional two {0,1} tensors broadcastable to [B, T, 256]"""
    from .text_autograd import hip_linear
    h = x
    for i, layer in enumerate(net._prenet.layers_h):
        h = torch.relu(hip_linear(h, layer.linear_layer.weight, layer.linear_layer.bias))
        m = masks[i].to(h.device).float() if masks is not None else (torch.rand(h.shape, device=h.device) >= 0.5).float()
        h = h * (m * 2.0)
    return h


def expand_index(alignments, pframes, n_rows):
    """The row index of textcoder.py:291-302 (`_expand`): position jj < len(a) // pframes takes phoneme a[jj * pframes]; the positions beyond an
    utterance's own length take the LAST ROW OF THE PADDED phoneme tensor (x[ii, -1], index n_rows - 1) — for every pframes, 1 included (this is not
    Languasito2's a[-1] rule of modules._expand_rows).  -> int64 [B, m] (non-decreasing per row)."""
    m = max(len(a) // pframes for a in alignments)
    idx = torch.full((len(alignments), m), n_rows - 1, dtype=torch.long)
    for b, a in enumerate(alignments):
        k = len(a) // pframes
        if k:
            idx[b, :k] = torch.as_tensor(list(a), dtype=torch.long)[0:k * pframes:pframes]
    return idx


def textcoder_forward_train(net, X, masks=None):
    """Differentiable CubenetTextcoder.forward (textcoder.py:101-138): (output_dur [B, N, D+1], output_pitch [B, m, P+1], output_mel [B, 3m', 80],
    output_mel_post).  masks: optional dict {'prenet': [m0, m1] ([B, T, 256] {0,1}), 'postnet': [four [B, 512, F] {0,1}]} for parity tests.
    In eval mode (validation) the PostNet takes its folded running-statistics kernel, as the reference's module does; the PreNet drops out anyway."""
    from .text_autograd import HipEmbeddingFn, char_cnn_train, hip_embedding, hip_linear
    masks = masks or {}
    dev = net._get_device()
    x_char, x_speaker = _h2d(X, 'x_char', dev), _h2d(X, 'x_speaker', dev)
    _require_device(x_char, 'textcoder_forward_train')
    pf = net._pframes
    B, N = x_char.shape
    h = hip_embedding(net._phon_emb, x_char).permute(0, 2, 1)
    h = char_cnn_train(net, '_char_cnn', h)
    h = lstm_forward_train(net._rnn_char, h.permute(0, 2, 1))
    spk = hip_embedding(net._speaker_emb, x_speaker)
    h = torch.cat([h, spk.repeat(1, h.shape[1], 1)], dim=-1)
    out_dur = hip_linear(lstm_forward_train(net._dur_rnn, h), net._dur_output.linear_layer.weight, net._dur_output.linear_layer.bias)
    idx = expand_index(X['y_frame2phone'], pf, N)
    flat = (idx + torch.arange(B, dtype=torch.long)[:, None] * N).to(dev, non_blocking=True)
    C_ = h.shape[2]
    h = HipEmbeddingFn.apply(h.reshape(B * N, C_), flat, None, True).reshape(B, idx.shape[1], C_)
    h = lstm_forward_train(net._rnn_overlay, h)
    out_pitch = hip_linear(lstm_forward_train(net._pitch_rnn, h), net._pitch_output.linear_layer.weight, net._pitch_output.linear_layer.bias)
    y_mgc = _h2d(X, 'y_mgc', dev).float()
    cond = torch.cat([torch.full((B, 1, y_mgc.shape[2]), -5.0, device=dev), y_mgc[:, pf - 1::pf][:, :y_mgc.shape[1] // pf]], dim=1)
    cond = prenet_train(net, cond, masks.get('prenet'))
    m = min(h.shape[1], cond.shape[1])
    hm = lstm_forward_train(net._mel_rnn, torch.cat([h[:, :m], cond[:, :m]], dim=-1))
    mel = hip_linear(hm, net._mel_output.linear_layer.weight, net._mel_output.linear_layer.bias).reshape(B, -1, 80)
    if net._postnet.training:
        post = postnet_train(net, mel, masks.get('postnet'))
    else:
        post = net._postnet(mel, add_residual=True)
    return out_dur, out_pitch, mel, post


# ---- the loss -------------------------------------------------------------------------------------------------------------------
class TextcoderLossFn(torch.autograd.Function):
    """[loss_duration, loss_pitch, l1(pre, t), l1(post, t)] and the kernel's status word (1: a duration target, 2: a pitch target outside
    [0, classes) that is not ignore_index).  Inputs are the trimmed tensors: logits [R, K], targets int64 [R], mel [B, m, 80]."""

    @staticmethod
    def forward(ctx, p_dur, p_pitch, pre, post, t_dur, t_pitch, t_mel, ignore_index):
        dev = pre.device
        ld, lp = p_dur.detach().contiguous().float(), p_pitch.detach().contiguous().float()
        a, b, t = pre.detach().contiguous(), post.detach().contiguous(), t_mel.contiguous().float()
        td, tp = t_dur.contiguous().long(), t_pitch.contiguous().long()
        Rd, Kd = ld.shape
        Rp, Kp = lp.shape
        n = a.numel()
        gd, gp, ga, gb = torch.empty_like(ld), torch.empty_like(lp), torch.empty_like(a), torch.empty_like(b)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        L = _lib.lib()
        ws = torch.empty(int(L.ttsc_textcoder_loss_workspace_bytes(Rd, Rp, n)), dtype=torch.uint8, device=dev)
        P = lambda x: _lib.dev_ptr(x) if x.numel() else None
        with _lib.on_device(dev):
            _lib.check(L.ttsc_textcoder_loss(P(ld), P(td), Rd, Kd, P(lp), P(tp), Rp, Kp, _lib.dev_ptr(a), _lib.dev_ptr(b), _lib.dev_ptr(t), n,
                                             int(ignore_index), _lib.dev_ptr(out), P(gd), P(gp), _lib.dev_ptr(ga), _lib.dev_ptr(gb),
                                             _lib.dev_ptr(status), _lib.dev_ptr(ws), ws.numel(), _lib.current_stream()), 'ttsc_textcoder_loss')
        ctx.save_for_backward(gd, gp, ga, gb)
        ctx.mark_non_differentiable(status)
        return out, status

    @staticmethod
    def backward(ctx, g_out, _g_status):
        gd, gp, ga, gb = ctx.saved_tensors
        return gd * g_out[0], gp * g_out[1], ga * g_out[2], gb * g_out[3], None, None, None, None


def prepare_pitch(y_pitch, pframes):
    """textcoder.py:309-314: the pitch of frame (i + 1) * pframes - 1 for i < T // pframes"""
    return y_pitch[:, pframes - 1::pframes][:, :y_pitch.shape[1] // pframes]


def textcoder_losses(p_dur, p_pitch, pre_mel, post_mel, t_dur, t_pitch, t_mel, ignore_index, check=False):
    """textcoder.py:197-215 on ttsc_textcoder_loss: the three `min` trims, CE(duration) and CE(pitch) with ignore_index (mean over the
    non-ignored rows), L1(pre) + L1(post) (plain means, padding included).  t_pitch is already `_prepare_pitch`-ed.
    -> (loss_duration, loss_pitch, loss_mel, status); check=True waits for the status word and raises TTSCError on an out-of-range target."""
    m = min(t_dur.shape[1], p_dur.shape[1])
    pd, td = p_dur[:, :m].reshape(-1, p_dur.shape[2]), t_dur[:, :m].reshape(-1)
    m = min(t_pitch.shape[1], p_pitch.shape[1])
    pp, tp = p_pitch[:, :m].reshape(-1, p_pitch.shape[2]), t_pitch[:, :m].reshape(-1)
    m = min(pre_mel.shape[1], t_mel.shape[1])
    vals, status = TextcoderLossFn.apply(pd, pp, pre_mel[:, :m], post_mel[:, :m], td, tp, t_mel[:, :m], int(ignore_index))
    if check:
        raise_on_status(int(status.item()))
    return vals[0], vals[1], vals[2] + vals[3], status


def raise_on_status(st):
    if st:
        which = ' and '.join(n for bit, n in ((1, 'duration'), (2, 'pitch')) if st & bit)
        raise _lib.TTSCError('ttsc_textcoder_loss: a %s target lies outside [0, classes) and is not the ignore index' % which)


def _ignore_index(net):
    e = net._encodings
    return int(max(e.max_pitch, e.max_duration) + 1)


def _targets(net, batch, dev):
    t_dur = _h2d(batch, 'y_dur', dev)
    t_pitch = prepare_pitch(_h2d(batch, 'y_pitch', dev), net._pframes)
    return t_dur, t_pitch, _h2d(batch, 'y_mgc', dev).float()


_HOST_SLOTS = []


def _send(values, status, words, names):
    """values (device scalars), the loss status and the split-recurrence status -> page-locked memory in one asynchronous copy -> StepLosses"""
    if not _HOST_SLOTS:
        _HOST_SLOTS.extend([[torch.zeros(8, dtype=torch.float32).pin_memory(), None] for _ in range(4)])
    slot = _HOST_SLOTS.pop(0)
    _HOST_SLOTS.append(slot)
    if slot[1] is not None and slot[1].pending:
        slot[1].wait()          # (a result nobody looked at for four steps: its copy finished long ago; a tripped status must not get lost)
    host = slot[0][:len(values) + 2]
    host.copy_(torch.cat([torch.stack([v.detach().float().reshape(()) for v in values]), status.float(), words[:1].float()]), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()

    def fetch():
        ev.synchronize()
        v = host.tolist()
        raise_on_status(int(v[len(values)]))
        if int(v[len(values) + 1]):
            raise _lib.TTSCError('textcoder_training_step: a split LSTM recurrence aborted on a hand-off timeout; the update was skipped on the '
                                 'device (TTSC_LSTM_SPLIT=1 selects the single-workgroup kernels)')
        return dict(zip(names, v[:len(values)]))
    slot[1] = StepLosses(fetch)
    return slot[1]


def textcoder_configure_optimizers(net):
    """textcoder.py:269-270: Adam(lr) over every parameter, as optim.FlatAdamW(weight_decay=0, betas=(0.9, 0.999)) — torch.optim.Adam's update;
    restores a `.opt.last` state queued in `net._loaded_optimizer_state`"""
    from ..optim import FlatAdamW
    ps = list(net.parameters())
    for p_ in ps:
        _require_device(p_, 'textcoder_configure_optimizers')
    opt = FlatAdamW(ps, net._lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    st = getattr(net, '_loaded_optimizer_state', None)
    if st is not None:
        opt.load_state_dict(st)
        net._loaded_optimizer_state = None
    return opt


def textcoder_training_step(net, batch, opt, masks=None):
    """textcoder.py:191-226: forward, losses, backward, Adam.  The update skips itself on the device when a split recurrence timed out or a target
    was out of range; both raise TTSCError when the returned StepLosses is looked at."""
    dev = net._get_device()
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    opt.zero_grad()
    p_dur, p_pitch, pre, post = textcoder_forward_train(net, batch, masks)
    t_dur, t_pitch, t_mel = _targets(net, batch, dev)
    l_dur, l_pitch, l_mel, status = textcoder_losses(p_dur, p_pitch, pre, post, t_dur, t_pitch, t_mel, _ignore_index(net))
    loss = l_dur + l_pitch + l_mel
    loss.backward()
    if _lib.lib().ttsc_split_status_collect(_lib.current_stream(), words[0:1].data_ptr(), 0) < 0:
        raise _lib.TTSCError('ttsc_split_status_collect: %s' % _lib.lib().ttsc_last_error().decode())
    opt.step(guard=torch.bitwise_or(words[0:1], status))
    return _send([loss, l_mel, l_pitch, l_dur], status, words, ('loss', 'l_mel', 'l_pitch', 'l_dur'))


def textcoder_validation_step(net, batch):
    """textcoder.py:228-251 (Lightning runs it in eval mode with no grad: the PostNet uses its running statistics and no dropout, the PreNet still
    drops out); the forward is the training composition (no lengths, the `_expand` rule of the reference) -> dict of floats"""
    dev = net._get_device()
    with torch.no_grad():
        p_dur, p_pitch, pre, post = textcoder_forward_train(net, batch)
        t_dur, t_pitch, t_mel = _targets(net, batch, dev)
        l_dur, l_pitch, l_mel, status = textcoder_losses(p_dur, p_pitch, pre, post, t_dur, t_pitch, t_mel, _ignore_index(net))
        vals = torch.cat([torch.stack([l_dur + l_pitch + l_mel, l_mel, l_pitch, l_dur]), status.float()]).tolist()   # ONE read-back
    raise_on_status(int(vals[4]))
    return dict(zip(('loss', 'l_mel', 'l_pitch', 'l_dur'), vals[:4]))
