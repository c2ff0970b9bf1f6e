"""Mirror of cube/networks/phonemizer.py:12-103: ``CubenetPhonemizer`` — the character tagger behind ``Text2FeatBlizzard`` (one phoneme tag, or
'_', per character of the sentence).  Same constructor and state_dict keys; torch modules are parameter containers only.

  tag(X, lengths)   the runtime path, tags on the device: ttsc_char_features (both embeddings, concat, permute, length mask in one launch) ->
                    3 x tanh(Conv1d k3) on Conv1dHip -> 2-layer BiLSTM on LSTMHip -> ttsc_tag_argmax (Linear + arg-max; no logits in HBM)
  forward(X)        logits [B, N, P] with the reference's semantics on a padded batch (no masking: pad id 0 has an ordinary embedding row and
                    every row runs the full N).  Training mode with grad enabled: the differentiable path (text_autograd.py / lstm_autograd.py);
                    otherwise the inference kernels.
  training_step     forward -> ttsc_masked_ce (CrossEntropyLoss(ignore_index=0), value and gradient in one launch) -> backward -> FlatAdamW"""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from ..hip_layers import LSTMHip, linear_hip
from ..io_utils.io_phonemizer import PhonemizerEncodings
from .modules import _ConvStack

STATUS_BAD_ID, STATUS_BAD_TARGET = 1, 2


def check_status(where):
    """raise if a phonemizer kernel met an id outside its table or a target outside [0, classes) since the last check (synchronises)"""
    st = int(_lib.lib().ttsc_phonemizer_status())
    if st < 0:
        raise _lib.TTSCError('%s: ttsc_phonemizer_status failed: %s' % (where, _lib.lib().ttsc_last_error().decode()))
    if st & STATUS_BAD_ID:
        raise _lib.TTSCError('%s: a character or case id lies outside its embedding table (ttsc_char_features wrote zeros there)' % where)
    if st & STATUS_BAD_TARGET:
        raise _lib.TTSCError('%s: a target lies outside [0, classes) and is not the ignore index (ttsc_masked_ce left it out)' % where)


def char_features(x_char, x_case, char_table, case_table, lengths_dev=None):
    """ttsc_char_features: int ids [B, N] x 2 -> fp32 [B, Ec + Es, N], zero at positions >= lengths_dev[b]"""
    if not x_char.is_cuda:
        raise _lib.TTSCError('char_features: ids must live on a HIP device; no CPU path')
    B, N = x_char.shape
    xc, xs = x_char.to(torch.int32).contiguous(), x_case.to(torch.int32).contiguous()
    ct, st = char_table.detach().float().contiguous(), case_table.detach().float().contiguous()
    out = torch.empty((B, ct.shape[1] + st.shape[1], N), dtype=torch.float32, device=x_char.device)
    with _lib.on_device(x_char.device):
        _lib.check(_lib.lib().ttsc_char_features(_lib.dev_ptr(xc), _lib.dev_ptr(xs), _lib.dev_ptr(ct), _lib.dev_ptr(st),
                                                 _lib.dev_ptr(lengths_dev) if lengths_dev is not None else None, B, N, ct.shape[0], ct.shape[1],
                                                 st.shape[0], st.shape[1], _lib.dev_ptr(out), _lib.current_stream()), 'ttsc_char_features')
    return out


def tag_argmax(x, weight, bias=None, lengths_dev=None, period=0, want_logits=False):
    """ttsc_tag_argmax: x [..., K] (rows at a constant stride) . weight [P, K]^T + bias -> int32 tags [...] (first maximum; 0 at rows >=
    lengths_dev[row // period]) and, when asked for, the logits [..., P]"""
    if not x.is_cuda:
        raise _lib.TTSCError('tag_argmax: input must live on a HIP device; no CPU path')
    K = x.shape[-1]
    x2 = x.float()
    if x2.dim() != 2 or x2.stride(1) != 1:
        x2 = x2.contiguous().reshape(-1, K)
    M = x2.shape[0]
    w = weight.detach().float().contiguous()
    b = bias.detach().float().contiguous() if bias is not None else None
    P = w.shape[0]
    assert w.shape[1] == K, (tuple(w.shape), K)
    tags = torch.empty((M,), dtype=torch.int32, device=x.device)
    logits = torch.empty((M, P), dtype=torch.float32, device=x.device) if want_logits else None
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().ttsc_tag_argmax(C.c_void_p(x2.data_ptr()), _lib.dev_ptr(w),
                                              _lib.dev_ptr(b) if b is not None else None,
                                              _lib.dev_ptr(lengths_dev) if lengths_dev is not None else None, int(period), M, P, K, x2.stride(0),
                                              _lib.dev_ptr(tags), _lib.dev_ptr(logits) if logits is not None else None, _lib.current_stream()),
                   'ttsc_tag_argmax')
    lead = tuple(x.shape[:-1])
    return tags.reshape(lead), (logits.reshape(lead + (P,)) if logits is not None else None)


class MaskedCEFn(torch.autograd.Function):
    """(loss, status) = ttsc_masked_ce(logits [R, K], targets int64 [R], ignore_index): mean cross-entropy over the rows whose target is not
    ignored — 0 when there is none, where torch.nn.CrossEntropyLoss gives NaN.  status: int32 [1], 2 when a target was out of range."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        lg = logits.detach().float().contiguous()
        tg = target.contiguous().long()
        R, K = lg.shape
        dev = lg.device
        L = _lib.lib()
        grad = torch.empty_like(lg)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.ttsc_masked_ce_workspace_bytes(R)), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.ttsc_masked_ce(_lib.dev_ptr(lg), _lib.dev_ptr(tg), R, K, int(ignore_index), _lib.dev_ptr(out), _lib.dev_ptr(grad),
                                        _lib.dev_ptr(status), _lib.dev_ptr(ws), ws.numel(), _lib.current_stream()), 'ttsc_masked_ce')
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(status)
        return out.reshape(()), status

    @staticmethod
    def backward(ctx, g_out, _g_status):
        grad, = ctx.saved_tensors
        return grad * g_out, None, None


def masked_ce(logits, target, ignore_index=0):
    if not logits.is_cuda:
        raise _lib.TTSCError('masked_ce: logits must live on a HIP device; no CPU path')
    return MaskedCEFn.apply(logits, target.to(logits.device), int(ignore_index))


class CubenetPhonemizer(nn.Module):
    def __init__(self, encodings: PhonemizerEncodings, lr=2e-4):
        super().__init__()
        self._encodings = encodings
        self._lr = lr
        self._char_emb = nn.Embedding(len(encodings.graphemes), 32)
        self._case_emb = nn.Embedding(2, 8)
        convs, inp = [], 40
        for _ in range(3):
            convs += [nn.Conv1d(in_channels=inp, out_channels=256, kernel_size=3, padding=1), nn.Tanh()]
            inp = 256
        self._convs = nn.ModuleList(convs)
        self._rnn = nn.LSTM(input_size=256, hidden_size=200, num_layers=2, batch_first=True, bidirectional=True)
        self._output_softmax = nn.Linear(200 * 2, len(encodings.phonemes))
        self._ignore_index = 0
        self._val_sacc = 0
        self._val_pacc = 0
        self._val_loss = 9999
        self._hip = {}
        self._optimizer = None
        self._train_convs = {}

    # ---- device handles ---------------------------------------------------------------------------------------------------
    @torch.jit.ignore
    def _get_device(self):
        p = self._output_softmax.weight
        if p.device.type == 'cpu':
            raise _lib.TTSCError('CubenetPhonemizer: parameters live on the CPU; move the module to a HIP device (no CPU path)')
        return p.device

    def _cnn(self):
        if 'cnn' not in self._hip:
            self._hip['cnn'] = _ConvStack([(self._convs[0], None), (self._convs[2], None), (self._convs[4], None)])
        return self._hip['cnn'].sync()

    def _lstm(self):
        if 'rnn' not in self._hip:
            self._hip['rnn'] = LSTMHip(self._rnn)
        return self._hip['rnn']

    def _ids(self, X, dev):
        return X['x_char'].to(dev), X['x_case'].to(dev)

    # ---- inference --------------------------------------------------------------------------------------------------------
    def _encode(self, x_char, x_case, lengths):
        """ids [B, N] -> BiLSTM output [B, N, 400]; with lengths (B > 1) the convolutions see zeros beyond each sentence's end and the recurrences
        stop there, so a sentence's rows equal its B = 1 result"""
        B, N = x_char.shape
        len_dev = _lib.lengths_dev(lengths, x_char.device) if (lengths is not None and B > 1) else None
        h = char_features(x_char, x_case, self._char_emb.weight, self._case_emb.weight, len_dev)
        mask = None
        if len_dev is not None:
            mask = (torch.arange(N, device=h.device)[None, :] < len_dev[:, None]).float()[:, None, :]
        for c in self._cnn():
            h = c(h, act='tanh')
            if mask is not None:
                h = h * mask
        h = self._lstm()(h.permute(0, 2, 1).contiguous(), lengths=lengths if len_dev is not None else None)
        return h, len_dev

    def tag(self, X, lengths=None, return_logits=False):
        """X {'x_char', 'x_case'} int [B, N] -> int32 tags [B, N] on the device (0 at positions >= lengths[b]).  lengths: per-sentence
        character counts of a padded batch — each sentence's tags then equal its B = 1 result.  return_logits (debug): -> (tags, logits [B, N, P])."""
        dev = self._get_device()
        with torch.no_grad():
            x_char, x_case = self._ids(X, dev)
            h, len_dev = self._encode(x_char, x_case, lengths)
            tags, logits = tag_argmax(h, self._output_softmax.weight, self._output_softmax.bias, len_dev, h.shape[1] if len_dev is not None else 0,
                                      want_logits=return_logits)
        return (tags, logits) if return_logits else tags

    def forward(self, X):
        """phonemizer.py:33-47 -> logits [B, N, P]"""
        if self.training and torch.is_grad_enabled():
            return self._forward_train(X)
        dev = self._get_device()
        with torch.no_grad():
            x_char, x_case = self._ids(X, dev)
            h, _ = self._encode(x_char, x_case, None)
            return linear_hip(h, self._output_softmax.weight, self._output_softmax.bias)

    # ---- training ---------------------------------------------------------------------------------------------------------
    def _forward_train(self, X):
        from ..hifigan.autograd import TrainConv, hip_conv
        from .lstm_autograd import lstm_forward_train
        from .text_autograd import hip_embedding, hip_linear
        dev = self._get_device()
        x_char, x_case = self._ids(X, dev)
        h = torch.cat([hip_embedding(self._char_emb, x_char), hip_embedding(self._case_emb, x_case)], dim=-1).permute(0, 2, 1)
        for i in (0, 2, 4):
            c = self._convs[i]
            tc = self._train_convs.get(i)
            if tc is None:
                tc = self._train_convs[i] = TrainConv(c.in_channels, c.out_channels, c.kernel_size[0], padding=c.padding[0], dilation=c.dilation[0])
            h = torch.tanh(hip_conv(tc, h, c.weight, c.bias))
        h = lstm_forward_train(self._rnn, h.permute(0, 2, 1))
        return hip_linear(h, self._output_softmax.weight, self._output_softmax.bias)

    def _loss(self, y_pred, y_target):
        return masked_ce(y_pred.reshape(y_pred.shape[0] * y_pred.shape[1], -1), y_target.reshape(-1), self._ignore_index)

    def configure_optimizers(self):
        """phonemizer.py:94-95: AdamW(lr) (torch's defaults: betas (0.9, 0.999), weight decay 0.01) as optim.FlatAdamW"""
        from ..optim import FlatAdamW
        self._get_device()
        self._optimizer = FlatAdamW(list(self.parameters()), self._lr)
        return self._optimizer

    def optimizers(self):
        if self._optimizer is None:
            self.configure_optimizers()
        return self._optimizer

    def training_step(self, batch, batch_idx=None):
        """phonemizer.py:49-55 plus what Lightning does around it: zero_grad, backward, optimizer step.  -> the loss (a device scalar).  The update
        skips itself on the device when a target was out of range or a split recurrence timed out; `check_status` / `_lib.check_split_status`
        report either (the trainer asks once per epoch)."""
        dev = self._get_device()
        opt = self.optimizers()
        opt.zero_grad()
        y_pred = self.forward(batch)
        loss, status = self._loss(y_pred, batch['y_phon'].to(dev))
        loss.backward()
        words = torch.zeros(1, dtype=torch.int32, device=dev)
        if _lib.lib().ttsc_split_status_collect(_lib.current_stream(), words.data_ptr(), 0) < 0:
            raise _lib.TTSCError('ttsc_split_status_collect: %s' % _lib.lib().ttsc_last_error().decode())
        opt.step(guard=torch.bitwise_or(words, status))
        return loss.detach()

    def validation_step(self, batch, batch_idx=None):
        """phonemizer.py:57-67 -> {'loss', 'target', 'pred'} (numpy arrays [B, N]); run it in eval mode, as Lightning does"""
        dev = self._get_device()
        y_target = batch['y_phon']
        with torch.no_grad():
            X = {k: v for k, v in batch.items() if k != 'y_phon'}
            x_char, x_case = self._ids(X, dev)
            h, _ = self._encode(x_char, x_case, None)
            pred, logits = tag_argmax(h, self._output_softmax.weight, self._output_softmax.bias, want_logits=True)
            loss, _ = self._loss(logits, y_target.to(dev))
        return {'loss': loss.item(), 'target': y_target.detach().cpu().numpy(), 'pred': pred.cpu().numpy()}

    def validation_epoch_end(self, outputs):
        """phonemizer.py:69-92: a position counts as an error when target and prediction differ and neither is 0; _val_pacc = 1 - errors /
        positions with a target, _val_sacc = 1 - sentences with an error / sentences"""
        self._val_loss = sum(o['loss'] for o in outputs) / len(outputs)
        perr = serr = total_phones = total_seqs = 0
        for o in outputs:
            t, p = o['target'], o['pred']
            t, p = t.reshape(t.shape[0], -1), p.reshape(p.shape[0], -1)
            n = min(t.shape[1], p.shape[1])
            wrong = (t[:, :n] != p[:, :n]) & (t[:, :n] != 0) & (p[:, :n] != 0)
            total_phones += int((t[:, :n] != 0).sum())
            total_seqs += t.shape[0]
            perr += int(wrong.sum())
            serr += int(wrong.any(axis=1).sum())
        self._val_pacc = 1.0 - (perr / total_phones)
        self._val_sacc = 1.0 - (serr / total_seqs)

    @torch.jit.ignore
    def save(self, path):
        torch.save(self.state_dict(), path)

    @torch.jit.ignore
    def load(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))
