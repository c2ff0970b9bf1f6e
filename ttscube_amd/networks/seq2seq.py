"""Mirror of cube/networks/modules.py:58-88 (``Attention``) and 208-314 (``Seq2Seq``): the attention encoder-decoder behind the word-level G2P.
Same constructors and state_dict keys (``input_emb``, ``output_emb``, ``encoder.*``, ``decoder.*``, ``attention.attn.conv.*``, ``attention.v``,
``output.*``); torch modules are parameter containers only.  Inference only (eval mode: no attention / inter-layer dropout).

  embed            ttsc_g2p_embed (range-checked gather of the input embedding)
  encoder          LSTMHip over all N positions of the padded word (PAD positions included, as the reference; with per-word `n` each word's
                   recurrences run over its own n positions, i.e. what it would see in a batch padded to n)
  hoisted          pe = enc . W_att[:, D:]^T + b for all positions; tab = output_emb . W_ih0[:, E:]^T (both linear_hip, exact fp32)
  decode           ttsc_g2p_decode: the whole autoregressive loop of every word in one launch (csrc/g2p.hip)

  forward(x)             logits [B, T, L] of the free-running loop, T as the reference's batch-wide loop gives it (the latest first <EOS>, at
                         most 10 N + 1): one stopping launch for the step counts, one fixed-T launch that writes the logits
  forward(x, gs_output)  teacher-forced logits [B, gs_output.shape[1], L]
  transcribe_ids(x, n)   the runtime path: labels and step counts per word, per-word stop, no logits in HBM"""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from ..hip_layers import LSTMHip, linear_hip
from .modules import ConvNorm

STATUS_BAD_TOKEN, STATUS_BAD_LABEL, STATUS_BAD_N = 1, 2, 4
LAUNCHES = [0]      # ttsc_g2p_decode launches of this process (tests: a text of lexicon hits launches none)


def check_status(where):
    """raise if a G2P kernel met an id outside its table since the last check (synchronises); the convention of phonemizer.check_status"""
    st = int(_lib.lib().ttsc_g2p_status())
    if st < 0:
        raise _lib.TTSCError('%s: ttsc_g2p_status failed: %s' % (where, _lib.lib().ttsc_last_error().decode()))
    if st & STATUS_BAD_TOKEN:
        raise _lib.TTSCError('%s: a token id lies outside the input embedding table (ttsc_g2p_embed wrote zeros there)' % where)
    if st & STATUS_BAD_LABEL:
        raise _lib.TTSCError('%s: a teacher label lies outside the output embedding table (ttsc_g2p_decode fed back zeros)' % where)
    if st & STATUS_BAD_N:
        raise _lib.TTSCError('%s: a padded word length lies outside [1, N] (ttsc_g2p_decode clamped it)' % where)


def pack4(w):
    """[rows, K] -> [K/4][rows][4]: the layout rnn_chain.hpp streams (four consecutive k of a row are one 16-byte load)"""
    rows, K = w.shape
    return w.reshape(rows, K // 4, 4).permute(1, 0, 2).contiguous()


def g2p_embed(ids, table):
    """ttsc_g2p_embed: int ids [...] -> fp32 [..., Em]; zeros (and a status bit) for ids outside the table"""
    if not ids.is_cuda:
        raise _lib.TTSCError('g2p_embed: ids must live on a HIP device; no CPU path')
    x = ids.to(torch.int32).contiguous()
    tab = table.detach().float().contiguous()
    out = torch.empty(tuple(x.shape) + (tab.shape[1],), dtype=torch.float32, device=x.device)
    if x.numel():
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_g2p_embed(_lib.dev_ptr(x), _lib.dev_ptr(tab), x.numel(), tab.shape[0], tab.shape[1], _lib.dev_ptr(out),
                                                 _lib.current_stream()), 'ttsc_g2p_embed')
    return out


class Attention(nn.Module):
    """cube/networks/modules.py:58-69 (parameter container)"""

    def __init__(self, enc_hid_dim, dec_hid_dim, att_proj_size=100, dropout_prob=0.1, kernel_size=1):
        super().__init__()
        self.dropout_prob = dropout_prob
        self.enc_hid_dim = enc_hid_dim
        self.dec_hid_dim = dec_hid_dim
        self.attn = ConvNorm(enc_hid_dim + dec_hid_dim, att_proj_size, kernel_size=kernel_size, w_init_gain='tanh', padding=kernel_size // 2)
        self.v = nn.Parameter(torch.rand(att_proj_size))


class Seq2Seq(nn.Module):
    def __init__(self, num_input_tokens, num_output_tokens, embedding_size=100, encoder_size=200, encoder_layers=2, decoder_size=200,
                 decoder_layers=2, pad_index=0, unk_index=1, stop_index=2):
        super().__init__()
        self.emb_size = embedding_size
        self.input_emb = nn.Embedding(num_input_tokens, embedding_size, padding_idx=pad_index)
        self.output_emb = nn.Embedding(num_output_tokens, embedding_size, padding_idx=pad_index)
        self.encoder = nn.LSTM(embedding_size, encoder_size, encoder_layers, dropout=0.33, bidirectional=True, batch_first=True)
        self.decoder = nn.LSTM(encoder_size * 2 + embedding_size, decoder_size, decoder_layers, dropout=0.33, batch_first=True)
        self.attention = Attention(encoder_size * 2, decoder_size, att_proj_size=decoder_size)
        self.output = nn.Linear(decoder_size, num_output_tokens)
        self._PAD = pad_index
        self._UNK = unk_index
        self._EOS = stop_index
        self._dec_input_size = encoder_size * 2 + embedding_size
        self._hip = {}
        self._sig = None

    # ---- device handles -------------------------------------------------------------------------------------------------------------------
    @torch.jit.ignore
    def _get_device(self):
        p = self.input_emb.weight
        if p.device.type == 'cpu':
            raise _lib.TTSCError('Seq2Seq: parameters live on the CPU; move the module to a HIP device (no CPU path)')
        return p.device

    def _weights(self):
        """device tensors in the kernel's layouts, rebuilt when a parameter changed"""
        pl = getattr(self, '_plist', None)
        if pl is None:
            pl = self._plist = list(self.parameters())
        sig = tuple((p.data_ptr(), p._version) for p in pl)
        if sig == self._sig:
            return self._hip['w']
        self._get_device()
        if self.decoder.num_layers != 2:
            raise _lib.TTSCError('Seq2Seq: ttsc_g2p_decode runs a 2-layer decoder (got %d layers)' % self.decoder.num_layers)
        g = lambda t: t.detach().float()
        D = self.decoder.hidden_size
        E = self.encoder.hidden_size * 2
        w_att = g(self.attention.attn.conv.weight)
        if w_att.shape[2] != 1:
            raise _lib.TTSCError('Seq2Seq: the attention projection must have kernel size 1')
        w_att = w_att[:, :, 0]                                     # [A, D + E], hidden columns first
        w_ih0 = g(self.decoder.weight_ih_l0)                       # [4D, E + Em]
        if D % 4 or E % 4 or w_att.shape[0] % 4 or w_att.shape[1] != D + E:
            raise _lib.TTSCError('Seq2Seq: decoder size, encoder width and attention width must be multiples of 4')
        w = {
            'w_aq': pack4(w_att[:, :D]), 'w_pe': w_att[:, D:].contiguous(), 'b_pe': g(self.attention.attn.conv.bias).contiguous(),
            'v': g(self.attention.v).contiguous(), 'w_ic': pack4(w_ih0[:, :E]),
            'tab': linear_hip(g(self.output_emb.weight).contiguous(), w_ih0[:, E:].contiguous()),
            'w_hh0': pack4(g(self.decoder.weight_hh_l0)), 'b0': (g(self.decoder.bias_ih_l0) + g(self.decoder.bias_hh_l0)).contiguous(),
            'w_ih1': pack4(g(self.decoder.weight_ih_l1)), 'w_hh1': pack4(g(self.decoder.weight_hh_l1)),
            'b1': (g(self.decoder.bias_ih_l1) + g(self.decoder.bias_hh_l1)).contiguous(),
            'w_out': pack4(g(self.output.weight)), 'b_out': g(self.output.bias).contiguous(), 'D': D, 'E': E, 'A': w_att.shape[0],
            'L': self.output.weight.shape[0],
        }
        self._hip['w'] = w
        self._sig = sig
        return w

    def _lstm(self):
        if 'enc' not in self._hip:
            self._hip['enc'] = LSTMHip(self.encoder)
        return self._hip['enc']

    # ---- the pieces -----------------------------------------------------------------------------------------------------------------------
    def encode(self, x, n=None):
        """token ids [B, N] -> encoder states [B, N, E]; n (list of per-word padded lengths, each <= N): word b's recurrences run over its first
        n[b] positions — what it sees in a batch padded to n[b]; rows beyond are never read"""
        emb = g2p_embed(x, self.input_emb.weight)
        lengths = None
        if n is not None and any(int(v) != x.shape[1] for v in n):
            lengths = n if isinstance(n, _lib.DevLengths) else _lib.DevLengths(n, device=x.device)
        return self._lstm()(emb, lengths=lengths)

    def decode(self, enc, n=None, gs=None, steps=None, stop=False, want_logits=True, want_idx=True):
        """ttsc_g2p_decode on encoder states [B, N, E].  n: per-word padded lengths (list / int tensor) or None (N); gs: int teacher labels
        [B, T]; steps: T (default: gs.shape[1], else 10 N + 1); stop: end a word at its first <EOS> / after 10 n + 1 steps.
        -> (idx int32 [B, T] or None, count int32 [B], logits [B, T, L] or None)"""
        if not enc.is_cuda:
            raise _lib.TTSCError('Seq2Seq.decode: encoder states must live on a HIP device; no CPU path')
        w = self._weights()
        dev = enc.device
        enc = enc.float().contiguous()
        B, N, E = enc.shape
        if E != w['E']:
            raise _lib.TTSCError('Seq2Seq.decode: encoder states are %d wide, the decoder expects %d' % (E, w['E']))
        pe = linear_hip(enc, w['w_pe'], w['b_pe'])
        n_dev = None
        if n is not None:
            # the kernel reads one length per word: the count is checked here for every kind of n, the values on the host where they
            # are there (a device tensor's are clamped by the kernel, which sets STATUS_BAD_N)
            count_n = n.numel() if torch.is_tensor(n) else len(n)
            if count_n != B:
                raise _lib.TTSCError('Seq2Seq.decode: one padded length per word (got %d for %d words)' % (count_n, B))
            if not torch.is_tensor(n) and any(int(v) < 1 or int(v) > N for v in n):
                raise _lib.TTSCError('Seq2Seq.decode: a padded word length lies outside [1, %d]' % N)
            n_dev = _lib.lengths_dev(n, dev)
            if n_dev.numel() != B:
                raise _lib.TTSCError('Seq2Seq.decode: the device copy of the padded lengths holds %d values for %d words' % (n_dev.numel(), B))
        gs_dev = None
        if gs is not None:
            gs_dev = gs.to(dev).to(torch.int32).contiguous()
            T = gs_dev.shape[1] if steps is None else int(steps)
            if tuple(gs_dev.shape) != (B, T):
                raise _lib.TTSCError('Seq2Seq.decode: teacher labels must be [%d, %d] (got %s)' % (B, T, tuple(gs_dev.shape)))
        else:
            T = 10 * N + 1 if steps is None else int(steps)
        idx = torch.empty((B, T), dtype=torch.int32, device=dev) if want_idx else None
        count = torch.empty((B,), dtype=torch.int32, device=dev)
        logits = torch.empty((B, T, w['L']), dtype=torch.float32, device=dev) if want_logits else None
        scratch = torch.empty((2, B, N), dtype=torch.float32, device=dev)
        P = lambda t: t.data_ptr() if t is not None else None
        a = _lib.G2pArgs(P(enc), P(pe), P(n_dev), P(gs_dev), P(w['w_aq']), P(w['v']), P(w['w_ic']), P(w['tab']), P(w['w_hh0']), P(w['b0']),
                         P(w['w_ih1']), P(w['w_hh1']), P(w['b1']), P(w['w_out']), P(w['b_out']), P(scratch), P(idx), P(count), P(logits),
                         B, N, T, E, w['A'], w['D'], w['L'], self._EOS, int(bool(stop)))
        with _lib.on_device(dev):
            _lib.check(_lib.lib().ttsc_g2p_decode(C.byref(a), _lib.current_stream()), 'ttsc_g2p_decode')
        LAUNCHES[0] += 1
        return idx, count, logits

    def _check_input(self, x, n=None):
        if self.training and torch.is_grad_enabled():
            raise _lib.TTSCError('Seq2Seq: G2P training is not built into forward() (no attention / decoder backward here); call eval() or run under '
                                 'torch.no_grad(), or train through networks/g2p_train.py (scripts/train_g2p.py)')
        dev = self._get_device()
        if not x.is_cuda:
            raise _lib.TTSCError('Seq2Seq: token ids must live on a HIP device; no CPU path')
        if n is None or isinstance(n, _lib.DevLengths):
            return n
        if len(n) != x.shape[0] or any(int(v) < 1 or int(v) > x.shape[1] for v in n):
            raise _lib.TTSCError('Seq2Seq: one padded length per word, each inside [1, %d]' % x.shape[1])
        return _lib.DevLengths(n, device=dev)      # one upload for the encoder and the decoder

    def transcribe_ids(self, x, n=None):
        """token ids [B, N] -> (labels int32 [B, 10 N + 1], steps int32 [B]): free running, each word stops at its first <EOS>"""
        n = self._check_input(x, n)
        with torch.no_grad():
            idx, count, _ = self.decode(self.encode(x, n), n=n, stop=True, want_logits=False)
        return idx, count

    def forward(self, x, gs_output=None, n=None):
        """modules.py:258-297 -> logits [B, T, L]"""
        n = self._check_input(x, n)
        with torch.no_grad():
            enc = self.encode(x, n)
            if gs_output is not None:
                return self.decode(enc, n=n, gs=gs_output, want_idx=False)[2]
            # the reference's loop is batch-wide: it ends when every word has emitted <EOS>, at the latest after 10 N + 1 steps
            _, count, _ = self.decode(enc, n=n, stop=True, want_logits=False, want_idx=False)
            T = min(int(count.max().item()), 10 * x.shape[1] + 1)
            return self.decode(enc, n=n, steps=T, want_idx=False)[2]

    @torch.jit.ignore
    def save(self, path):
        torch.save(self.state_dict(), path)

    @torch.jit.ignore
    def load(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))
