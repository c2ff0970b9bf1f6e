"""Mirror of cube/networks/textcoder.py: ``CubenetTextcoder`` — phonemes -> log10-mel (two-stage path of
cube/io_utils/runtime.py:41-80).  Same constructor / state_dict keys; `inference` and the teacher-forced `forward` run
on the HIP conv / GEMM / LSTM kernels."""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from ..hip_layers import LSTMHip, linear_hip
from .modules import ConvNorm, LinearNorm, PostNet, PreNet, _ConvStack, _char_lengths, _cnn_forward, _expand_rows, align_durations


class CubenetTextcoder(nn.Module):
    def __init__(self, encodings, pframes: int = 3, lr: float = 2e-4):
        super().__init__()
        self._pframes = pframes
        self._lr = lr
        self._encodings = encodings
        self._phon_emb = nn.Embedding(len(encodings.phon2int) + 1, 64, padding_idx=0)
        self._speaker_emb = nn.Embedding(len(encodings.speaker2int) + 1, 128, padding_idx=0)
        cnn = []
        inp = 64
        for _ in range(3):
            cnn += [ConvNorm(inp, 256, kernel_size=3, padding=1, w_init_gain='tanh'), nn.Tanh()]
            inp = 256
        self._char_cnn = nn.ModuleList(cnn)
        self._rnn_char = nn.LSTM(input_size=256, hidden_size=256, num_layers=2, bidirectional=True, batch_first=True)
        self._rnn_overlay = nn.LSTM(input_size=640, hidden_size=512, num_layers=2, bidirectional=True, batch_first=True)
        self._dur_rnn = nn.LSTM(input_size=640, hidden_size=256, num_layers=2, bidirectional=True, batch_first=True)
        self._dur_output = LinearNorm(512, encodings.max_duration + 1)
        self._pitch_rnn = nn.LSTM(input_size=1024, hidden_size=256, num_layers=2, bidirectional=True, batch_first=True)
        self._pitch_output = LinearNorm(512, int(encodings.max_pitch) + 1)
        self._mel_rnn = nn.LSTM(input_size=1024 + 256, hidden_size=512, num_layers=2, bidirectional=False, batch_first=True)
        self._mel_output = LinearNorm(512, 80 * pframes)
        self._prenet = PreNet(80, 256, 2)
        self._postnet = PostNet(80)
        self._hip = {}
        self._val_loss_durs = self._val_loss_pitch = self._val_loss_mel = 9999
        self._val_loss_total = 999
        self._loaded_optimizer_state = None

    def _lstm(self, name):
        if name not in self._hip:
            self._hip[name] = LSTMHip(getattr(self, name))
        return self._hip[name]

    def _cnn(self):
        if '_cnn' not in self._hip:
            ml = self._char_cnn
            self._hip['_cnn'] = _ConvStack([(ml[0].conv, None), (ml[2].conv, None), (ml[4].conv, None)])
        return self._hip['_cnn']

    @torch.jit.ignore
    def _get_device(self):
        p = self._mel_output.linear_layer.weight
        if p.device.type == 'cpu':
            raise _lib.TTSCError('CubenetTextcoder: parameters live on the CPU; move the module to a HIP device')
        return p.device

    def _text_stack(self, x_char, x_speaker, lengths):
        emb = self._phon_emb.weight[x_char]
        spk = self._speaker_emb.weight[x_speaker]
        h = _cnn_forward(self._cnn(), emb, lengths)
        h = self._lstm('_rnn_char')(h, lengths=lengths)
        h = torch.cat([h, spk.expand(-1, h.shape[1], -1)], dim=-1).contiguous()
        hd = self._lstm('_dur_rnn')(h, lengths=lengths)
        return h, linear_hip(hd, self._dur_output.linear_layer.weight, self._dur_output.linear_layer.bias)

    def inference(self, X, dropout_masks=None):
        """textcoder.py:140-189 (B=1 like the reference).  dropout_masks: optional [steps, 2, 1, 256] {0,1} PreNet masks
        (parity tests); otherwise drawn from torch's device generator.  Returns post-net mel [1, F, 80] (log10)."""
        dev = self._get_device()
        x_char, x_speaker = X['x_char'].to(dev), X['x_speaker'].to(dev)
        assert x_char.shape[0] == 1, 'CubenetTextcoder.inference follows the reference: one utterance per call'
        with torch.no_grad():
            h, out_dur = self._text_stack(x_char, x_speaker, None)
            # duration head -> alignment -> gathered overlay input, all on the device (textcoder.py:160-166,291-302 do it on the host)
            h, _ = _expand_rows(h, align_durations(out_dur, None), stride=self._pframes)
            if h.shape[1] == 0:
                return torch.zeros((1, 0, 80), device=dev)
            h = self._lstm('_rnn_overlay')(h)
            mel = self._ar_decode(h, dropout_masks)
            out = self._postnet(mel, add_residual=True)
            _lib.check_split_status('CubenetTextcoder.inference')
            return out

    def _melar_handle(self):
        """(re)build the persistent AR-decoder handle when a parameter changed"""
        mods = [self._mel_rnn, self._mel_output, self._prenet]
        sig = tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())
        if self._hip.get('_melar_sig') == sig:
            return self._hip['_melar']
        L = _lib.lib()
        _lib.require_gpu()
        if '_melar' in self._hip:
            L.ttsc_melar_destroy(self._hip['_melar'])
        hnd = C.c_void_p()
        _lib.check(L.ttsc_melar_create(self._mel_rnn.hidden_size, 256, 80, 80 * self._pframes, C.byref(hnd)), 'ttsc_melar_create')
        g = lambda t: t.detach().float().cpu().contiguous()
        r = self._mel_rnn
        ts = [g(r.weight_ih_l0), g(r.weight_hh_l0), g(r.weight_ih_l1), g(r.weight_hh_l1), g(r.bias_ih_l1), g(r.bias_hh_l1),
              g(self._mel_output.linear_layer.weight), g(self._mel_output.linear_layer.bias),
              g(self._prenet.layers_h[0].linear_layer.weight), g(self._prenet.layers_h[0].linear_layer.bias),
              g(self._prenet.layers_h[1].linear_layer.weight), g(self._prenet.layers_h[1].linear_layer.bias)]
        P = lambda t: C.c_void_p(t.data_ptr())
        _lib.check(L.ttsc_melar_set_weights(hnd, P(ts[0]), ts[0].shape[1], *[P(t) for t in ts[1:]]), 'ttsc_melar_set_weights')
        self._hip['_melar'] = hnd
        self._hip['_melar_sig'] = sig
        return hnd

    def _ar_decode(self, h, dropout_masks=None, steps=None, seed=None, out=None):
        """textcoder.py:174-185 as ONE persistent kernel launch (csrc/melar.hip).  h: overlay states [B, S, 1024]; dropout_masks
        [S, 2, B, 256] or None (in-kernel Philox from seed); steps [B] or None (all S); out: optional device tensor [B, S, 80 * pframes]
        the kernel writes (every element of it)."""
        hnd = self._melar_handle()
        B, S, _ = h.shape
        r = self._mel_rnn
        n_ov = r.weight_ih_l0.shape[1] - 256
        xg1 = linear_hip(h, r.weight_ih_l0[:, :n_ov].contiguous(), r.bias_ih_l0 + r.bias_hh_l0)    # hoisted input projection
        y = torch.empty((B, S, 80 * self._pframes), dtype=torch.float32, device=h.device) if out is None else out
        assert y.shape == (B, S, 80 * self._pframes) and y.dtype == torch.float32 and y.is_contiguous() and y.device == h.device
        m = None
        if dropout_masks is not None:
            m = torch.as_tensor(dropout_masks).to(h.device).float().reshape(S, 2, B, 256).permute(2, 0, 1, 3).contiguous()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        st = torch.as_tensor(steps, dtype=torch.int32, device=h.device) if steps is not None else None
        with _lib.on_device(h.device):
            _lib.check(_lib.lib().ttsc_melar_decode(hnd, _lib.dev_ptr(xg1), B, S, _lib.dev_ptr(m) if m is not None else None,
                                                    C.c_uint64(seed), _lib.dev_ptr(st) if st is not None else None, _lib.dev_ptr(y),
                                                    _lib.current_stream()), 'ttsc_melar_decode')
        return y.reshape(B, S * self._pframes, 80).contiguous()

    def _ar_decode_stepwise(self, h, dropout_masks=None):
        """The same loop as one kernel launch per layer and step (kept for A/B tests of the persistent kernel)."""
        dev = h.device
        last = torch.full((1, 1, 80), -5.0, device=dev)
        hx = None
        outs = []
        rnn = self._lstm('_mel_rnn')
        for t in range(h.shape[1]):
            m = None if dropout_masks is None else [dropout_masks[t][0].to(dev), dropout_masks[t][1].to(dev)]
            pn = self._prenet(last, masks=m)
            y, hx = rnn(torch.cat([h[:, t:t + 1], pn], dim=-1).contiguous(), hx=hx, return_state=True)
            o = linear_hip(y, self._mel_output.linear_layer.weight, self._mel_output.linear_layer.bias)
            outs.append(o)
            last = o[:, :, -80:].contiguous()
        return torch.cat(outs, dim=1).reshape(1, -1, 80).contiguous()

    def forward(self, X, dropout_masks=None):
        """Teacher-forced path (textcoder.py:100-138): returns (output_dur, output_pitch, output_mel, output_mel_post).  In training mode with
        grad enabled: the differentiable path (networks/textcoder_train.py; dropout_masks: its {'prenet': ..., 'postnet': ...} dict); otherwise
        inference numerics (no autograd)."""
        if self.training and torch.is_grad_enabled():
            from .textcoder_train import textcoder_forward_train
            return textcoder_forward_train(self, X, dropout_masks)
        dev = self._get_device()
        x_char, x_speaker = X['x_char'].to(dev), X['x_speaker'].to(dev)
        B = x_char.shape[0]
        lengths = _char_lengths(X, x_char) if B > 1 else None
        with torch.no_grad():
            h, out_dur = self._text_stack(x_char, x_speaker, lengths)
            h, flens = _expand_rows(h, X['y_frame2phone'], stride=self._pframes)
            h = self._lstm('_rnn_overlay')(h, lengths=flens if B > 1 else None)
            hp = self._lstm('_pitch_rnn')(h, lengths=flens if B > 1 else None)
            out_pitch = linear_hip(hp, self._pitch_output.linear_layer.weight, self._pitch_output.linear_layer.bias)
            y_mgc = X['y_mgc'].to(dev).float()
            lst = [torch.full((B, 1, 80), -5.0, device=dev)]
            for ii in range(y_mgc.shape[1] // self._pframes):
                lst.append(y_mgc[:, (ii + 1) * self._pframes - 1, :].unsqueeze(1))
            cond = self._prenet(torch.cat(lst, dim=1).contiguous(), masks=dropout_masks)
            m = min(h.shape[1], cond.shape[1])
            y = self._lstm('_mel_rnn')(torch.cat([h[:, :m], cond[:, :m]], dim=-1).contiguous())
            mel = linear_hip(y, self._mel_output.linear_layer.weight, self._mel_output.linear_layer.bias).reshape(B, -1, 80).contiguous()
            return out_dur, out_pitch, mel, self._postnet(mel, add_residual=True)

    # ---- the LightningModule surface the reference's trainer drives (textcoder.py:191-270; scripts/train_textcoder.py) ----------------------
    # The step logic lives in networks/textcoder_train.py (HIP kernels end to end).  `optimizers()` hands out what `configure_optimizers()` built;
    # `log_dict` is a no-op unless a logger was attached with `set_logger`.
    def configure_optimizers(self):
        """textcoder.py:269-270: Adam(lr) as optim.FlatAdamW(weight_decay=0); restores a `.opt.last` state queued in `_loaded_optimizer_state`"""
        from .textcoder_train import textcoder_configure_optimizers
        self._optimizer = textcoder_configure_optimizers(self)
        return self._optimizer

    def optimizers(self):
        if getattr(self, '_optimizer', None) is None:
            self.configure_optimizers()
        return self._optimizer

    def set_logger(self, fn):
        self._log_fn = fn

    def log_dict(self, d, **kw):
        fn = getattr(self, '_log_fn', None)
        if fn is not None:
            fn(d)

    def training_step(self, batch, batch_ids=None, dropout_masks=None):
        """textcoder.py:191-226 -> {'loss', 'l_mel', 'l_pitch', 'l_dur'} (read back when first looked at: training.StepLosses)"""
        from .textcoder_train import textcoder_training_step
        out = textcoder_training_step(self, batch, self.optimizers(), dropout_masks)
        self.log_dict(out, prog_bar=True)
        return out

    def validation_step(self, batch, batch_ids=None):
        """textcoder.py:228-251 (run it in eval mode, as Lightning does)"""
        from .textcoder_train import textcoder_validation_step
        out = textcoder_validation_step(self, batch)
        self.log_dict(out, prog_bar=True)
        return out

    def validation_epoch_end(self, outputs) -> None:
        """textcoder.py:253-261"""
        n = len(outputs)
        self._val_loss_total = sum(o['loss'] for o in outputs) / n
        self._val_loss_mel = sum(o['l_mel'] for o in outputs) / n
        self._val_loss_pitch = sum(o['l_pitch'] for o in outputs) / n
        self._val_loss_durs = sum(o['l_dur'] for o in outputs) / n

    @torch.jit.ignore
    def save(self, path):
        torch.save(self.state_dict(), path)

    @torch.jit.ignore
    def load(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))
