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

    @staticmethod
    def _dur_controls(X):
        """the duration controls of X ('x_dur_scale' float [B, N] in [0.25, 4], 'x_dur_set' int [B, N]: Languasito2.inference's);
        this model takes no pitch input at inference, so a pitch control is refused instead of being dropped"""
        if X.get('x_pitch_mul') is not None or X.get('x_pitch_range') is not None:
            raise ValueError('CubenetTextcoder has no pitch input at inference: x_pitch_mul / x_pitch_range cannot be applied (duration controls only)')
        return X.get('x_dur_scale'), X.get('x_dur_set')

    def inference(self, X, dropout_masks=None, seed=None):
        """textcoder.py:140-189 (B=1 like the reference; `inference_batch` takes a padded batch).  dropout_masks: optional [steps, 2, 1, 256]
        {0,1} PreNet masks (parity tests); otherwise drawn in the kernel from Philox with key `seed` (None: a key from torch's generator).
        Returns post-net mel [1, F, 80] (log10)."""
        dev = self._get_device()
        x_char, x_speaker = X['x_char'].to(dev), X['x_speaker'].to(dev)
        assert x_char.shape[0] == 1, 'CubenetTextcoder.inference follows the reference: one utterance per call'
        with torch.no_grad():
            h, out_dur = self._text_stack(x_char, x_speaker, None)
            # duration head -> alignment -> gathered overlay input, all on the device (textcoder.py:160-166,291-302 do it on the host)
            h, _ = _expand_rows(h, align_durations(out_dur, None, *self._dur_controls(X)), stride=self._pframes)
            if h.shape[1] == 0:
                return torch.zeros((1, 0, 80), device=dev)
            h = self._lstm('_rnn_overlay')(h)
            mel = self._ar_decode(h, dropout_masks, seed=seed)
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

    def _ar_xg1(self, h):
        """the hoisted layer-1 input projection of all rows and steps: overlay states [B, S, 1024] -> [B, S, 4H]"""
        r = self._mel_rnn
        n_ov = r.weight_ih_l0.shape[1] - 256
        return linear_hip(h, r.weight_ih_l0[:, :n_ov].contiguous(), r.bias_ih_l0 + r.bias_hh_l0)

    def _ar_decode(self, h, dropout_masks=None, steps=None, seed=None, out=None, seeds=None, members=None):
        """textcoder.py:174-185 as ONE persistent kernel launch (csrc/melar.hip).  h: overlay states [B, S, 1024]; dropout_masks
        [S, 2, B, 256] or None (in-kernel Philox from seed); steps [B] or None (all S); out: optional device tensor [B, S, 80 * pframes]
        the kernel writes (every element of it).
        seeds (B integers < 2**63 or a device int64 tensor [B]) selects the ragged entry (ttsc_melar_decode_ragged): row b draws the masks
        of its solo decode with seed = seeds[b], wherever it stands in the batch; members (None / 0: the dispatcher's rule for B rows; 1, 2,
        4, 8: that split, refused when members * B workgroups cannot be co-resident) belongs to that entry."""
        B, S, _ = h.shape
        y = torch.empty((B, S, 80 * self._pframes), dtype=torch.float32, device=h.device) if out is None else out
        assert y.shape == (B, S, 80 * self._pframes) and y.dtype == torch.float32 and y.is_contiguous() and y.device == h.device
        if seeds is None and members is not None:
            raise _lib.TTSCError('CubenetTextcoder._ar_decode: members= belongs to the per-row-key entry (give seeds=)')
        self._ar_launch(self._ar_xg1(h), dropout_masks, steps, seed, seeds, members, y)
        return y.reshape(B, S * self._pframes, 80).contiguous()

    @staticmethod
    def _row_keys(seeds, B, dev):
        """per-row Philox keys as a device int64 tensor [B] (the kernel reads the same 64 bits unsigned)"""
        if torch.is_tensor(seeds):
            k = seeds.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        else:
            vals = [int(v) for v in seeds]
            if any(v < 0 or v >= 2 ** 63 for v in vals):
                raise _lib.TTSCError('CubenetTextcoder: seeds must be integers in [0, 2**63)')
            k = torch.tensor(vals, dtype=torch.int64, device=dev)
        if k.numel() != B:
            raise _lib.TTSCError('CubenetTextcoder: %d seeds for a batch of %d' % (k.numel(), B))
        return k

    def _ar_launch(self, xg1, dropout_masks, steps, seed, seeds, members, y):
        """one launch of the AR kernel on xg1 [B, S, 4H] into y [B, S, O]"""
        hnd = self._melar_handle()
        B, S, _ = xg1.shape
        dev = xg1.device
        m = None
        if dropout_masks is not None:
            m = torch.as_tensor(dropout_masks).to(dev).float().reshape(S, 2, B, 256).permute(2, 0, 1, 3).contiguous()
        st = torch.as_tensor(steps, dtype=torch.int32, device=dev).contiguous() if steps is not None else None
        P = lambda t: _lib.dev_ptr(t) if t is not None else None
        with _lib.on_device(dev):
            if seeds is not None:
                keys = self._row_keys(seeds, B, dev)
                if st is None:
                    st = torch.full((B,), S, dtype=torch.int32, device=dev)
                _lib.check(_lib.lib().ttsc_melar_decode_ragged(hnd, P(xg1), B, S, P(m), P(keys), P(st), int(members or 0), P(y),
                                                               _lib.current_stream()), 'ttsc_melar_decode_ragged')
                return
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            _lib.check(_lib.lib().ttsc_melar_decode(hnd, P(xg1), B, S, P(m), C.c_uint64(seed), P(st), P(y), _lib.current_stream()),
                       'ttsc_melar_decode')

    def ar_members(self, B=1):
        """the split factor the AR dispatcher picks for B rows on the current device (ttsc_melar_members)"""
        return int(_lib.lib().ttsc_melar_members(self._melar_handle(), int(B)))

    def _ar_decode_batch(self, h, steps, seeds=None, dropout_masks=None, max_rows=None, members=None):
        """The AR stage of `inference_batch`: overlay states h [B, S, 1024] with `steps` [B] valid steps per row -> (pre-postnet mel
        [B, S * pframes, 80], zeros past a row's steps; number of launches).  One hoisted xg1 GEMM, then the launches of
        textcoder_plan.plan_ar_launches: longest rows first, at most max_rows rows each (default CUs // members: the member workgroups of
        a launch must all be resident), every launch at the SAME split `members` (default: what one sentence gets alone) — so a row's bits
        do not depend on the launch it lands in."""
        from .textcoder_plan import plan_ar_launches
        B, S, _ = h.shape
        dev = h.device
        steps = [int(v) for v in steps]
        assert len(steps) == B and max(steps, default=0) <= S
        O = 80 * self._pframes
        if members is None:
            with _lib.on_device(dev):
                members = self.ar_members(1)
        if max_rows is None:
            max_rows = max(1, torch.cuda.get_device_properties(dev).multi_processor_count // members)
        if seeds is None and dropout_masks is None:
            seeds = torch.randint(0, 2 ** 62, (B,)).tolist()
        keys = self._row_keys(seeds, B, dev) if seeds is not None else torch.zeros(B, dtype=torch.int64, device=dev)
        mk = None
        if dropout_masks is not None:
            mk = torch.as_tensor(dropout_masks).to(dev).float().reshape(S, 2, B, 256)
        plan = plan_ar_launches(steps, max_rows)
        y = torch.zeros((B, S, O), dtype=torch.float32, device=dev)
        if not plan:
            return y.reshape(B, S * self._pframes, 80), 0
        xg1 = self._ar_xg1(h)
        st_all = torch.tensor(steps, dtype=torch.int32, device=dev)
        for rows in plan:
            Sl = steps[rows[0]]                      # (longest first: the launch's horizon)
            if len(rows) == B and Sl == S and rows == list(range(B)):
                self._ar_launch(xg1, mk, st_all, None, keys, members, y)
                continue
            idx = torch.tensor(rows, dtype=torch.int64, device=dev)
            yl = torch.empty((len(rows), Sl, O), dtype=torch.float32, device=dev)
            self._ar_launch(xg1.index_select(0, idx)[:, :Sl].contiguous(), None if mk is None else mk[:Sl].index_select(2, idx),
                            st_all.index_select(0, idx), None, keys.index_select(0, idx), members, yl)
            y[idx, :Sl] = yl
        return y.reshape(B, S * self._pframes, 80), len(plan)

    def inference_batch(self, X, seeds=None, dropout_masks=None, max_rows=None, members=None, channel_major=False, return_stats=False):
        """A padded batch of sentences -> (post-net mel [B, Fmax, 80] log10, frames [B]): each row holds what `inference` gives for that
        sentence alone with seed = seeds[b] (zeros past its own frames[b]), wherever the row stands and whichever AR launch it lands in.
        X: 'x_char' long [B, N] (0 = padding AND an out-of-vocabulary phone: give 'x_len', rule of _char_lengths), 'x_speaker' long [B, 1].
        seeds: B integers < 2**63 (None: drawn from torch's generator); dropout_masks [S, 2, B, 256] injects the PreNet masks instead
        (parity tests).  members / max_rows: see _ar_decode_batch.  Rows without a frame are launched nowhere: their mel is empty.
        channel_major=True returns the mel as [B, 80, Fmax] (what a vocoder takes); return_stats=True appends {'launches', 'max_steps', 'rows', 'mel_ar'}."""
        dev = self._get_device()
        x_char, x_speaker = X['x_char'].to(dev), X['x_speaker'].to(dev)
        B = x_char.shape[0]
        pf = self._pframes
        with torch.no_grad():
            lengths = _lib.DevLengths(_char_lengths(X, x_char), device=dev)
            h, out_dur = self._text_stack(x_char, x_speaker, lengths)
            h, steps = _expand_rows(h, align_durations(out_dur, lengths, *self._dur_controls(X)), stride=pf)
            steps = [int(v) for v in steps]
            frames = [n * pf for n in steps]
            S = max(steps) if steps else 0
            stats = {'launches': 0, 'max_steps': S}
            if S == 0:
                out = torch.zeros((B, 80, 0) if channel_major else (B, 0, 80), device=dev)
                return (out, frames, stats) if return_stats else (out, frames)
            act = [b for b in range(B) if steps[b] > 0]      # (rows without a frame take part in nothing below)
            if len(act) < B:
                idx = torch.tensor(act, dtype=torch.int64, device=dev)
                h = h.index_select(0, idx)
                if dropout_masks is not None:
                    dropout_masks = torch.as_tensor(dropout_masks).reshape(S, 2, B, 256)[:, :, act]
                if seeds is not None:
                    seeds = seeds[idx.to(seeds.device)] if torch.is_tensor(seeds) else [seeds[b] for b in act]
            st_act = _lib.DevLengths([steps[b] for b in act], device=dev)
            h = self._lstm('_rnn_overlay')(h, lengths=st_act)
            mel, stats['launches'] = self._ar_decode_batch(h, st_act, seeds, dropout_masks, max_rows, members)
            stats['rows'], stats['mel_ar'] = act, mel       # (the AR output [len(rows), S * pframes, 80] before the PostNet: parity tests)
            fr_act = _lib.DevLengths([n * pf for n in st_act], device=dev)
            out = self._postnet(mel, add_residual=True, lengths=fr_act, channel_major=channel_major)
            if len(act) < B:
                full = torch.zeros((B,) + tuple(out.shape[1:]), dtype=out.dtype, device=dev)
                full[idx] = out
                out = full
            _lib.check_split_status('CubenetTextcoder.inference_batch')
        return (out, frames, stats) if return_stats else (out, frames)

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
