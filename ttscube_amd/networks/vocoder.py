"""Mirror of cube/networks/vocoder.py: ``CubenetVocoder`` = low-res WaveRNN (2.4 kHz) + high-res WaveRNN (24 kHz)
conditioned on the low-res signal, with the reference's chunk-folded inference (vocoder.py:96-131) and checkpoint
layout (`_wavernn_hr.` / `_wavernn_lr.` prefixes; train_vocoder.py:36-59)."""
import numpy as np
import torch
import torch.nn as nn

from .modules import WaveRNN


class CubenetVocoder(nn.Module):
    def __init__(self, num_layers_lr: int = 2, layer_size_lr: int = 512, num_layers_hr: int = 2, layer_size_hr: int = 512,
                 upsample=100, upsample_low=10, learning_rate=1e-4, output='mol'):
        super().__init__()
        self._learning_rate = learning_rate
        self._wavernn_hr = WaveRNN(num_layers=num_layers_hr, layer_size=layer_size_hr, upsample=upsample, use_lowres=True,
                                   upsample_low=upsample_low, learning_rate=learning_rate, output=output)
        self._wavernn_lr = WaveRNN(num_layers=num_layers_lr, layer_size=layer_size_lr, upsample=upsample // upsample_low,
                                   use_lowres=False, learning_rate=learning_rate, output=output)
        self._val_loss_hr = 9999
        self._val_loss_lr = 9999
        self.automatic_optimization = False
        self._global_step = 0
        self._upsample = upsample
        self._upsample_low = upsample_low

    def forward(self, X):
        if 'x' in X:
            return self._train(X)
        return self._inference(X)

    def _train(self, X):
        from .training import wavernn_loss
        loss_hr = wavernn_loss(self._wavernn_hr, {'x': X['x'], 'x_low': X['x_low'], 'mel': X['mel']})
        loss_lr = wavernn_loss(self._wavernn_lr, {'x': X['x_low'], 'mel': X['mel']})
        return {'lr': loss_lr, 'hr': loss_hr, 'loss': (loss_hr + loss_lr) / 2}

    def _inference(self, X, num_batches=20, **kw):
        """vocoder.py:96-107: lr net over the utterance, fold the hr problem into `num_batches` chunks (time -> batch),
        hr net over the folded batch, drop each chunk's warm-up prefix and concatenate.  Returns (x_lr, x_hr) numpy."""
        with torch.no_grad():
            dev = self._wavernn_lr._get_device()
            mel = X['mel'].to(dev).float()
            _, x_lr, _ = self._wavernn_lr.decode({'mel': mel}, **kw)          # [B, 24T] on device
            folded = self._inference_batch(mel, x_lr, num_batches=num_batches)
            _, batched_x_hr, _ = self._wavernn_hr.decode(folded, **kw)        # [nb, (T/nb+1)*240 | ...]
            x_hr = self._compose_batched_inference(batched_x_hr)
        return x_lr.unsqueeze(2).cpu().numpy(), x_hr.cpu().numpy()

    def _compose_batched_inference(self, batched_x):
        batched_x = batched_x[:, self._upsample:]
        return batched_x.reshape(1, -1)

    def _inference_batch(self, mel, x_low, num_batches=5):
        """vocoder.py:113-131 on the device (torch indexing = data movement only): each chunk gets a 1-frame mel
        prefix (pad value -5 for chunk 0) and a `upsample_low`-sample x_low prefix (zeros for chunk 0)."""
        if mel.shape[1] < num_batches:
            num_batches = mel.shape[1]
        mel = mel[:, :mel.shape[1] // num_batches * num_batches]
        x_low = x_low[:, :x_low.shape[1] // num_batches * num_batches]
        mel_split = mel.reshape(num_batches, -1, mel.shape[2])
        x_low_split = x_low.reshape(num_batches, -1)
        m = torch.full((mel_split.shape[0], mel_split.shape[1] + 1, mel_split.shape[2]), -5.0, dtype=torch.float32,
                       device=mel.device)
        m[:, 1:, :] = mel_split
        m[1:, 0, :] = mel_split[:-1, -1, :]
        xl = torch.zeros((x_low_split.shape[0], x_low_split.shape[1] + self._upsample_low), dtype=torch.float32,
                         device=mel.device)
        xl[:, self._upsample_low:] = x_low_split
        xl[1:, 0:self._upsample_low] = x_low_split[:-1, -self._upsample_low:]
        return {'mel': m, 'x_low': xl}

    # ---- a LIST of utterances through both nets as ragged rows (not in the reference, which synthesizes one utterance per call) ----
    def _synthesize_batch_device(self, mels, num_batches=20, max_rows=None, seed=None, mode='philox'):
        """mels: list of [T_i, 80] log10-mels.  Returns a list of (x_lr [24 T_i], x_hr) DEVICE tensors in input order; item i has the
        bits of ``_inference({'mel': mels[i][None]}, seed=s_i, mode=mode)`` with s_i = seed + i (a list `seed` is taken as is).

        The low-resolution net decodes every utterance as one ragged row (stream 0, seed s_i).  networks/vocode_plan.py folds every
        utterance as `_inference_batch` does and sorts the rows (utterance, chunk c; stream c, seed s_i) longest first into launches of
        at most `max_rows` rows (default: the CU count rounded down to a multiple of 8, which keeps the tile kernel eligible); one
        ragged high-resolution decode per launch.  Fold and un-fold are torch gathers on the device."""
        from .vocode_plan import plan_vocode
        if mode not in ('philox', 'argmax'):
            raise ValueError("synthesize_batch: mode must be 'philox' or 'argmax', got %r" % (mode,))
        with torch.no_grad():
            dev = self._wavernn_lr._get_device()
            mels = [torch.as_tensor(m, dtype=torch.float32).to(dev) for m in mels]
            for m in mels:
                if m.dim() != 2 or m.shape[0] < 1:
                    raise ValueError('synthesize_batch: every mel is [T, num_mels] with T >= 1, got %s' % (tuple(m.shape),))
            if isinstance(seed, (list, tuple)):
                seeds = [int(s) for s in seed]
            else:
                if seed is None:
                    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if mode == 'philox' else 0
                seeds = [int(seed) + i for i in range(len(mels))]
            if max_rows is None:
                max_rows = max(8, torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8)
            plan = plan_vocode([int(m.shape[0]) for m in mels], seeds, num_batches=num_batches, max_rows=max_rows,
                               upsample=self._upsample, upsample_low=self._upsample_low)
            per_frame = self._upsample // self._upsample_low
            mel_src = torch.cat([torch.full((1, mels[0].shape[1]), -5.0, dtype=torch.float32, device=dev)] + mels, dim=0)
            # (a) low-resolution net
            x_lr = [None] * len(mels)
            for li, launch in enumerate(plan.lr_launches):
                lengths, sd, st = plan.lr_tables(li)
                m = mel_src[torch.from_numpy(plan.lr_mel_index(li)).to(dev)]
                _, wav, _, _ = self._wavernn_lr.decode({'mel': m}, mode=mode, seed=0, lengths=lengths, seeds=sd, streams=st)
                for r, i in enumerate(launch):
                    x_lr[i] = wav[r, :plan.utts[i].T * per_frame]
            low_src = torch.cat([torch.zeros(1, dtype=torch.float32, device=dev)] + x_lr)
            # (b)-(d) folded high-resolution rows, one ragged decode per launch
            outs = []
            for li in range(len(plan.launches)):
                im, il = plan.fold_index(li)
                fr, ll, sd, st = plan.hr_tables(li)
                X = {'mel': mel_src[torch.from_numpy(im).to(dev)], 'x_low': low_src[torch.from_numpy(il).to(dev)]}
                _, wav, _, _ = self._wavernn_hr.decode(X, mode=mode, seed=0, lengths=fr, low_lengths=ll, seeds=sd, streams=st)
                assert wav.shape[1] == plan.launch_width(li)
                outs.append(wav.reshape(-1))
            flat = torch.cat(outs)
            x_hr = [flat[torch.from_numpy(ix).to(dev)] for ix in plan.unfold_index()]
            self.last_plan = plan
        return list(zip(x_lr, x_hr))

    def synthesize_batch(self, mels, num_batches=20, max_rows=None, seed=None, mode='philox'):
        """``_synthesize_batch_device`` with numpy results: a list of (x_lr [24 T_i], x_hr) pairs in input order."""
        return [(a.cpu().numpy(), b.cpu().numpy())
                for a, b in self._synthesize_batch_device(mels, num_batches=num_batches, max_rows=max_rows, seed=seed, mode=mode)]

    # ---- the LightningModule surface of vocoder.py:133-176 (pl.Trainer.fit(model) in the reference's scripts/train_vocoder.py) ----
    def configure_optimizers(self):
        """vocoder.py:169-173: two Adam optimizers (low-resolution net first)"""
        self._optimizers = [torch.optim.Adam(self._wavernn_lr.parameters(), lr=self._learning_rate),
                            torch.optim.Adam(self._wavernn_hr.parameters(), lr=self._learning_rate)]
        return self._optimizers

    def optimizers(self):
        if getattr(self, '_optimizers', None) is None:
            self.configure_optimizers()
        return self._optimizers

    def set_gradient_exchange(self, reducers):
        self._reducers = reducers

    def log_dict(self, d, **kw):
        fn = getattr(self, '_log_fn', None)
        if fn is not None:
            fn(d)

    def log(self, name, value, **kw):
        self.log_dict({name: value})

    def training_step(self, batch, batch_idx=None):
        """vocoder.py:136-156: both networks' teacher-forced CE losses, clip_grad_norm 5, Adam x 2, lr decay — on the HIP GRU / GEMM / convolution
        kernels behind autograd (networks/training.py::vocoder_training_step)"""
        from .training import vocoder_training_step
        out = vocoder_training_step(self, batch, self.optimizers(), getattr(self, '_reducers', None))
        self.log_dict(out, prog_bar=True)
        return out

    def validation_step(self, batch, batch_idx=None):
        """vocoder.py:133-134"""
        with torch.no_grad():
            return self.forward(batch)

    def validation_epoch_end(self, outputs) -> None:
        """vocoder.py:158-165"""
        loss_lr = sum(float(x['lr']) for x in outputs) / len(outputs)
        loss_hr = sum(float(x['hr']) for x in outputs) / len(outputs)
        self.log('val_loss', (loss_hr + loss_lr) / 2)
        self._val_loss_hr = loss_hr
        self._val_loss_lr = loss_lr

    @torch.jit.ignore
    def save(self, path):
        torch.save(self.state_dict(), path)

    @torch.jit.ignore
    def load(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))

    def _compute_lr(self, initial_lr, delta, step):
        return initial_lr / (1 + delta * step)
