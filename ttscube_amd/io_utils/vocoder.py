"""Mirror of cube/io_utils/vocoder.py::MelVocoder.

`melspectrogram` (vocoder.py:54-63) is the part the vocoder pipeline uses: STFT 1024 / hop_size, Hann, centred frames -> 80-bin mel (Slaney) ->
log10(max(1e-5, .)).  The reference computes it with librosa on the CPU inside DataLoader workers; here it runs on the GPU (io_utils/melspec.py:
DFT and mel projection as MFMA GEMMs).

The rest of the class — `fft`, `ifft`, `griffinlim`, `_preemphasis` and the small helpers — runs on the LDS FFT kernels of io_utils/stft.py
(csrc/stft_fft.hip) and hands numpy arrays in the reference's [F, nb] layout back.  Departures from the reference, all stated where they occur:
`fft` works (the reference's raises TypeError), and `GriffinLimVocoder` — not in the reference — turns this project's natural-log mel into audio
through a pseudo-inverse of the mel basis and Griffin-Lim, with the `vocoder` contract of io_utils/runtime.py::synthesize_devset, so that a
Textcoder checkpoint can be heard without a trained HiFi-GAN generator."""
import math

import numpy as np
import torch

from . import melspec
from . import stft as _stft


class MelVocoder:
    def __init__(self, device='cuda:0'):
        self._device = torch.device(device)

    def melspectrogram(self, y, sample_rate, num_mels, hop_size, use_preemphasis=False):
        """y: 1-D numpy array / tensor (or [B, L]) -> numpy [frames, num_mels] (or [B, frames, num_mels]), float32."""
        if use_preemphasis:
            y = self._preemphasis(y.cpu().numpy() if torch.is_tensor(y) else y)
        t = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y, dtype=torch.float32)
        single = t.dim() == 1
        if single:
            t = t.unsqueeze(0)
        m = melspec.melspectrogram_log10(t.to(self._device), sample_rate=sample_rate, num_mels=num_mels, hop_size=hop_size)
        m = m.cpu().numpy()
        return m[0] if single else m

    def _preemphasis(self, x):
        """scipy.signal.lfilter([1, -0.97], [1], x) (vocoder.py:66-67) along the last axis: y[0] = x[0], y[t] = x[t] - 0.97 x[t-1]; float64"""
        x = np.asarray(x, dtype=np.float64)
        y = x.copy()
        y[..., 1:] -= 0.97 * x[..., :-1]
        return y

    def _stft_parameters(self, sample_rate):
        n_fft = 1024
        hop_length = 256
        win_length = n_fft
        return n_fft, hop_length, win_length

    def _amp_to_db(self, x):
        reference = 0.0
        return np.log10(np.maximum(1e-5, x)) - reference

    def _normalize(self, S):
        min_level_db = -100.0
        return np.clip((S - min_level_db) / -min_level_db, 0, 1)

    def _to_device(self, a, dtype):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype).to(self._device)

    def fft(self, y, sample_rate, use_preemphasis=True):
        """y [L] (or [B, L]) -> numpy complex64 [F, nb] (or [B, F, nb]): the transposed librosa.stft of vocoder.py:42-48.  The reference's own
        `fft` raises TypeError (it calls `_stft` without the hop); this one uses the hop of `_stft_parameters`, 256."""
        n_fft, hop, _ = self._stft_parameters(sample_rate)
        if use_preemphasis:
            y = self._preemphasis(y.cpu().numpy() if torch.is_tensor(y) else y)
        return _stft.stft(self._to_device(y, torch.float32), n_fft=n_fft, hop=hop).cpu().numpy()

    def ifft(self, y, sample_rate):
        """y complex [F, nb] (or [B, F, nb]) -> numpy float32 [hop (F - 1)]: librosa.istft at hop 256 (vocoder.py:50-52,69-71)"""
        n_fft, hop, _ = self._stft_parameters(sample_rate)
        return _stft.istft(self._to_device(y, torch.complex64), n_fft=n_fft, hop=hop).cpu().numpy()

    def griffinlim(self, spectrogram, n_iter=100, sample_rate=16000, angles=None):
        """spectrogram [F, nb] (or [B, F, nb]) linear magnitude -> numpy float32 audio (vocoder.py:100-124 at n_fft 1024 / hop 256).  angles
        (complex, the spectrogram's shape): starting phases; None draws them from numpy's global generator exactly as the reference does."""
        n_fft, hop, _ = self._stft_parameters(sample_rate)
        a = None if angles is None else self._to_device(angles, torch.complex64)
        return _stft.griffinlim(self._to_device(spectrogram, torch.float32), n_iter=n_iter, n_fft=n_fft, hop=hop, angles=a).cpu().numpy()


class GriffinLimVocoder:
    """A `vocoder` for io_utils/runtime.py::synthesize_devset that needs no training (NOT in the reference): natural-log mel [B, num_mels, F] on
    the device -> audio [B, 1, hop_size (F - 1)] on the device, by stft.mel_to_linear and `n_iter` Griffin-Lim iterations.  The starting phases
    come from a RandomState(seed) of its own, created anew on every call: the same mel gives the same audio, and numpy's global generator is left
    alone.  The audio is clamped to [-1, 1] because the consumer casts audio * 32767 to int16 unguarded."""

    def __init__(self, n_iter=100, sample_rate=24000, hop_size=240, num_mels=80, n_fft=1024, seed=0, device='cuda:0'):
        self.n_iter, self.sample_rate, self.hop_size, self.num_mels, self.n_fft, self.seed = n_iter, sample_rate, hop_size, num_mels, n_fft, seed
        self._device = torch.device(device)

    def __call__(self, mel):
        mel = torch.as_tensor(mel, dtype=torch.float32).to(self._device)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        mel_log10 = (mel.permute(0, 2, 1) * (1.0 / math.log(10.0))).contiguous()
        mag = _stft.mel_to_linear(mel_log10, self.sample_rate, self.num_mels, self.n_fft)
        y = _stft.griffinlim(mag, n_iter=self.n_iter, n_fft=self.n_fft, hop=self.hop_size, rng=np.random.RandomState(self.seed))
        return y.clamp_(-1.0, 1.0).unsqueeze(1)


class WaveRNNVocoder:
    """The `vocoder` contract of io_utils/runtime.py::synthesize_devset for a CubenetVocoder (NOT in the reference, whose WaveRNN path takes one
    utterance per call): natural-log mel [B, num_mels, F] on the device -> audio [B, 1, L] on the device, L = the longest item's
    high-resolution length, zeros behind a shorter item.  The items go through ``CubenetVocoder._synthesize_batch_device`` `batch` at a time
    (both nets as ragged rows); ``frames`` (valid frames per item, default F) keeps padding frames out of the decode.  Item i is seeded with
    seed + i, so its audio does not depend on `batch`; ``last_lengths`` holds the per-item sample counts of the last call."""

    def __init__(self, vocoder, batch=16, seed=0, mode='philox', num_batches=20):
        self.vocoder, self.batch, self.seed, self.mode, self.num_batches = vocoder, max(1, int(batch)), seed, mode, num_batches
        self.last_lengths = []

    def __call__(self, mel, frames=None):
        mel = torch.as_tensor(mel, dtype=torch.float32)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        B, _, F = mel.shape
        frames = [F] * B if frames is None else [int(f) for f in frames]
        mels = [(mel[b, :, :frames[b]].t() * (1.0 / math.log(10.0))).contiguous() for b in range(B)]
        out = []
        for k in range(0, B, self.batch):
            seeds = [self.seed + i for i in range(k, min(k + self.batch, B))]
            out += [hr for _, hr in self.vocoder._synthesize_batch_device(mels[k:k + self.batch], num_batches=self.num_batches, seed=seeds,
                                                                           mode=self.mode)]
        self.last_lengths = [int(o.shape[0]) for o in out]
        audio = torch.zeros((B, 1, max(self.last_lengths)), dtype=torch.float32, device=out[0].device)
        for b, o in enumerate(out):
            audio[b, 0, :o.shape[0]] = o
        return audio.clamp_(-1.0, 1.0)
