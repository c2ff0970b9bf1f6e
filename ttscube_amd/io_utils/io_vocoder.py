"""Mirror of cube/io_utils/io_vocoder.py: ``VocoderDataset`` (:20-82 — wav folder -> (audio, low-rate audio, log10-mel) with the
`data/cache` files `<name>.mgc.npy / .audio.npy / .audio_low.npy`, random hop-aligned crops) and ``VocoderCollate`` (:85-112).
Differences: librosa.load -> scipy (io_utils/audio.py); the mel features come from the GPU (io_utils/vocoder.py::MelVocoder).
``VocoderDataset.precompute`` (not in the reference) fills the cache ahead of the first epoch in batches: both rate changes on the HIP resampler
(io_utils/resample.py), one spectrogram call per batch."""
import os
import random

import numpy as np
import torch

from .audio import load_wav

N_FFT = 1024        # MelVocoder's analysis window


def mel_rows(segs, half=N_FFT // 2):
    """signals of different lengths as the rows of one spectrogram call -> np.float32 [len(segs), Lmax + half].  The spectrogram reflects a signal
    about its last sample; a shorter row carries its own reflection behind its end, so that its 1 + len // hop frames see the samples they see
    when it is analysed alone, whatever else is in the batch (corpus_import.import_audio lays its rows out the same way).  Every signal must be
    longer than `half` samples."""
    rows = np.zeros((len(segs), max(len(s) for s in segs) + half), dtype=np.float32)
    for r, seg in enumerate(segs):
        rows[r, :len(seg)] = seg
        rows[r, len(seg):len(seg) + half] = seg[-2:-2 - half:-1]
    return rows


class VocoderDataset:
    def __init__(self, path, target_sample_rate=24000, lowres_sample_rate=2400, max_segment_size=-1, random_start=True, hop_size=240,
                 cache_dir='data/cache', mel_vocoder=None):
        self._examples = []
        self._sample_rate = target_sample_rate
        self._sample_rate_low = lowres_sample_rate
        self._max_segment_size = max_segment_size
        self._mel_vocoder = mel_vocoder
        self._hop_size = hop_size
        self._random_start = random_start
        self._cache_dir = cache_dir
        for f in sorted(os.listdir(path)):
            full = os.path.join(path, f)
            if f.endswith('.wav') and os.path.isfile(full):
                w_size = os.stat(full).st_size
                if w_size > 4096 and w_size > max_segment_size * 2:
                    self._examples.append(full)
        os.makedirs(cache_dir, exist_ok=True)

    def __len__(self):
        return len(self._examples)

    def _cache_base(self, filename):
        return os.path.join(self._cache_dir, filename.replace('/', '_').replace('\\', '_'))

    def _features(self, filename):
        cache = self._cache_base(filename)
        if os.path.exists(cache + '.mgc.npy'):
            return np.load(cache + '.audio.npy'), np.load(cache + '.audio_low.npy'), np.load(cache + '.mgc.npy')
        wav, _ = load_wav(filename, self._sample_rate)
        wav_low, _ = load_wav(filename, self._sample_rate_low)
        wav = (wav / np.max(np.abs(wav))) * 0.98
        wav_low = (wav_low / np.max(np.abs(wav_low))) * 0.98
        if self._mel_vocoder is None:
            from .vocoder import MelVocoder
            self._mel_vocoder = MelVocoder()
        mel = self._mel_vocoder.melspectrogram(wav, sample_rate=self._sample_rate, num_mels=80, hop_size=self._hop_size,
                                               use_preemphasis=False)
        np.save(cache + '.mgc', mel)
        np.save(cache + '.audio', wav)
        np.save(cache + '.audio_low', wav_low)
        return wav, wav_low, mel

    def precompute(self, batch=32, device='cuda:0', resampler=None, mel_vocoder=None):
        """Write the cache files of every example that has none yet, `batch` files per GPU call: the files are read and grouped by their own
        rate, each group is uploaded once and resampled from there to both rates (io_utils/resample.py), normalised with the bits of the lazy
        path, and the full-rate rows of a group go through one spectrogram call.  A file that is all zeros or shorter than half an analysis window
        is reported and left uncached (reading it later takes the lazy path).  -> number of files written.  No CPU path."""
        from .. import _lib
        from .audio import read_wav
        _lib.require_gpu()
        if batch < 1:
            raise ValueError('precompute: batch must be at least 1, got %r' % (batch,))
        from .resample import Resampler
        from .vocoder import MelVocoder
        device = torch.device(device)
        resampler = resampler or Resampler(device)
        mel_vocoder = mel_vocoder or self._mel_vocoder or MelVocoder(device)
        groups, written = {}, 0

        def flush(rate):
            nonlocal written
            pending = groups.pop(rate, [])
            if not pending:
                return
            lens = [len(x) for _, x in pending]
            host = np.zeros((len(pending), max(lens)), dtype=np.float32)
            for r, (_, x) in enumerate(pending):
                host[r, :len(x)] = x
            x_dev = torch.from_numpy(host).to(device)
            len_dev = torch.tensor(lens, dtype=torch.int32).to(device)
            per_rate = []
            for sr in (self._sample_rate, self._sample_rate_low):
                y, out_lens, peak = resampler.resample_device(x_dev, len_dev, rate, sr)
                y, out_lens = y.cpu().numpy(), [int(v) for v in out_lens.cpu()]
                peak = peak.cpu().numpy() if peak is not None else np.abs(y).max(axis=1)     # (equal rates: nothing ran, the rows are the files)
                per_rate.append((y, out_lens, peak))
            (y, out_lens, peak), (y_low, out_lens_low, peak_low) = per_rate
            keep = []
            for r, (filename, _) in enumerate(pending):
                if peak[r] == 0 or peak_low[r] == 0:
                    print('Skipping {0}: the file is empty or all zeros'.format(filename))
                elif out_lens[r] <= N_FFT // 2:
                    print('Skipping {0}: {1} samples are fewer than half an analysis window'.format(filename, out_lens[r]))
                else:
                    keep.append(r)
            if not keep:
                return
            wavs = [(y[r, :out_lens[r]] / np.float32(peak[r])) * np.float32(0.98) for r in keep]
            lows = [(y_low[r, :out_lens_low[r]] / np.float32(peak_low[r])) * np.float32(0.98) for r in keep]
            mels = mel_vocoder.melspectrogram(mel_rows(wavs), sample_rate=self._sample_rate, num_mels=80, hop_size=self._hop_size,
                                              use_preemphasis=False)
            for k, r in enumerate(keep):
                cache = self._cache_base(pending[r][0])
                np.save(cache + '.audio', wavs[k])
                np.save(cache + '.audio_low', lows[k])
                np.save(cache + '.mgc', np.ascontiguousarray(mels[k, :1 + len(wavs[k]) // self._hop_size]))      # (last: _features looks for it)
                written += 1

        for filename in self._examples:
            if os.path.exists(self._cache_base(filename) + '.mgc.npy'):
                continue
            x, rate = read_wav(filename)
            if x.size == 0:
                print('Skipping {0}: the file is empty or all zeros'.format(filename))
                continue
            groups.setdefault(rate, []).append((filename, x))
            if len(groups[rate]) >= batch:
                flush(rate)
        for rate in sorted(groups):
            flush(rate)
        return written

    def __getitem__(self, item):
        wav, wav_low, mel = self._features(self._examples[item])
        ms, hs = self._max_segment_size, self._sample_rate // self._sample_rate_low
        if ms == -1 or len(wav) < ms or not self._random_start:
            if not self._random_start and ms != -1 and len(wav) > ms:
                return wav[:ms], wav_low[:ms // hs], mel[:ms // self._hop_size + 1]
            return wav, wav_low, mel
        start = random.randint(0, len(wav) - ms - 1)
        start = start // self._hop_size * self._hop_size   # multiple of the hop size
        stop = start + ms
        start_low = start // hs
        return wav[start:stop], wav_low[start_low:start_low + ms // hs], mel[start // self._hop_size:stop // self._hop_size + 1]


class VocoderCollate:
    def __init__(self, x_zero=0, mel_zero=-5):
        self._x_zero = x_zero
        self._mel_zero = mel_zero

    def collate_fn(self, examples):
        la = max(x[0].shape[0] for x in examples)
        ll = max(x[1].shape[0] for x in examples)
        lm = max(x[2].shape[0] for x in examples)
        mel = np.ones((len(examples), lm, examples[0][2].shape[1]), dtype=np.float64) * self._mel_zero
        x = np.ones((len(examples), la)) * self._x_zero
        x_low = np.ones((len(examples), ll)) * self._x_zero
        for ii, (cx, cxl, cmel) in enumerate(examples):
            mel[ii, :cmel.shape[0], :] = cmel
            x[ii, :cx.shape[0]] = cx
            x_low[ii, :cxl.shape[0]] = cxl
        return {'x': torch.tensor(x, dtype=torch.float), 'x_low': torch.tensor(x_low, dtype=torch.float),
                'mel': torch.tensor(mel, dtype=torch.float)}
