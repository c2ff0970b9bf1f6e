"""Mirror of cube/story.py: ``StoryCube(base_model)(text, speaker=None, background_music_path=None)`` — several paragraphs (separated by a blank
line) in, one narrated int16 track at 24 kHz with looped background music and per-paragraph timestamps out.

The reference synthesises the paragraphs one by one and mixes in a Python loop over every sample.  Here the paragraphs run through the batched,
pipelined path of ``TTSCube`` (sorted by phoneme count, groups of `max_batch`), their float32 waveforms stay on the device, and the whole timeline
— 5 s of music, each paragraph followed by 1 s, 5 s more — is written by one HIP launch (io_utils/story_mix.py, csrc/story.hip) and leaves the GPU
once, as int16.  The samples are the reference's bits (three separately rounded float32 operations and a truncating cast), with two stated
departures:

  * where speech plus music leaves the int16 range the reference's cast is undefined; this build saturates to [-32768, 32767] and reports the
    number of such samples through ``warnings.warn`` (never in `meta`).  It cannot happen for |speech| <= 0.69 of full scale with |music| <= 1;
  * a music file that is not at 24 kHz is resampled by the HIP polyphase resampler (io_utils/resample.py: scipy.signal.resample_poly's default
    filter), not by the soxr resampler behind the reference's `librosa.load(path, sr=24000)`."""
import warnings
from pathlib import Path

import numpy as np
import torch

from .api import TTSCube
from .io_utils.story_mix import mix_timeline, plan_timeline

SAMPLE_RATE = 24000
MUSIC_GAIN, MUSIC_SCALE = 0.30, 32700.0      # cube/story.py:51


class StoryCube:
    def __init__(self, base_model, *, cube=None, music=None, device='cuda:0', max_batch=16, **load_kw):
        """StoryCube(base_model): cube/story.py:8-11 — `TTSCube.load(base_model)` and `~/.ttscube/models/<base_model>/music.wav`.
        cube=: a ready TTSCube instead of the load; music=: a path, or a float32 array already at 24 kHz, instead of that file (both so that a
        StoryCube can be built without ~/.ttscube); load_kw goes to TTSCube.load (text2feat, word_vectors)."""
        self._device = torch.device(device)
        self._cube = cube if cube is not None else TTSCube.load(base_model, device=device, **load_kw)
        self._max_batch = int(max_batch)
        if self._max_batch < 1:
            raise ValueError('StoryCube: max_batch must be at least 1')
        self._resampler = None
        if music is None:
            music = '{0}/.ttscube/models/{1}/music.wav'.format(str(Path.home()), base_model)
        self._default_music = self._upload_music(music)

    def _upload_music(self, music):
        """a path (any rate, mono or not: load_wav) or a float32 array at 24 kHz -> float32 device tensor"""
        if isinstance(music, (str, Path)):
            from .io_utils.audio import load_wav
            from .io_utils.resample import Resampler
            if self._resampler is None:
                self._resampler = Resampler(self._device)
            music, _ = load_wav(str(music), SAMPLE_RATE, resampler=self._resampler)
        music = torch.as_tensor(np.ascontiguousarray(np.asarray(music, dtype=np.float32)))
        if music.dim() != 1 or music.numel() < 1:
            raise ValueError('StoryCube: the background music must be a non-empty mono signal, got shape %s' % (tuple(music.shape),))
        return music.to(self._device)

    def __call__(self, text, speaker=None, background_music_path: str = None, rate=1.0, pitch=0.0, pitch_range=1.0, markup=False, loudness=None,
                 peak_db=-1.0):
        """-> {'audio': np.int16 [total], 'meta': [...]} with the reference's keys and float values (cube/story.py:13-56).
        rate / pitch / pitch_range / markup: TTSCube.__call__'s prosody controls, applied to every paragraph; with markup=True
        each paragraph is read as markup on its own (tags do not span paragraphs, and a paragraph may not contain a newline).
        loudness (LUFS, a scalar or one value per paragraph; None: the generator's own level) / peak_db: every paragraph is brought to that
        integrated loudness on the device before the mix; the music path and `meta` do not change."""
        parts = text.split('\n\n')
        music = self._default_music if background_music_path is None else self._upload_music(background_music_path)
        waves = self._cube._synthesize_batch_device(parts, speaker=speaker, max_batch=self._max_batch, rate=rate, pitch=pitch, pitch_range=pitch_range,
                                                    markup=markup, **({} if loudness is None else {'loudness': loudness, 'peak_db': peak_db}))
        lengths = [int(w.numel()) for w in waves]
        seg_dst, total, meta = plan_timeline(lengths, SAMPLE_RATE, texts=parts)
        seg_src = [sum(lengths[:p]) for p in range(len(lengths))]
        with torch.cuda.device(self._device):
            speech = torch.cat(waves) if waves else torch.zeros((0,), dtype=torch.float32, device=self._device)
            track, clipped = mix_timeline(speech, seg_src, lengths, seg_dst, music, total, gain=MUSIC_GAIN, scale=MUSIC_SCALE, return_clipped=True)
            audio = track.cpu().numpy()
            clipped = int(clipped.item())
        if clipped:
            warnings.warn('StoryCube: %d of %d samples left the int16 range and were saturated (the reference leaves them undefined); lower the '
                          'level of the music' % (clipped, total), RuntimeWarning)
        return {'audio': audio, 'meta': meta}
