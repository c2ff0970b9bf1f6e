"""Mirror of cube/io_utils/io_textcoder.py: ``TextcoderDataset`` (<id>.json / .mgc / .pitch; no wav, no silencing, no length filter),
``TextcoderEncodings`` (the schema and computation of ``CubeganEncodings``, whose numpy >= 1.24 fix it shares) and ``TextcoderCollate.collate_fn``
(same batch-dict keys, dtypes and padding values)."""
import json
import os

import numpy as np
import torch

from .io_cubegan import CubeganEncodings


class TextcoderDataset:
    """io_textcoder.py:18-46: every `<id>.mgc` of `base_path` whose `<id>.json` and `<id>.pitch` exist; items are {'meta', 'mgc', 'pitch'}"""

    def __init__(self, base_path):
        self._base_path = base_path
        self._examples = []
        for f in sorted(os.listdir(base_path)):
            if not f.endswith('.mgc') or not os.path.isfile(os.path.join(base_path, f)):
                continue
            bpath = os.path.join(base_path, f[:-4])
            if os.path.exists(bpath + '.json') and os.path.exists(bpath + '.pitch'):
                self._examples.append(json.load(open(bpath + '.json')))

    def __len__(self):
        return len(self._examples)

    def __getitem__(self, item):
        description = self._examples[item]
        base_fn = '{0}/{1}'.format(self._base_path, description['id'])
        return {'meta': description, 'mgc': np.load(base_fn + '.mgc'), 'pitch': np.load(base_fn + '.pitch')}


class TextcoderEncodings(CubeganEncodings):
    """io_textcoder.py:49-88: the same file schema and computation as the Cubegan encodings"""


class TextcoderCollate:
    """io_textcoder.py:91-128: x_char (phoneme id + 1, unknown phonemes 0), x_speaker (id + 1), y_mgc padded with -5, y_dur (frames per phoneme,
    padding = ignore index), y_pitch padded with the ignore index, y_frame2phone as lists"""

    def __init__(self, encodings):
        self._encodings = encodings
        self._ignore_index = int(max(encodings.max_pitch, encodings.max_duration) + 1)

    def collate_fn(self, batch):
        max_char = max(len(ex['meta']['phones']) for ex in batch)
        max_mel = max(ex['mgc'].shape[0] for ex in batch)
        B = len(batch)
        x_char = np.zeros((B, max_char))
        y_mgc = np.ones((B, max_mel, 80)) * -5
        x_speaker = np.zeros((B, 1))
        y_dur = np.zeros((B, max_char))
        y_pitch = np.ones((B, max_mel)) * self._ignore_index
        y_frame2phone = []
        for ii, ex in enumerate(batch):
            meta = ex['meta']
            y_mgc[ii, :ex['mgc'].shape[0], :] = ex['mgc']
            x_speaker[ii] = self._encodings.speaker2int[meta['speaker']] + 1
            for jj, ph in enumerate(meta['phones']):
                if ph in self._encodings.phon2int:
                    x_char[ii, jj] = self._encodings.phon2int[ph] + 1
            y_frame2phone.append(meta['frame2phon'])
            for p in meta['frame2phon']:
                y_dur[ii, p] += 1
            y_dur[ii, len(meta['phones']):] = self._ignore_index
            y_pitch[ii, :ex['pitch'].shape[0]] = ex['pitch']
        return {'x_char': torch.tensor(x_char, dtype=torch.long), 'x_speaker': torch.tensor(x_speaker, dtype=torch.long),
                'y_mgc': torch.tensor(y_mgc, dtype=torch.float), 'y_frame2phone': y_frame2phone,
                'y_pitch': torch.tensor(y_pitch, dtype=torch.long), 'y_dur': torch.tensor(y_dur, dtype=torch.long)}
