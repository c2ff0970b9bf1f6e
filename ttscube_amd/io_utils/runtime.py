"""Mirror of the synthesis glue in cube/io_utils/runtime.py:
  cubegan_synthesize_dataset (:83-109)  Cubegan over a processed dev set -> <out>/<id>.wav (int16 @ 24 kHz), free or forced alignment
  synthesize_devset          (:41-80)   two-stage path: CubenetTextcoder -> log10-mel -> ln-mel -> HiFi-GAN Generator checkpoint
                                        (`ckpt['generator']`, config.json next to it, remove_weight_norm)
The PNG spectrogram rendering of the reference (PIL) is a debugging aid and is not reproduced."""
import json
import os

import numpy as np
import torch

from .audio import save_wav
from .io_cubegan import CubeganCollate, CubeganDataset


def cubegan_synthesize_batches(model, devset_path, limit=-1, free=True, conditioning=None, speaker=None, word_vectors=None, batch=1):
    """The synthesis behind cubegan_synthesize_dataset(batch > 1) and io_utils/evaluate.py: yields (ids, (wav [B, L] float32 in (-1, 1) ON THE DEVICE,
    sample counts)) for `batch` dev items at a time, collated and run through the ragged path of TTSCube.synthesize_batch
    (Cubegan.inference(return_lengths=True): each row equals its single-item call).  Forced alignment (free=False) has no ragged path: one item
    per yield."""
    collate = CubeganCollate(model._encodings, conditioning_type=conditioning, word_vectors=word_vectors)
    dataset = CubeganDataset(devset_path)
    m_gen = len(dataset) if limit == -1 or limit >= len(dataset) else limit
    step = max(int(batch), 1) if free else 1
    with torch.no_grad():
        for s in range(0, m_gen, step):
            exs = [dataset[ii] for ii in range(s, min(s + step, m_gen))]
            if speaker is not None:
                for ex in exs:
                    ex['meta']['speaker'] = speaker
            X = collate.collate_fn(exs)
            for key in X:
                if isinstance(X[key], torch.Tensor):
                    X[key] = X[key].to(model.get_device())
            if len(exs) == 1:
                wav = (model.inference(X) if free else model(X)).detach().reshape(1, -1)
                lens = [int(wav.shape[1])]
            else:
                wav, lens = model.inference(X, return_lengths=True)
                wav = wav.detach()[:, 0]
            yield [ex['meta']['id'] for ex in exs], (wav, lens)


def cubegan_synthesize_dataset(model, output_path, devset_path, limit=-1, free=True, conditioning=None, speaker=None, word_vectors=None, batch=1):
    """batch (an addition): 1 = the reference's item-by-item loop; above 1, `batch` items are collated at a time and run as one ragged call
    (free=True only), each file equal to what the loop writes."""
    if batch > 1:
        if not free:
            raise ValueError('cubegan_synthesize_dataset: batch > 1 runs the ragged inference path and needs free=True')
        os.makedirs(output_path, exist_ok=True)
        m_gen = 0
        for ids, (wav, lens) in cubegan_synthesize_batches(model, devset_path, limit=limit, free=True, conditioning=conditioning, speaker=speaker,
                                                           word_vectors=word_vectors, batch=batch):
            wav = wav.cpu().numpy()
            for j, i in enumerate(ids):
                save_wav('{0}/{1}.wav'.format(output_path, i), np.asarray(wav[j, :lens[j]] * 32767, dtype=np.int16), 24000)
            m_gen += len(ids)
        return m_gen
    collate = CubeganCollate(model._encodings, conditioning_type=conditioning, word_vectors=word_vectors)
    dataset = CubeganDataset(devset_path)
    m_gen = len(dataset) if limit == -1 or limit >= len(dataset) else limit
    os.makedirs(output_path, exist_ok=True)
    with torch.no_grad():
        for ii in range(m_gen):
            ex = dataset[ii]
            if speaker is not None:
                ex['meta']['speaker'] = speaker
            X = collate.collate_fn([ex])
            for key in X:
                if isinstance(X[key], torch.Tensor):
                    X[key] = X[key].to(model.get_device())
            audio = model.inference(X) if free else model(X)
            audio = audio.detach().cpu().numpy().squeeze()
            save_wav('{0}/{1}.wav'.format(output_path, ex['meta']['id']), np.asarray(audio * 32767, dtype=np.int16), 24000)
    return m_gen


def load_generator_checkpoint(vocoder_path):
    """runtime.py:44-54: config.json beside the checkpoint, state under 'generator', weight norm removed, eval mode"""
    from ..hifigan.env import AttrDict
    from ..hifigan.models import Generator
    h = AttrDict(json.loads(open(os.path.join(os.path.split(vocoder_path)[0], 'config.json')).read()))
    vocoder = Generator(h)
    vocoder.load_state_dict(torch.load(vocoder_path, map_location='cpu')['generator'])
    vocoder.remove_weight_norm()
    return vocoder.eval()


def synthesize_devset(textcoder, collate, dataset, vocoder, output_path='generated_files/', forced_synthesis=True, limit=-1, dropout_masks=None):
    """runtime.py:41-80 with the loaded objects passed in (textcoder: CubenetTextcoder on a HIP device; collate / dataset: whatever
    produces its batch dicts — the reference's TextcoderDataset / TextcoderCollate are corpus tooling; vocoder: from
    load_generator_checkpoint, on the same device).  dropout_masks (optional, one tensor per item): PreNet dropout masks to inject instead of
    the in-kernel Philox draw — the PreNet's dropout is always on (modules.py:159-164), so reproducible synthesis (tests, A/B listening)
    needs them."""
    os.makedirs(output_path, exist_ok=True)
    m_gen = len(dataset) if limit == -1 or limit >= len(dataset) else limit
    with torch.no_grad():
        for ii in range(m_gen):
            ex = dataset[ii]
            X = collate.collate_fn([ex])
            mk = dropout_masks[ii] if dropout_masks is not None else None
            mel = textcoder(X, dropout_masks=mk)[3] if forced_synthesis else textcoder.inference(X, dropout_masks=mk)
            mel = torch.log(10 ** mel)                       # log10-mel -> natural-log mel (runtime.py:77)
            audio = vocoder(mel.permute(0, 2, 1).contiguous()).detach().cpu().numpy().squeeze()
            save_wav('{0}/{1}.wav'.format(output_path, ex['meta']['id']), np.array(audio * 32767, dtype=np.int16), 24000)
    return m_gen
