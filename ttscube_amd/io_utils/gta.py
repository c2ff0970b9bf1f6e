"""Ground-truth-aligned (GTA) mels for vocoder fine-tuning: the Textcoder's TEACHER-FORCED mel of every training utterance, in the domain the
HiFi-GAN generator is fed at synthesis time (io_utils/runtime.py::synthesize_devset: `log(10 ** mel)` = mel ln 10), written as `<id>.npy`,
float32 [80, F] — the layout the public trainer's --fine_tuning reads (hifigan/train.py, --input-features gta).

The forward is the call synthesize_devset(forced_synthesis=True) makes, over padded batches.  Two things make a file independent of the batch it
was computed in:
  * the PreNet's dropout is always on; its masks come from a generator seeded by (seed, the item's position in the dataset), never from the batch
  * the post-net is a stack of k = 5 convolutions without length masks: in a padded batch the frames behind a short item's end would leak into
    its last ten frames.  The batched call's pre-post-net mel (output 2) is therefore cut to the item's own frames and the same post-net module is
    applied to it alone — for a batch of one that is output 3 itself."""
import math
import os

import numpy as np
import torch

LN10 = math.log(10.0)


def gta_dropout_masks(seed, index, steps):
    """the two PreNet masks [steps, 256] of dataset item `index` ({0, 1} float32, Bernoulli(0.5)), from a CPU generator seeded by (seed, index)"""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(index)) & 0x7fffffffffffffff)
    return [(torch.rand((int(steps), 256), generator=g) >= 0.5).float() for _ in range(2)]


def export_gta_mels(textcoder, collate, dataset, output_folder, batch=1, seed=0, limit=-1):
    """-> number of files written.  textcoder: a CubenetTextcoder on a HIP device (put into eval mode here); collate / dataset as for
    synthesize_devset."""
    os.makedirs(output_folder, exist_ok=True)
    textcoder.eval()
    p = int(textcoder._pframes)
    n = len(dataset) if limit == -1 or limit >= len(dataset) else limit
    batch = max(int(batch), 1)
    with torch.no_grad():
        for s in range(0, n, batch):
            exs = [dataset[i] for i in range(s, min(s + batch, n))]
            X = collate.collate_fn(exs)
            own = [(ex['mgc'].shape[0] // p) * p for ex in exs]                  # the frames the teacher-forced decoder emits for the item alone
            steps = X['y_mgc'].shape[1] // p + 1                                 # PreNet rows of the padded batch (textcoder.py:119-127)
            masks = [torch.zeros((len(exs), steps, 256)), torch.zeros((len(exs), steps, 256))]
            for j, ex in enumerate(exs):
                mj = gta_dropout_masks(seed, s + j, ex['mgc'].shape[0] // p + 1)
                for k in range(2):
                    masks[k][j, :mj[k].shape[0]] = mj[k]
            mel = textcoder(X, dropout_masks=masks)[2]
            for j, ex in enumerate(exs):
                post = textcoder._postnet(mel[j:j + 1, :own[j]].contiguous(), add_residual=True)[0]
                np.save(os.path.join(output_folder, ex['meta']['id'] + '.npy'), (post * LN10).t().contiguous().cpu().numpy().astype(np.float32))
    return n
