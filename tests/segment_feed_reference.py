"""Float32 numpy restatement of the segment gather (include/ttscube_hip.h::ttsc_segment_gather), element by element; no import from ttscube_amd.

    y[b, 0, i]   = float32(wav[wav_off[u] + s hop + i]) * gain[u]          0 at and beyond wav_off[u + 1]
    mel[b, c, t] = mel_arena[mel_off[u] + s + t, c] * float32(mel_scale)   float32(mel_pad) where s + t >= mel_off[u + 1] - mel_off[u]

One float32 product per element (numpy multiplies two float32 scalars in float32, rounded once)."""
import numpy as np


def gather(wav, wav_off, gain, mel, mel_off, utt, start, frames, hop, mel_scale, mel_pad):
    B = len(utt)
    n = frames * hop
    y = np.zeros((B, 1, n), np.float32)
    out = None
    if mel is not None:
        n_mels = mel.shape[1]
        out = np.full((B, n_mels, frames), np.float32(mel_pad), np.float32)
    for b in range(B):
        u, s = int(utt[b]), int(start[b])
        lo, end = int(wav_off[u]) + s * hop, int(wav_off[u + 1])
        for i in range(n):
            if lo + i < end:
                y[b, 0, i] = np.float32(wav[lo + i]) * np.float32(gain[u])
        if mel is not None:
            F = int(mel_off[u + 1] - mel_off[u])
            for t in range(frames):
                if s + t < F:
                    out[b, :, t] = mel[int(mel_off[u]) + s + t].astype(np.float32) * np.float32(mel_scale)
    return y, out
