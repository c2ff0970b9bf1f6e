"""Segment feed of the HiFi-GAN trainer (hifigan/train.py): a training corpus that lives on the device and a gather that cuts a whole batch of
random crops out of it in ONE launch (csrc/segment_feed.hip; tests/segment_feed_reference.py restates it in numpy).

    SegmentCorpus   all utterances' audio as one int16 arena (one hour at 24 kHz is 172 MB), a float32 gain per utterance (upstream's
                    `normalize(audio) * 0.95`, with the int16 scale folded in: a sample is rounded once), optionally a frame-major float32 mel arena
                    holding the `.mgc` / GTA rows as they sit on disk
    epoch_plan      the sampler.  It stays on the host and is counter-based: epoch e of seed s draws from RandomState([s, e]) and from nothing else,
                    so a run resumed in the middle of an epoch draws what the uninterrupted run would have drawn

`build_tables` and `epoch_plan` are plain numpy; nothing here imports the extension until `SegmentCorpus.gather` runs, and there is no CPU path for
the gather."""
import math

import numpy as np

MEL_PAD = math.log(1e-5)      # the generator's own floor: log(clamp(mel, min=1e-5))
LN10 = math.log(10.0)         # .mgc rows are log10: log(10 ** x) = x ln 10 (io_utils/runtime.py::synthesize_devset)
ALIGN = 8                     # every utterance starts on a multiple of 8 samples: the kernel's 16-byte load path (hop = 240 keeps start * hop on one)


def utterance_gain(audio_i16):
    """float32(0.95 / peak) with the peak in int16 units — `normalize(audio) * 0.95` of a file read as int16 / 32768, the 1/32768 folded in; 0 for
    an all-zero file"""
    peak = int(np.abs(np.asarray(audio_i16, dtype=np.int32)).max()) if len(audio_i16) else 0
    return np.float32(0.95 / peak) if peak > 0 else np.float32(0.0)


def build_tables(items, hop=240, n_mels=80):
    """items: sequence of (audio int16 [L], mel float32 [F, n_mels] or None) — all with a mel or none ->
    dict(wav int16 [N], wav_off int64 [U + 1], length int64 [U], gain float32 [U], mel float32 [sum F, n_mels] or None, mel_off int64 [U + 1],
    n_frames int64 [U]).  wav_off[u + 1] - wav_off[u] is the utterance's length rounded up to a multiple of 8, the slack zero: samples past an
    utterance's end read as 0 either way.  n_frames[u] is the mel's own row count, or L // hop without one."""
    items = list(items)
    if not items:
        raise ValueError('build_tables: no items')
    with_mel = items[0][1] is not None
    if any((m is not None) != with_mel for _, m in items):
        raise ValueError('build_tables: either every item carries a mel or none does')
    U = len(items)
    length = np.zeros((U,), np.int64)
    wav_off = np.zeros((U + 1,), np.int64)
    mel_off = np.zeros((U + 1,), np.int64)
    for u, (a, m) in enumerate(items):
        a = np.asarray(a)
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError('build_tables: item %d: audio must be a 1-d int16 array (got %s %s)' % (u, a.dtype, a.shape))
        length[u] = a.shape[0]
        wav_off[u + 1] = wav_off[u] + -(-a.shape[0] // ALIGN) * ALIGN
        if with_mel:
            m = np.asarray(m)
            if m.ndim != 2 or m.shape[1] != n_mels:
                raise ValueError('build_tables: item %d: mel must be [frames, %d] (got %s)' % (u, n_mels, m.shape))
            mel_off[u + 1] = mel_off[u] + m.shape[0]
    wav = np.zeros((int(wav_off[U]),), np.int16)
    gain = np.zeros((U,), np.float32)
    mel = np.zeros((int(mel_off[U]), n_mels), np.float32) if with_mel else None
    for u, (a, m) in enumerate(items):
        wav[wav_off[u]:wav_off[u] + length[u]] = a
        gain[u] = utterance_gain(a)
        if with_mel:
            mel[mel_off[u]:mel_off[u + 1]] = np.asarray(m, dtype=np.float32)
    n_frames = (mel_off[1:] - mel_off[:-1]) if with_mel else length // hop
    return dict(wav=wav, wav_off=wav_off, length=length, gain=gain, mel=mel, mel_off=mel_off, n_frames=n_frames.astype(np.int64))


def epoch_plan(seed, epoch, n_frames, frames):
    """-> (perm int64 [U], start int64 [U]): the order in which epoch `epoch` visits the utterances and each UTTERANCE's first frame in it,
    start[u] = floor(r_u max(F_u - frames, 0)) with one uniform r_u in [0, 1) per utterance: 0 <= start[u] <= max(F_u - frames, 0).  Both come from
    np.random.RandomState([seed, epoch]) alone.  (Upstream's fine-tuning rule is randint(0, F - frames - 1), from a generator whose state depends
    on everything drawn before.)"""
    n_frames = np.asarray(n_frames, dtype=np.int64)
    rs = np.random.RandomState([int(seed) & 0xffffffff, int(epoch)])
    perm = rs.permutation(n_frames.shape[0]).astype(np.int64)
    r = rs.random_sample(n_frames.shape[0])
    room = np.maximum(n_frames - int(frames), 0)
    start = np.minimum(np.floor(r * room).astype(np.int64), room)
    return perm, start


def epoch_batches(seed, epoch, n_frames, frames, batch_size, first=0):
    """the batches of one epoch from batch `first` on, as (utt int64 [B], start int64 [B]); the incomplete last batch is dropped, as upstream's
    DataLoader(drop_last=True) does.  epoch_batches(..., first=k) is the tail of epoch_batches(..., first=0)."""
    perm, start = epoch_plan(seed, epoch, n_frames, frames)
    for k in range(int(first), perm.shape[0] // int(batch_size)):
        utt = perm[k * batch_size:(k + 1) * batch_size]
        yield utt, start[utt]


class SegmentCorpus:
    """The device-resident corpus.  items as for build_tables; `gather(utt, start, frames)` -> (y [B, 1, frames hop], mel [B, n_mels, frames] or
    None) by one launch on the current stream."""

    def __init__(self, items, hop=240, n_mels=80, device='cuda:0'):
        import torch

        from .. import _lib
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.TTSCError('SegmentCorpus lives on a HIP device (got %s); the gather has no CPU path' % (self.device,))
        self.hop, self.n_mels = int(hop), int(n_mels)
        t = build_tables(items, self.hop, self.n_mels)
        self.length, self.n_frames = t['length'], t['n_frames']
        self.num = int(self.length.shape[0])
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.wav = up(t['wav']) if t['wav'].shape[0] else torch.zeros((ALIGN,), dtype=torch.int16, device=self.device)
        self.wav_off, self.gain, self.mel_off = up(t['wav_off']), up(t['gain']), up(t['mel_off'])
        self.mel = None if t['mel'] is None else (up(t['mel']) if t['mel'].shape[0] else torch.zeros((1, self.n_mels), device=self.device))

    def gather(self, utt, start, frames, mel_scale=1.0, mel_pad=MEL_PAD, with_mel=None):
        """utt, start: B utterance numbers and first frames (host values: they are checked here and uploaded in one copy)"""
        import torch

        from .. import _lib
        utt, start = np.asarray(utt, dtype=np.int64).reshape(-1), np.asarray(start, dtype=np.int64).reshape(-1)
        B, frames = int(utt.shape[0]), int(frames)
        if B < 1 or start.shape[0] != B or frames < 1:
            raise _lib.TTSCError('SegmentCorpus.gather: %d utterances, %d starts, %d frames' % (B, start.shape[0], frames))
        if utt.min() < 0 or utt.max() >= self.num or start.min() < 0 or start.max() >= 1 << 31:
            raise _lib.TTSCError('SegmentCorpus.gather: an utterance number outside [0, %d) or a negative start frame' % self.num)
        with_mel = (self.mel is not None) if with_mel is None else bool(with_mel)
        if with_mel and self.mel is None:
            raise _lib.TTSCError('SegmentCorpus.gather: with_mel=True, but the corpus was built without mels')
        idx = torch.from_numpy(np.stack([utt, start]).astype(np.int32)).to(self.device)
        return segment_gather(self.wav, self.wav_off, self.gain, self.mel if with_mel else None, self.mel_off, idx[0], idx[1], frames, self.hop,
                              self.n_mels, mel_scale, mel_pad)


def segment_gather(wav, wav_off, gain, mel, mel_off, utt, start, frames, hop, n_mels, mel_scale=1.0, mel_pad=MEL_PAD):
    """The launch itself over device tensors (include/ttscube_hip.h::ttsc_segment_gather): wav int16 [N], wav_off / mel_off int64 [U + 1], gain
    float32 [U], mel float32 [sum F, n_mels] or None, utt / start int32 [B] -> (y [B, 1, frames hop], mel [B, n_mels, frames] or None).  The index
    tensors are the caller's promise (0 <= utt < U, start >= 0); SegmentCorpus.gather checks its host copies."""
    import ctypes as C

    import torch

    from .. import _lib
    dev = wav.device
    tables = [(wav, torch.int16), (wav_off, torch.int64), (gain, torch.float32), (mel_off, torch.int64), (utt, torch.int32), (start, torch.int32)]
    if mel is not None:
        tables.append((mel, torch.float32))
    for t, dt in tables:
        if not t.is_cuda:
            raise _lib.TTSCError('segment_gather: tensors must live on a HIP device (got %s); the gather has no CPU path' % (t.device,))
        assert t.dtype == dt and t.is_contiguous() and t.device == dev, 'segment_gather: a table has the wrong type, layout or device'
    B, frames, hop, n_mels = int(utt.numel()), int(frames), int(hop), int(n_mels)
    assert start.numel() == B and wav_off.numel() == mel_off.numel() == gain.numel() + 1
    y = torch.empty((B, 1, frames * hop), dtype=torch.float32, device=dev)
    out = torch.empty((B, n_mels, frames), dtype=torch.float32, device=dev) if mel is not None else None
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().ttsc_segment_gather(p(wav), p(wav_off), p(gain), p(mel), p(mel_off), p(utt), p(start), B, n_mels, frames, hop,
                                                  float(mel_scale), float(mel_pad), p(y), p(out), _lib.current_stream()), 'ttsc_segment_gather')
    return y, out
