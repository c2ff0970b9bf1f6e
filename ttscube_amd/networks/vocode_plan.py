"""Planner of ``CubenetVocoder.synthesize_batch``: which rows the two WaveRNN nets decode for a LIST of utterances, and how the
high-resolution problem of every utterance is folded into rows and un-folded again — exactly as ``_inference_batch`` /
``_compose_batched_inference`` (vocoder.py:109-131) do for one utterance.  Plain Python and numpy: no torch, no HIP library, so a
machine without a GPU can import and test it.

The fold is expressed as gather indices into two flat sources, each with one pad element in front:
    mel source   row 0 = the pad frame (-5), then the frames of every utterance in input order
    x_low source [0]   = 0.0, then the low-resolution samples (24 per frame) of every utterance in input order
and the un-fold as gather indices into the concatenation of the launches' flattened [rows, L] outputs."""
from collections import namedtuple

import numpy as np

# one row of a high-resolution launch: chunk `chunk` of utterance `utt`; Philox key `seed`, counter word 2 `stream` (= the chunk: the
# batch position the row has when its utterance is folded alone)
Row = namedtuple('Row', 'utt chunk frames low_len out_len seed stream')
Utt = namedtuple('Utt', 'T nb frames_per_chunk low_per_chunk keep mel_off low_off seed')


class VocodePlan:
    def __init__(self, utts, rows, launches, lr_launches, upsample, upsample_low):
        self.utts = utts                  # per utterance, input order
        self.rows = rows                  # every (utterance, chunk), longest first
        self.launches = launches          # lists of indices into rows, at most max_rows each
        self.lr_launches = lr_launches    # lists of utterance indices (longest first), at most max_rows each
        self.upsample = upsample
        self.upsample_low = upsample_low

    # ---- low-resolution net: utterance i is one ragged row, stream 0, seed s_i ----
    def lr_tables(self, launch):
        us = [self.utts[i] for i in self.lr_launches[launch]]
        return [u.T for u in us], [u.seed for u in us], [0] * len(us)

    def lr_mel_index(self, launch):
        """[rows, Tmax] indices into the mel source (padding: the pad frame)"""
        us = [self.utts[i] for i in self.lr_launches[launch]]
        idx = np.zeros((len(us), max(u.T for u in us)), dtype=np.int64)
        for r, u in enumerate(us):
            idx[r, :u.T] = 1 + u.mel_off + np.arange(u.T)
        return idx

    # ---- high-resolution net ----
    def hr_tables(self, launch):
        rs = [self.rows[k] for k in self.launches[launch]]
        return [r.frames for r in rs], [r.low_len for r in rs], [r.seed for r in rs], [r.stream for r in rs]

    def fold_index(self, launch):
        """(mel [rows, Tmax], x_low [rows, Tlmax]) gather indices of one launch; padding points at the pad elements"""
        rs = [self.rows[k] for k in self.launches[launch]]
        im = np.zeros((len(rs), max(r.frames for r in rs)), dtype=np.int64)
        il = np.zeros((len(rs), max(r.low_len for r in rs)), dtype=np.int64)
        ul = self.upsample_low
        for k, r in enumerate(rs):
            u = self.utts[r.utt]
            f, s = u.frames_per_chunk, u.low_per_chunk
            if r.chunk == 0:   # chunk 0: pad frame, zero x_low prefix
                im[k, 1:f + 1] = 1 + u.mel_off + np.arange(f)
                il[k, ul:ul + s] = 1 + u.low_off + np.arange(s)
            else:              # the last frame / the last upsample_low samples of the chunk before
                im[k, :f + 1] = 1 + u.mel_off + r.chunk * f - 1 + np.arange(f + 1)
                il[k, :ul + s] = 1 + u.low_off + r.chunk * s - ul + np.arange(ul + s)
        return im, il

    def launch_width(self, launch):
        """L of a launch's [rows, L] output: out_len(Tmax, Tlmax)"""
        rs = [self.rows[k] for k in self.launches[launch]]
        return min(max(r.frames for r in rs) * self.upsample, max(r.low_len for r in rs) * self.upsample_low)

    def unfold_index(self):
        """per utterance: indices into the concatenation of the launches' flattened outputs — every chunk without its first `upsample`
        samples, chunks in order"""
        where = {}
        base = 0
        for li, launch in enumerate(self.launches):
            W = self.launch_width(li)
            for k, ri in enumerate(launch):
                r = self.rows[ri]
                where[(r.utt, r.chunk)] = base + k * W
            base += len(launch) * W
        out = []
        for i, u in enumerate(self.utts):
            out.append(np.concatenate([where[(i, c)] + self.upsample + np.arange(u.keep) for c in range(u.nb)]))
        return out

    def steps(self):
        """sequential decode steps: (of this plan: the longest row of every launch, low-resolution launches included; of the loop of
        single-utterance calls: 24 T_i + the folded row length, summed over the utterances)"""
        batch = sum(max(self.utts[i].T for i in l) * (self.upsample // self.upsample_low) for l in self.lr_launches)
        batch += sum(max(self.rows[k].out_len for k in l) for l in self.launches)
        loop = sum(u.T * (self.upsample // self.upsample_low) + u.keep + self.upsample for u in self.utts)
        return batch, loop


def plan_vocode(T_list, seeds, num_batches=20, max_rows=256, upsample=240, upsample_low=10):
    """T_list: mel frames per utterance; seeds: s_i per utterance."""
    if not len(T_list):
        raise ValueError('plan_vocode: no utterances')
    if len(seeds) != len(T_list):
        raise ValueError('plan_vocode: %d seeds for %d utterances' % (len(seeds), len(T_list)))
    if max_rows < 1 or num_batches < 1:
        raise ValueError('plan_vocode: max_rows and num_batches must be positive')
    per_frame = upsample // upsample_low       # low-resolution samples per mel frame (24)
    utts, rows = [], []
    mel_off = low_off = 0
    for i, T in enumerate(T_list):
        T = int(T)
        if T < 1:
            raise ValueError('plan_vocode: utterance %d has no frames' % i)
        nb = min(T, num_batches)
        f = T // nb                            # mel trimmed to a multiple of nb (vocoder.py:116)
        s = (T * per_frame) // nb              # x_low trimmed to a multiple of nb, independently (vocoder.py:117)
        frames, low_len = f + 1, s + upsample_low
        out_len = min(frames * upsample, low_len * upsample_low)
        utts.append(Utt(T, nb, f, s, out_len - upsample, mel_off, low_off, int(seeds[i])))
        rows += [Row(i, c, frames, low_len, out_len, int(seeds[i]), c) for c in range(nb)]
        mel_off += T
        low_off += T * per_frame
    rows.sort(key=lambda r: (-r.out_len, r.utt, r.chunk))
    launches = [list(range(k, min(k + max_rows, len(rows)))) for k in range(0, len(rows), max_rows)]
    order = sorted(range(len(utts)), key=lambda i: (-utts[i].T, i))
    lr_launches = [order[k:k + max_rows] for k in range(0, len(order), max_rows)]
    return VocodePlan(utts, rows, launches, lr_launches, upsample, upsample_low)
