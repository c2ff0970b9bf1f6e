"""Objective scores of a synthesized dev set against its recordings (NOT in the reference, which only writes wav files to listen to): both sides are
time-aligned by dynamic time warping over mel cepstra (csrc/dtw.hip, one launch for a ragged batch of pairs) and the warping path is turned into a
mel-cepstral distortion and F0 / voicing figures.  tests/dtw_reference.py states the alignment and the scores in numpy.

Definition — read before comparing numbers:
  * The cepstra are an orthonormal DCT-II over THIS project's 80-bin log-mel (io_utils/melspec.py::melspectrogram_log10, times ln 10), coefficients
    1 .. 24, c0 dropped.  That is a mel-cepstral distortion, but it is not SPTK's mel-generalised cepstrum: `mcd_db` is comparable between runs of
    this tool (two checkpoints, two conditionings, two builds of a kernel) and NOT with MCD figures from papers.
  * mcd_db = (10 sqrt 2 / ln 10) * (DTW cost) / (path length); the corpus value pools sum(cost) / sum(path length).
  * Silence is not trimmed and the path is not weighted by voice activity; the steps (1,1), (1,0), (0,1) are unweighted, without slope limits.
  * F0 figures come from io_utils/pitch.py::PitchTracker over the path cells where both sides are voiced; they are nan (never 0) where there is none.
A frame is `hop` samples; an utterance of L samples has L // hop frames on both the cepstral and the F0 side (the log-mel's last, partial frame is
left out so that one path indexes both)."""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from .. import _lib

SAMPLE_RATE, HOP, N_FFT, N_MELS, N_COEF = 24000, 240, 1024, 80, 24
MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)
SCORES = ('mcd_db', 'f0_rmse_hz', 'f0_rmse_cents', 'gpe', 'vde', 'dur_ratio', 'n_path', 'n_both_voiced')

_tables = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def dct_table(n_coef=N_COEF, n_bins=N_MELS):
    """rows 1 .. n_coef of the orthonormal DCT-II over n_bins points (c0, row 0, is dropped): float64 [n_coef, n_bins], T T^T = I"""
    c = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_bins, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / n_bins) * np.cos(math.pi * c * (m + 0.5) / n_bins)


def mel_cepstra(logmel10, n_coef=N_COEF):
    """[B, F, 80] log10-mel on the device -> [B, F, n_coef] float32: the DCT-II of ln(10) * logmel10, coefficients 1 .. n_coef.  The table is built in
    float64 on the host with ln(10) folded in and rounded once; the product runs on ttsc_linear_forward (as melspec.py::_gemm), no library GEMM."""
    if not logmel10.is_cuda:
        raise _lib.TTSCError('mel_cepstra: input must live on a HIP device; no CPU path')
    x = logmel10.float().contiguous()
    B, F, nb = x.shape
    if not 1 <= n_coef < nb:
        raise ValueError('mel_cepstra: n_coef must lie in 1 .. %d, got %r' % (nb - 1, n_coef))
    key = (n_coef, nb, str(x.device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.ascontiguousarray((math.log(10.0) * dct_table(n_coef, nb)).astype(np.float32))).to(x.device)
    y = torch.empty((B, F, n_coef), dtype=torch.float32, device=x.device)
    if B * F:
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().ttsc_linear_forward(_lib.dev_ptr(x), _lib.dev_ptr(_tables[key]), None, _lib.dev_ptr(y), B * F, n_coef, nb, nb, n_coef,
                                                      _lib.ACT_NONE, 0, _lib.current_stream()), 'ttsc_linear_forward')
    return y


def dtw_align(a, len_a, b, len_b):
    """a [P, Na, K], b [P, Nb, K] float32 and len_a, len_b [P] int32, all on the device -> dict of device tensors (ttsc_dtw_align, one launch, no
    synchronisation): cost [P] float32 (D at the end cell), plen [P] int32, path_a / path_b [P, Na + Nb - 1] int32 in forward order, -1 behind
    plen.  Local cost = Euclidean distance; steps (1,1), (1,0), (0,1); ties to the diagonal, then (i-1, j), then (i, j-1)."""
    for t, dt in ((a, torch.float32), (b, torch.float32), (len_a, torch.int32), (len_b, torch.int32)):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.TTSCError('dtw_align: expected contiguous %s tensors on a HIP device' % dt)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2] or len_a.numel() != a.shape[0] or len_b.numel() != a.shape[0]:
        raise ValueError('dtw_align: a [P, Na, K], b [P, Nb, K], len_a [P], len_b [P]; got %s %s %s %s'
                         % (tuple(a.shape), tuple(b.shape), tuple(len_a.shape), tuple(len_b.shape)))
    P, Na, K = a.shape
    Nb = b.shape[1]
    dev = a.device
    Lp = max(Na + Nb - 1, 0)
    out = {'cost': torch.empty((P,), dtype=torch.float32, device=dev), 'plen': torch.empty((P,), dtype=torch.int32, device=dev),
           'path_a': torch.empty((P, Lp), dtype=torch.int32, device=dev), 'path_b': torch.empty((P, Lp), dtype=torch.int32, device=dev)}
    L = _lib.lib()
    nbytes = int(L.ttsc_dtw_workspace_bytes(P, Na, Nb))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.ttsc_dtw_align(_p(a), _p(b), _p(len_a), _p(len_b), P, Na, Nb, K, _p(ws), nbytes, _p(out['cost']), _p(out['plen']),
                                    _p(out['path_a']), _p(out['path_b']), _lib.current_stream()), 'ttsc_dtw_align')
    return out


def _scores(s):
    """one pair's (or the pooled corpus') float64 sums -> the scores"""
    nan = float('nan')
    n, nb = int(s['n_path']), int(s['n_both_voiced'])
    return {'mcd_db': MCD_SCALE * s['cost'] / n if n else nan,
            'f0_rmse_hz': math.sqrt(s['sq_hz'] / nb) if nb else nan,
            'f0_rmse_cents': math.sqrt(s['sq_cents'] / nb) if nb else nan,
            'gpe': s['gross'] / nb if nb else nan,
            'vde': s['vdiff'] / n if n else nan,
            'dur_ratio': s['len_syn'] / s['len_ref'] if s['len_ref'] else nan,
            'n_path': n, 'n_both_voiced': nb}


_SUMS = ('cost', 'n_path', 'n_both_voiced', 'sq_hz', 'sq_cents', 'gross', 'vdiff', 'len_ref', 'len_syn')


def pool(sums):
    """the corpus scores of a list of per-pair sums (path_metrics()['sums'], possibly of several batches)"""
    return _scores({k: sum(s[k] for s in sums) for k in _SUMS})


def path_metrics(path_a, path_b, plen, cost, f0_ref, f0_syn, len_ref, len_syn):
    """The scores of P aligned pairs.  path_a / path_b [P, Lp] int32 index the reference's / the synthesized side's frames (-1 behind plen [P]),
    cost [P] is D at the end cell, f0_ref [P, >= Na] and f0_syn [P, >= Nb] are in Hz with 0 = unvoiced, len_ref / len_syn [P] count frames; all
    device tensors.  The values are gathered along the path and reduced in float64 on the device, one small copy brings the sums to the host.
    -> {'pairs': [scores per pair], 'sums': [the float64 sums per pair, what a corpus pools], 'corpus': pooled scores}:
         mcd_db          (10 sqrt 2 / ln 10) cost / plen;              corpus: sum cost / sum plen
         f0_rmse_hz, f0_rmse_cents   over the path cells where both sides are voiced (cents: 1200 log2(f_syn / f_ref))
         gpe             share of those cells with |f_syn / f_ref - 1| > 0.2
         vde             share of all path cells whose voicing differs
         dur_ratio       len_syn / len_ref
         n_path, n_both_voiced
       Without a both-voiced cell the three F0 figures are nan; an empty path makes mcd_db and vde nan."""
    P, Lp = path_a.shape
    dev = path_a.device
    valid = torch.arange(Lp, device=dev)[None, :] < plen[:, None]
    if Lp and f0_ref.shape[1] and f0_syn.shape[1]:
        fr = torch.gather(f0_ref.double(), 1, path_a.clamp(min=0).long().clamp(max=f0_ref.shape[1] - 1))
        fs = torch.gather(f0_syn.double(), 1, path_b.clamp(min=0).long().clamp(max=f0_syn.shape[1] - 1))
    else:
        fr = fs = torch.zeros((P, Lp), dtype=torch.float64, device=dev)
    vr, vs = (fr > 0) & valid, (fs > 0) & valid
    both = vr & vs
    one = torch.ones_like(fr)
    ratio = torch.where(both, fs, one) / torch.where(both, fr, one)
    zero = torch.zeros_like(fr)
    cols = [cost.double(), plen.double(), both.double().sum(1), torch.where(both, (fs - fr) ** 2, zero).sum(1),
            torch.where(both, (1200.0 * torch.log2(ratio)) ** 2, zero).sum(1), (both & ((ratio - 1.0).abs() > 0.2)).double().sum(1),
            (vr != vs).double().sum(1), len_ref.double(), len_syn.double()]
    host = torch.stack(cols, dim=1).cpu().numpy()
    sums = [{k: (float(v) if k in ('cost', 'sq_hz', 'sq_cents') else int(v)) for k, v in zip(_SUMS, row)} for row in host]
    return {'pairs': [_scores(s) for s in sums], 'sums': sums, 'corpus': pool(sums)}


def _fmt(name, s):
    return '%s mcd_db %.4f f0_rmse_hz %.3f f0_rmse_cents %.2f gpe %.4f vde %.4f dur_ratio %.4f n_path %d n_both_voiced %d' % (
        name, s['mcd_db'], s['f0_rmse_hz'], s['f0_rmse_cents'], s['gpe'], s['vde'], s['dur_ratio'], s['n_path'], s['n_both_voiced'])


class Evaluator:
    """Scores batches of (reference, synthesized) utterances on one HIP device."""

    def __init__(self, device='cuda:0', sample_rate=SAMPLE_RATE, hop_size=HOP, n_coef=N_COEF, fmin=60, fmax=400, aligner=None, cepstra=None):
        from .pitch import PitchTracker
        self._device = torch.device(device)
        self._sr, self._hop, self._n_coef, self._fmin, self._fmax = sample_rate, hop_size, n_coef, fmin, fmax
        self._tracker = PitchTracker(device)
        # (the CPU tests check the glue around the kernels with injected host restatements of the two; nothing else ever passes them)
        self._align = aligner if aligner is not None else dtw_align
        self._cepstra = cepstra if cepstra is not None else mel_cepstra

    # ---- analysis ----------------------------------------------------------------------------------------------------------------------------------
    def _lengths(self, lens, B, Lmax, what):
        lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        if len(lens) != B or any(v < 0 or v > Lmax for v in lens):
            raise ValueError('Evaluator: %s lengths must hold one value in [0, %d] per row' % (what, Lmax))
        return lens

    def analyse(self, x, lens):
        """x [B, Lmax] float32 waveforms in [-1, 1] on the device, lens: samples per row (host list) -> (log10-mel [B, F, 80], f0 [B, F] in Hz, frames
        per row [B] int32 on the device; F = Lmax // hop).  Every row is analysed as it is alone: it carries its own reflection behind its end, as
        in the importer (io_utils/corpus_import.py::import_audio)."""
        from . import melspec
        x = x.to(self._device, torch.float32)
        B, Lmax = x.shape
        half = N_FFT // 2
        ld = torch.tensor(lens, dtype=torch.int32).to(self._device)
        rows = torch.zeros((B, Lmax + half), dtype=torch.float32, device=self._device)
        rows[:, :Lmax] = x
        pos = torch.arange(Lmax + half, device=self._device)[None, :]
        l64 = ld.long()[:, None]
        src = (2 * l64 - 2 - pos).clamp(min=0)                       # sample L + k mirrors sample L - 2 - k
        tail = (pos >= l64) & (pos < l64 + half) & (l64 > half)
        rows = torch.where(tail, torch.gather(rows, 1, src.clamp(max=Lmax + half - 1)), torch.where(pos < l64, rows, torch.zeros_like(rows)))
        F = Lmax // self._hop
        mel = melspec.melspectrogram_log10(rows, sample_rate=self._sr, num_mels=N_MELS, hop_size=self._hop, n_fft=N_FFT)[:, :F].contiguous()
        f0 = self._tracker.f0_device(rows[:, :Lmax].contiguous(), ld, self._sr, self._hop, self._fmin, self._fmax) if F else \
            torch.zeros((B, 0), dtype=torch.float32, device=self._device)
        return mel, f0, torch.div(ld, self._hop, rounding_mode='floor').to(torch.int32)

    # ---- scoring -----------------------------------------------------------------------------------------------------------------------------------
    def evaluate_features(self, ref_mel, ref_f0, ref_frames, syn_mel, syn_f0, syn_frames):
        """log10-mels [P, F, 80], F0 tracks [P, F] and frame counts [P] int32 of both sides, on the device -> path_metrics(...) plus 'align' (the
        aligner's output)"""
        a, b = self._cepstra(ref_mel, self._n_coef), self._cepstra(syn_mel, self._n_coef)
        al = self._align(a, ref_frames, b, syn_frames)
        out = path_metrics(al['path_a'], al['path_b'], al['plen'], al['cost'], ref_f0, syn_f0, ref_frames, syn_frames)
        out['align'] = al
        return out

    def evaluate_audio(self, ref, ref_len, syn, syn_len):
        """two batches of waveforms [P, L] in [-1, 1] on the device with their sample counts; the log-mel and the F0 of both sides are computed here.
        -> {'pairs', 'sums', 'corpus', 'align'} (path_metrics)"""
        ref_len = self._lengths(ref_len, ref.shape[0], ref.shape[1], 'reference')
        syn_len = self._lengths(syn_len, syn.shape[0], syn.shape[1], 'synthesized')
        if ref.shape[0] != syn.shape[0]:
            raise ValueError('Evaluator: %d reference and %d synthesized utterances' % (ref.shape[0], syn.shape[0]))
        rm, rf, rn = self.analyse(ref, ref_len)
        sm, sf, sn = self.analyse(syn, syn_len)
        return self.evaluate_features(rm, rf, rn, sm, sf, sn)

    # ---- dev sets ----------------------------------------------------------------------------------------------------------------------------------
    def _reference_features(self, devset_path, ids):
        """the reference side of `ids`: <id>.mgc and <id>.pitch where both exist (cut to len(pitch) frames), else analysed from <id>.wav"""
        from .audio import load_wav
        mels, f0s = [None] * len(ids), [None] * len(ids)
        todo = []
        for k, i in enumerate(ids):
            base = os.path.join(devset_path, i)
            if os.path.exists(base + '.mgc') and os.path.exists(base + '.pitch'):
                mel = np.asarray(np.load(open(base + '.mgc', 'rb')), dtype=np.float32)
                f0 = np.asarray(np.load(open(base + '.pitch', 'rb')), dtype=np.float32)
                n = min(mel.shape[0], f0.shape[0])
                mels[k], f0s[k] = torch.from_numpy(mel[:n].copy()), torch.from_numpy(f0[:n].copy())
            else:
                todo.append(k)
        if todo:
            wavs = [np.asarray(load_wav(os.path.join(devset_path, ids[k]) + '.wav', self._sr)[0], dtype=np.float32) for k in todo]
            m, f, n = self._analyse_list(wavs)
            for r, k in enumerate(todo):
                mels[k], f0s[k] = m[r, :int(n[r])], f[r, :int(n[r])]
        return self._pad_features(mels, f0s)

    def _analyse_list(self, wavs):
        lens = [int(w.shape[0]) for w in wavs]
        x = torch.zeros((len(wavs), max(lens + [1])), dtype=torch.float32)
        for r, w in enumerate(wavs):
            x[r, :lens[r]] = torch.as_tensor(w, dtype=torch.float32)
        m, f, n = self.analyse(x.to(self._device), lens)
        return m, f, n.tolist()

    def _pad_features(self, mels, f0s):
        n = [int(m.shape[0]) for m in mels]
        F = max(n + [1])
        mel = torch.zeros((len(mels), F, N_MELS), dtype=torch.float32, device=self._device)
        f0 = torch.zeros((len(mels), F), dtype=torch.float32, device=self._device)
        for r, (m, f) in enumerate(zip(mels, f0s)):
            mel[r, :n[r]] = m.to(self._device)
            f0[r, :n[r]] = f.to(self._device)
        return mel, f0, torch.tensor(n, dtype=torch.int32).to(self._device)

    @staticmethod
    def devset_ids(devset_path):
        """ids of a processed folder: every <id>.json with an <id>.wav, or an <id>.mgc and <id>.pitch, beside it; sorted"""
        have = set(os.listdir(devset_path))
        ids = [f[:-5] for f in sorted(have) if f.endswith('.json')]
        return [i for i in ids if i + '.wav' in have or (i + '.mgc' in have and i + '.pitch' in have)]

    def evaluate_devset(self, devset_path, generated, batch=32, limit=-1, free=True, conditioning=None, word_vectors=None, speaker=None, log=None):
        """devset_path: a processed folder (<id>.json / .mgc / .pitch / .wav).  generated: a folder of <id>.wav files, or a Cubegan — then the dev
        set is synthesized here, `batch` utterances per padded call (free=True; forced alignment runs them one by one), and the audio stays on the
        device between synthesis and scoring.  -> {'corpus': {...}, 'items': [{'id', ...scores}]}; log (optional): called with one line per item
        and the corpus line."""
        from .audio import load_wav
        if isinstance(generated, (str, os.PathLike)):
            ids = [i for i in self.devset_ids(devset_path) if os.path.exists(os.path.join(generated, i + '.wav'))]
            ids = ids if limit == -1 else ids[:limit]
            groups = ((ids[s:s + batch], None) for s in range(0, len(ids), batch))
        else:
            from .runtime import cubegan_synthesize_batches
            groups = cubegan_synthesize_batches(generated, devset_path, limit=limit, free=free, conditioning=conditioning, speaker=speaker,
                                                word_vectors=word_vectors, batch=batch)
        items, sums = [], []
        for gids, audio in groups:
            if audio is None:
                wavs = [np.asarray(load_wav(os.path.join(generated, i + '.wav'), self._sr)[0], dtype=np.float32) for i in gids]
                sm, sf, sn = self._analyse_list(wavs)
                sn = torch.tensor(sn, dtype=torch.int32).to(self._device)
            else:
                wav, lens = audio
                sm, sf, sn = self.analyse(wav, lens)
            rm, rf, rn = self._reference_features(devset_path, gids)
            res = self.evaluate_features(rm, rf, rn, sm, sf, sn)
            for i, s in zip(gids, res['pairs']):
                items.append(dict(id=i, **s))
                if log is not None:
                    log(_fmt(i, s))
            sums += res['sums']
        corpus = pool(sums)
        if log is not None:
            log(_fmt('corpus (%d items)' % len(items), corpus))
        return {'corpus': corpus, 'items': items}


def write_json(result, path):
    """the result of evaluate_devset as JSON (nan figures become null)"""
    clean = lambda d: {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in d.items()}
    with open(path, 'w') as f:
        json.dump({'corpus': clean(result['corpus']), 'items': [clean(it) for it in result['items']]}, f, indent=1)
