"""Forced alignment of text to audio (NOT in the reference, which reads TextGrids that Montreal Forced Aligner wrote): recordings and their
transcripts in, word and phone intervals out, so that scripts/import_textgrid.py can build a corpus without a tool from outside.
csrc/forced_align.hip holds the search and the statistics; tests/forced_align_reference.py states all of it in numpy.

What it is — read before comparing boundaries:
  * Monophones, `n_sub` left-to-right sub-states per phone, ONE diagonal Gaussian per sub-state over 26 features: DCT-II coefficients 0 .. 12 of
    this project's 80-bin log-mel (io_utils/melspec.py::melspectrogram_log10, times ln 10; c0 is kept, silence needs it) and their centred deltas.
  * Trained by Viterbi re-estimation in closed form from a flat start (a uniform segmentation): no gradient, no neural acoustic model.
  * Silence (phone 0, 'sil') is optional before the first word, between words and behind the last.
  * No triphones, no mixtures, no speaker adaptation, no pronunciation variants, no beam pruning.  Nothing here claims MFA's boundaries.
A frame is `hop` samples; an utterance of L samples has L // hop frames (the convention of io_utils/evaluate.py).  A boundary between frames t - 1
and t is written at (t - 0.5) hop / sample_rate; the first boundary is 0 and the last the file's duration."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib

SAMPLE_RATE, HOP, N_FFT, N_MELS, N_CEP = 24000, 240, 1024, 80, 13
N_FEAT = 2 * N_CEP
SMAX = 1024                         # lattice positions per utterance: the kernel's limit (include/ttscube_hip.h)
SIL = 'sil'
VAR_FLOOR = 0.01
VAR_TINY = 1e-8                     # (a feature that never varies must not make a variance of zero)

_tables = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


# ---- features ----------------------------------------------------------------------------------------------------------------------------------------

def dct_table(n_coef=N_CEP, n_bins=N_MELS):
    """rows 0 .. n_coef - 1 of the orthonormal DCT-II over n_bins points: float64 [n_coef, n_bins], T T^T = I"""
    c = np.arange(n_coef, dtype=np.float64)[:, None]
    m = np.arange(n_bins, dtype=np.float64)[None, :]
    t = math.sqrt(2.0 / n_bins) * np.cos(math.pi * c * (m + 0.5) / n_bins)
    t[0] = math.sqrt(1.0 / n_bins)
    return t


def align_features(logmel10, nframes):
    """[B, F, 80] log10-mel and nframes [B] int32, both on the device -> [B, F, 26] float32: cepstra 0 .. 12 of ln(10) * logmel10 (the table is
    built in float64 on the host and rounded once; the product runs on ttsc_linear_forward) and the deltas (c[t+1] - c[t-1]) / 2 with the frame
    index clamped to the utterance's own 0 .. nframes - 1.  Rows at or behind nframes are zero.  A row has the same bits alone and in any batch."""
    if not logmel10.is_cuda:
        raise _lib.TTSCError('align_features: input must live on a HIP device; no CPU path')
    x = logmel10.float().contiguous()
    B, F, nb = x.shape
    key = (nb, str(x.device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.ascontiguousarray((math.log(10.0) * dct_table(N_CEP, nb)).astype(np.float32))).to(x.device)
    c = torch.empty((B, F, N_CEP), dtype=torch.float32, device=x.device)
    if B * F == 0:
        return torch.zeros((B, F, N_FEAT), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().ttsc_linear_forward(_lib.dev_ptr(x), _lib.dev_ptr(_tables[key]), None, _lib.dev_ptr(c), B * F, N_CEP, nb, nb, N_CEP,
                                                  _lib.ACT_NONE, 0, _lib.current_stream()), 'ttsc_linear_forward')
    n = nframes.to(x.device).long().clamp(min=0, max=F)[:, None]
    t = torch.arange(F, device=x.device)[None, :]
    last = (n - 1).clamp(min=0)
    nxt = torch.minimum(t + 1, last)[:, :, None].expand(B, F, N_CEP)
    prv = torch.minimum((t - 1).clamp(min=0), last)[:, :, None].expand(B, F, N_CEP)
    delta = (torch.gather(c, 1, nxt) - torch.gather(c, 1, prv)) * 0.5
    out = torch.cat([c, delta], dim=2)
    return torch.where((t < n)[:, :, None], out, torch.zeros_like(out)).contiguous()


# ---- lattices ----------------------------------------------------------------------------------------------------------------------------------------

def build_lattice(prons, n_sub):
    """prons: the phone ids (>= 1; 0 is silence) of every word of ONE utterance, in order; a token without phones (punctuation) contributes no
    positions.  Model state id = phone id * n_sub + sub-state.  -> dict of numpy arrays over the S lattice positions, left to right:
         state int32, skip int32 (one extra predecessor < j, or -1), start / final uint8,
         word int32 (index into prons, -1 for silence), unit int32 (running number of the phone or silence block the position belongs to),
         phone int32 (phone id of that block).
    Every phone is n_sub positions; an optional silence block stands before the first word (with phones), between such words and behind the last:
    `start` is set on the first position and on the first behind the leading silence, `final` on the last position and on the last before the
    trailing silence, `skip` leads from the first position behind an inner silence block to the last position before it.  No word with phones:
    an empty lattice."""
    if n_sub < 1:
        raise ValueError('build_lattice: n_sub must be at least 1, got %r' % (n_sub,))
    spoken = [(w, [int(p) for p in ph]) for w, ph in enumerate(prons) if len(ph)]
    cols = {k: [] for k in ('state', 'skip', 'start', 'final', 'word', 'unit', 'phone')}
    if not spoken:
        return {k: np.zeros((0,), np.uint8 if k in ('start', 'final') else np.int32) for k in cols}
    unit = 0

    def block(phone, word, skip_first=-1):
        nonlocal unit
        for s in range(n_sub):
            cols['state'].append(phone * n_sub + s)
            cols['skip'].append(skip_first if s == 0 else -1)
            cols['start'].append(0)
            cols['final'].append(0)
            cols['word'].append(word)
            cols['unit'].append(unit)
            cols['phone'].append(phone)
        unit += 1

    block(0, -1)
    cols['start'][0] = 1
    for k, (w, phones) in enumerate(spoken):
        jump = -1
        if k > 0:
            jump = len(cols['state']) - 1                 # the last position before the inner silence
            block(0, -1)
        for i, ph in enumerate(phones):
            if ph < 1:
                raise ValueError('build_lattice: phone ids of words start at 1 (0 is silence), got %r' % (ph,))
            block(ph, w, jump if i == 0 else -1)
        if k == 0:
            cols['start'][n_sub] = 1
    cols['final'][-1] = 1
    block(0, -1)
    cols['final'][-1] = 1
    return {k: np.asarray(v, np.uint8 if k in ('start', 'final') else np.int32) for k, v in cols.items()}


def pack_lattices(lattices, Smax=None):
    """a list of build_lattice results -> host arrays state, skip [B, Smax] int32 (-1 behind npos), start, final [B, Smax] uint8, npos [B] int32"""
    B = len(lattices)
    Smax = max([len(l['state']) for l in lattices] + [1]) if Smax is None else Smax
    out = {'state': np.full((B, Smax), -1, np.int32), 'skip': np.full((B, Smax), -1, np.int32), 'start': np.zeros((B, Smax), np.uint8),
           'final': np.zeros((B, Smax), np.uint8), 'npos': np.asarray([len(l['state']) for l in lattices], np.int32)}
    for b, l in enumerate(lattices):
        for k in ('state', 'skip', 'start', 'final'):
            out[k][b, :len(l[k])] = l[k]
    return out


def flat_alignment(nframes, npos, Tmax):
    """the flat start: frame t of an utterance with T >= S frames lies on position t * S // T (a uniform segmentation over ALL positions, optional
    silences included) -> (align [B, Tmax] int32 with -1 behind T, ok [B] int32: 0 where T < S or S == 0)"""
    B = len(nframes)
    align = np.full((B, Tmax), -1, np.int32)
    ok = np.zeros((B,), np.int32)
    for b in range(B):
        T, S = int(nframes[b]), int(npos[b])
        if S > 0 and T >= S:
            align[b, :T] = (np.arange(T, dtype=np.int64) * S) // T
            ok[b] = 1
    return align, ok


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------------------------

def upload_lattice(lat, M, device):
    """host arrays of pack_lattices -> device tensors, after ttsc_fa_check_lattice has seen them (a bad skip is an out-of-bounds read)"""
    host = {k: np.ascontiguousarray(lat[k]) for k in ('state', 'skip', 'start', 'final', 'npos')}
    for k, dt in (('state', np.int32), ('skip', np.int32), ('start', np.uint8), ('final', np.uint8), ('npos', np.int32)):
        if host[k].dtype != dt:
            raise ValueError('upload_lattice: %s must be %s, got %s' % (k, np.dtype(dt).name, host[k].dtype))
    B, Smax = host['state'].shape
    if any(host[k].shape != (B, Smax) for k in ('skip', 'start', 'final')) or host['npos'].shape != (B,):
        raise ValueError('upload_lattice: state, skip, start, final [B, Smax] and npos [B] expected')
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)
    _lib.check(_lib.lib().ttsc_fa_check_lattice(ptr(host['state']), ptr(host['skip']), ptr(host['start']), ptr(host['final']), ptr(host['npos']), B,
                                                Smax, M), 'ttsc_fa_check_lattice')
    return {k: torch.from_numpy(v).to(device) for k, v in host.items()}


def _check_dev(name, pairs):
    for t, dt in pairs:
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.TTSCError('%s: expected contiguous %s tensors on a HIP device' % (name, dt))


def viterbi(feat, nframes, lat, mean, ivar, cst):
    """feat [B, Tmax, D] float32, nframes [B] int32, lat: upload_lattice(...), mean / ivar [M, D], cst [M] float32, all on the device ->
    {'align' [B, Tmax] int32, 'score' [B] float32, 'ok' [B] int32} on the device (ttsc_fa_viterbi, one launch, no synchronisation)"""
    _check_dev('viterbi', [(feat, torch.float32), (nframes, torch.int32), (lat['state'], torch.int32), (lat['skip'], torch.int32),
                           (lat['start'], torch.uint8), (lat['final'], torch.uint8), (lat['npos'], torch.int32), (mean, torch.float32),
                           (ivar, torch.float32), (cst, torch.float32)])
    B, Tmax, D = feat.shape
    Smax, M = lat['state'].shape[1], mean.shape[0]
    if lat['state'].shape[0] != B or nframes.numel() != B or mean.shape != (M, D) or ivar.shape != (M, D) or cst.shape != (M,):
        raise ValueError('viterbi: feat [B, Tmax, D], nframes [B], lattice [B, Smax], mean / ivar [M, D], cst [M] expected')
    dev = feat.device
    out = {'align': torch.empty((B, Tmax), dtype=torch.int32, device=dev), 'score': torch.empty((B,), dtype=torch.float32, device=dev),
           'ok': torch.empty((B,), dtype=torch.int32, device=dev)}
    L = _lib.lib()
    nbytes = int(L.ttsc_fa_workspace_bytes(B, Tmax, Smax))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.ttsc_fa_viterbi(_p(feat), _p(nframes), _p(lat['state']), _p(lat['skip']), _p(lat['start']), _p(lat['final']), _p(lat['npos']),
                                     _p(mean), _p(ivar), _p(cst), B, Tmax, Smax, D, M, _p(ws), nbytes, _p(out['align']), _p(out['score']),
                                     _p(out['ok']), _lib.current_stream()), 'ttsc_fa_viterbi')
    return out


def accumulate(feat, nframes, align, ok, lat, count, total, sumsq):
    """adds the statistics of one aligned batch into the running float64 device tables count [M], total [M, D], sumsq [M, D] (ttsc_fa_accumulate)"""
    _check_dev('accumulate', [(feat, torch.float32), (nframes, torch.int32), (align, torch.int32), (ok, torch.int32), (lat['state'], torch.int32),
                              (lat['npos'], torch.int32), (count, torch.float64), (total, torch.float64), (sumsq, torch.float64)])
    B, Tmax, D = feat.shape
    Smax, M = lat['state'].shape[1], count.shape[0]
    if align.shape != (B, Tmax) or ok.numel() != B or lat['state'].shape[0] != B or total.shape != (M, D) or sumsq.shape != (M, D):
        raise ValueError('accumulate: feat [B, Tmax, D], align [B, Tmax], ok [B], lattice [B, Smax], count [M], sum / sumsq [M, D] expected')
    L = _lib.lib()
    nbytes = int(L.ttsc_fa_accumulate_workspace_bytes(B, Smax, D))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=feat.device)
    with _lib.on_device(feat.device):
        _lib.check(L.ttsc_fa_accumulate(_p(feat), _p(nframes), _p(align), _p(ok), _p(lat['state']), _p(lat['npos']), B, Tmax, Smax, D, M, _p(ws),
                                        nbytes, _p(count), _p(total), _p(sumsq), _lib.current_stream()), 'ttsc_fa_accumulate')


# ---- the model (host, float64) -----------------------------------------------------------------------------------------------------------------------

def global_stats(count, total, sumsq):
    """float64 tables -> (global mean [D], global variance [D]) over every frame counted"""
    n = count.sum()
    mean = total.sum(axis=0) / n
    var = sumsq.sum(axis=0) / n - mean * mean
    return mean, var


def reestimate(count, total, sumsq, prev_mean, prev_var, floor):
    """mean = sum / count, var = max(sumsq / count - mean^2, floor) for the states that got frames; the others keep prev_mean / prev_var"""
    mean, var = prev_mean.copy(), prev_var.copy()
    for m in np.nonzero(count > 0)[0]:
        mu = total[m] / count[m]
        mean[m] = mu
        var[m] = np.maximum(sumsq[m] / count[m] - mu * mu, floor)
    return mean, var


def kernel_model(mean, var):
    """float64 mean / var [M, D] -> the float32 tables of the search: mean, ivar = 1 / var, cst = -0.5 (D ln 2 pi + sum ln var)"""
    D = mean.shape[1]
    cst = -0.5 * (D * math.log(2.0 * math.pi) + np.log(var).sum(axis=1))
    return mean.astype(np.float32), (1.0 / var).astype(np.float32), cst.astype(np.float32)


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------------------

def intervals(align, lattice, words, phones, hop, sample_rate, duration):
    """one utterance: align [T] positions per frame, lattice: its build_lattice result, words: the marks of prons' words, phones: mark per phone id
    -> (word intervals, phone intervals) as lists of (mark, start s, end s); silences carry the empty mark, a silence block without a frame
    writes nothing, both tiers are contiguous from 0 to duration"""
    unit, word, phone = lattice['unit'], lattice['word'], lattice['phone']
    T = len(align)
    runs = []                                                     # (unit, word, phone id, first frame)
    for t in range(T):
        u = int(unit[align[t]])
        if not runs or runs[-1][0] != u:
            runs.append((u, int(word[align[t]]), int(phone[align[t]]), t))
    edge = [0.0] + [(r[3] - 0.5) * hop / sample_rate for r in runs[1:]] + [float(duration)]
    ph_iv = [('' if r[2] == 0 else phones[r[2]], edge[i], edge[i + 1]) for i, r in enumerate(runs)]
    wd_iv = []
    for i, r in enumerate(runs):
        if wd_iv and r[1] >= 0 and wd_iv[-1][3] == r[1]:
            wd_iv[-1] = (wd_iv[-1][0], wd_iv[-1][1], edge[i + 1], r[1])
        else:
            wd_iv.append(('' if r[1] < 0 else words[r[1]], edge[i], edge[i + 1], r[1]))
    return [iv[:3] for iv in wd_iv], ph_iv


# ---- the aligner -------------------------------------------------------------------------------------------------------------------------------------

class ForcedAligner:
    """Trains and applies the monophone Gaussian aligner on one HIP device.  phones: the phone inventory (silence is added as id 0).
    Items are dicts with 'audio' (a float array in [-1, 1] at sample_rate, or a wav path), 'words' (the marks) and 'prons' (the phone symbols of
    each word, [] for a token that is not spoken); 'id' is optional (default: the index)."""

    def __init__(self, phones, n_sub=3, device='cuda:0', sample_rate=SAMPLE_RATE, hop_size=HOP, features=None, search=None, statistics=None):
        self.phones = [SIL] + [p for p in phones if p != SIL]
        if len(set(self.phones)) != len(self.phones):
            raise ValueError('ForcedAligner: the phone list holds a symbol twice')
        self.phone_id = {p: i for i, p in enumerate(self.phones)}
        self.n_sub, self.sample_rate, self.hop = int(n_sub), int(sample_rate), int(hop_size)
        self.device = torch.device(device)
        self.M, self.D = len(self.phones) * self.n_sub, N_FEAT
        self.mean = self.var = self.floor = None
        # (the CPU tests check the glue around the kernels with injected host restatements; nothing else ever passes them)
        self._features = features if features is not None else self._device_features
        self._search = search if search is not None else viterbi
        self._statistics = statistics if statistics is not None else accumulate

    # ---- input -----------------------------------------------------------------------------------------------------------------------------------
    def _audio(self, item):
        a = item['audio']
        if isinstance(a, str):
            from .audio import load_wav
            a = load_wav(a, self.sample_rate)[0]
        return np.asarray(a, dtype=np.float32).reshape(-1)

    def _device_features(self, wavs):
        """waveforms -> (features [B, F, 26] on the device, frames per row [B] int32 on the device): one melspectrogram_log10 call for the batch;
        every row carries its own reflection behind its end, as in corpus_import.import_audio, so that it is analysed as it is alone"""
        from . import melspec
        half = N_FFT // 2
        lens = [int(w.shape[0]) for w in wavs]
        Lmax = max(lens + [1])
        rows = np.zeros((len(wavs), Lmax + half), dtype=np.float32)
        for r, w in enumerate(wavs):
            rows[r, :lens[r]] = w
            if lens[r] > half:
                rows[r, lens[r]:lens[r] + half] = w[-2:-2 - half:-1]
        F = Lmax // self.hop
        nf = torch.tensor([l // self.hop for l in lens], dtype=torch.int32).to(self.device)
        mel = melspec.melspectrogram_log10(torch.from_numpy(rows).to(self.device), sample_rate=self.sample_rate, num_mels=N_MELS, hop_size=self.hop,
                                           n_fft=N_FFT)[:, :F].contiguous()
        return align_features(mel, nf), nf

    def lattice(self, item):
        unknown = sorted({p for ph in item['prons'] for p in ph if p not in self.phone_id or p == SIL})
        if unknown:
            raise ValueError('ForcedAligner: phones outside the inventory: %s' % ' '.join(unknown))
        return build_lattice([[self.phone_id[p] for p in ph] for ph in item['prons']], self.n_sub)

    def _batches(self, items, batch):
        for s in range(0, len(items), batch):
            part = items[s:s + batch]
            wavs = [self._audio(it) for it in part]
            lats = [self.lattice(it) for it in part]
            if max(len(l['state']) for l in lats) > SMAX:
                raise ValueError('ForcedAligner: an utterance needs more than %d lattice positions; cut the recordings into sentences' % SMAX)
            feat, nf = self._features(wavs)
            yield {'ids': [it.get('id', s + k) for k, it in enumerate(part)], 'items': part, 'lattices': lats, 'samples': [len(w) for w in wavs],
                   'feat': feat, 'nframes': nf, 'lat': upload_lattice(pack_lattices(lats), self.M, feat.device)}

    def _tables(self):
        dev, z = self.device, torch.zeros
        return z(self.M, dtype=torch.float64, device=dev), z((self.M, self.D), dtype=torch.float64, device=dev), \
            z((self.M, self.D), dtype=torch.float64, device=dev)

    def _model(self):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in kernel_model(self.mean, self.var)]

    # ---- training --------------------------------------------------------------------------------------------------------------------------------
    def fit(self, items, iterations=4, batch=32, log=None, trace=None):
        """Flat start (a uniform segmentation, its statistics through ttsc_fa_accumulate; the global mean and variance become every state's first
        parameters and 0.01 x the global variance the floor), then `iterations` times: Viterbi, accumulate, re-estimate on the host in float64.  A
        state without a frame keeps its previous parameters.  The features of the corpus stay on the device between the iterations.
        trace (a list, for tests): gets one dict per step — the flat start, then every iteration — with the parameters after it ('mean', 'var') and
        the alignments they came from ('align' [rows of positions per frame], 'ok').
        -> one dict per iteration: 'score' (the sum over the feasible utterances), 'frames' (their frames), 'infeasible' (ids)"""
        batches = list(self._batches(items, batch))
        count, total, sumsq = self._tables()
        rows, oks = [], []
        for bt in batches:
            Tmax = bt['feat'].shape[1]
            al, ok = flat_alignment(bt['nframes'].cpu().numpy(), bt['lat']['npos'].cpu().numpy(), Tmax)
            if trace is not None:
                rows += [al[b, :int(n)].copy() for b, n in enumerate(bt['nframes'].cpu().numpy())]
                oks += ok.tolist()
            self._statistics(bt['feat'], bt['nframes'], torch.from_numpy(al).to(self.device), torch.from_numpy(ok).to(self.device), bt['lat'],
                             count, total, sumsq)
        c, s, q = count.cpu().numpy(), total.cpu().numpy(), sumsq.cpu().numpy()
        if c.sum() == 0:
            raise ValueError('ForcedAligner.fit: no utterance has as many frames as lattice positions')
        gmean, gvar = global_stats(c, s, q)
        self.floor = np.maximum(VAR_FLOOR * gvar, VAR_TINY)
        self.mean, self.var = reestimate(c, s, q, np.tile(gmean, (self.M, 1)), np.tile(np.maximum(gvar, self.floor), (self.M, 1)), self.floor)
        if trace is not None:
            trace.append({'mean': self.mean.copy(), 'var': self.var.copy(), 'align': rows, 'ok': oks})
        history = []
        for it in range(iterations):
            mean, ivar, cst = self._model()
            count, total, sumsq = self._tables()
            score, frames, infeasible, rows, oks = 0.0, 0, [], [], []
            for bt in batches:
                out = self._search(bt['feat'], bt['nframes'], bt['lat'], mean, ivar, cst)
                self._statistics(bt['feat'], bt['nframes'], out['align'], out['ok'], bt['lat'], count, total, sumsq)
                ok, sc, nf = out['ok'].cpu().numpy(), out['score'].cpu().numpy(), bt['nframes'].cpu().numpy()
                score += float(sc[ok != 0].astype(np.float64).sum())
                frames += int(nf[ok != 0].sum())
                infeasible += [i for i, k in zip(bt['ids'], ok) if k == 0]
                if trace is not None:
                    al = out['align'].cpu().numpy()
                    rows += [al[b, :int(n)].copy() for b, n in enumerate(nf)]
                    oks += ok.tolist()
            self.mean, self.var = reestimate(count.cpu().numpy(), total.cpu().numpy(), sumsq.cpu().numpy(), self.mean, self.var, self.floor)
            history.append({'score': score, 'frames': frames, 'infeasible': infeasible})
            if trace is not None:
                trace.append({'mean': self.mean.copy(), 'var': self.var.copy(), 'align': rows, 'ok': oks})
            if log is not None:
                log('iteration %d: score %.3f over %d frames (%.4f per frame), %d infeasible' % (it + 1, score, frames, score / max(frames, 1),
                                                                                               len(infeasible)))
        return history

    # ---- alignment -------------------------------------------------------------------------------------------------------------------------------
    def align(self, items, batch=32):
        """-> per item {'id', 'ok', 'score', 'duration', 'frames' (positions per frame), 'words', 'phones'}: word and phone intervals (mark, start s,
        end s), silences with the empty mark; an infeasible item has ok False and no intervals"""
        if self.mean is None:
            raise _lib.TTSCError('ForcedAligner.align: no model; call fit() or load() first')
        mean, ivar, cst = self._model()
        res = []
        for bt in self._batches(items, batch):
            out = self._search(bt['feat'], bt['nframes'], bt['lat'], mean, ivar, cst)
            al, ok, sc, nf = [out[k].cpu().numpy() for k in ('align', 'ok', 'score')] + [bt['nframes'].cpu().numpy()]
            for b, item in enumerate(bt['items']):
                dur = bt['samples'][b] / self.sample_rate
                rec = {'id': bt['ids'][b], 'ok': bool(ok[b]), 'score': float(sc[b]), 'duration': dur, 'frames': None, 'words': [], 'phones': []}
                if ok[b]:
                    rec['frames'] = al[b, :int(nf[b])].copy()
                    rec['words'], rec['phones'] = intervals(rec['frames'], bt['lattices'][b], item['words'], self.phones, self.hop,
                                                            self.sample_rate, dur)
                res.append(rec)
        return res

    # ---- files -----------------------------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """one .npz: the phone list, n_sub, the feature settings, means, variances and the variance floor"""
        if self.mean is None:
            raise _lib.TTSCError('ForcedAligner.save: no model')
        with open(path, 'wb') as f:
            np.savez(f, phones=np.asarray(self.phones), n_sub=np.int64(self.n_sub), sample_rate=np.int64(self.sample_rate), hop=np.int64(self.hop),
                     n_fft=np.int64(N_FFT), n_mels=np.int64(N_MELS), n_cep=np.int64(N_CEP), mean=self.mean, var=self.var, floor=self.floor)

    @classmethod
    def load(cls, path, device='cuda:0', **kw):
        with np.load(path, allow_pickle=False) as z:
            if (int(z['n_fft']), int(z['n_mels']), int(z['n_cep'])) != (N_FFT, N_MELS, N_CEP):
                raise ValueError('%s: the model was trained on other features (n_fft %d, n_mels %d, n_cep %d)'
                                 % (path, int(z['n_fft']), int(z['n_mels']), int(z['n_cep'])))
            phones = [str(p) for p in z['phones']]
            self = cls(phones[1:], n_sub=int(z['n_sub']), device=device, sample_rate=int(z['sample_rate']), hop_size=int(z['hop']), **kw)
            self.mean, self.var, self.floor = z['mean'].astype(np.float64), z['var'].astype(np.float64), z['floor'].astype(np.float64)
        if self.mean.shape != (self.M, self.D) or self.var.shape != (self.M, self.D):
            raise ValueError('%s: the tables do not fit %d phones x %d sub-states' % (path, len(phones), self.n_sub))
        return self


def to_textgrid(rec, text):
    """one result of ForcedAligner.align -> the TextGrid corpus_import.read_item expects: tier 0 'words', tier 1 'phones', tier 2 one interval
    holding the transcript"""
    from .textgrid import Interval, IntervalTier, TextGrid
    dur = float(rec['duration'])
    tier = lambda name, ivs: IntervalTier(name, 0.0, dur, [Interval(float(a), float(b), m) for m, a, b in ivs])
    return TextGrid(0.0, dur, [tier('words', rec['words']), tier('phones', rec['phones']), tier('text', [(text, 0.0, dur)])])
