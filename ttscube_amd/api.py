"""Mirror of cube/api.py: ``TTSCube.load(model_name)`` / ``TTSCube(model_path, phonemizer_path)`` /
``tts(text, speaker) -> np.int16 @ 24 kHz``.

The text front-end: when ``<phonemizer_path>.encodings`` and ``<phonemizer_path>.model`` exist, plain text is phonemized by
``io_utils.io_text.Text2FeatBlizzard`` (the reference's tokenizer + character tagger, on the HIP kernels); when the files are a word-level G2P
(JSON ``.encodings`` with ``token2int``, ``.best`` / ``.model`` and ``.lexicon``) by ``io_utils.io_text.Text2Feat``.  ``text2feat`` = any
callable ``text -> {'phones': [...], 'words': [...], 'phon2word': [...]}`` overrides it (the reference's Text2Feat* objects
satisfy it); with neither, the text is read as whitespace-separated phoneme symbols.
New on top of the reference (B=1 only): ``synthesize_batch`` runs many sentences per call, length-bucketed, and
``shard`` splits a sentence list across ranks (one process per GPU, no collectives).

A model trained with ``conditioning: fasttext:<lang>`` (the yaml's key) needs the word-vector table it was trained with: ``word_vectors=`` takes a path
(.vec / .npz) or a ``WordVectors``; by default ``<model_path>.vectors.npz`` (what the trainer writes: the corpus vocabulary) or ``<model_path>.vec`` is read when present.  The front end's ``words`` are
looked up there; at run time a sentence has no left or right context, so ``x_phon2word`` is the front end's ``phon2word`` itself.

``TTSCubeTwoStage(textcoder_path, vocoder)`` (not in the reference) is the same interface over the two-stage path: CubenetTextcoder -> mel -> a HiFi-GAN generator
checkpoint (or a Griffin-Lim / WaveRNN vocoder object), one sentence or a list, reproducible per sentence through ``seed``."""
import os
from pathlib import Path

import numpy as np
import torch
import yaml

from . import _lib
from .io_utils.io_cubegan import CubeganCollate, CubeganEncodings
from .networks.cubegan import Cubegan


def _per_text(v, n, name):
    """a call-level control: a scalar for every text, or one value per text"""
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != n:
            raise ValueError('%s: %d values for %d texts' % (name, len(v), n))
        return list(v)
    return [v] * n


def _plan_prosody(texts, rate, pitch, pitch_range, markup):
    """What the prosody arguments ask for.  None: nothing — no markup, every control at its identity —, the caller stays on the
    uncontrolled path.  Else (units, layout): units = [(text index, segment index, tag-free text, spans)], one batch row each (the segments of
    a text between its <break>s; a text without markup is one unit whose single span is the call-level Prosody); layout[i] = what text i is
    joined from, in order: ('unit', u) / ('pause', samples)."""
    from .io_utils.prosody import Prosody, Segment, parse_markup
    n = len(texts)
    rates, pitches, ranges, marks = (_per_text(v, n, k) for v, k in ((rate, 'rate'), (pitch, 'pitch'), (pitch_range, 'pitch_range'), (markup, 'markup')))
    bases = [Prosody(r, p, g) for r, p, g in zip(rates, pitches, ranges)]
    if not any(marks) and all(b.is_identity() for b in bases):
        return None
    units, layout = [], []
    for i, (text, base, mk) in enumerate(zip(texts, bases, marks)):
        segs = parse_markup(text, base) if mk else [Segment(text, [(0, len(text), base)])]
        parts = []
        for j, seg in enumerate(segs):
            if len(segs) == 1 or seg.text.strip():          # (a segment without text — two breaks in a row — takes no batch row)
                parts.append(('unit', len(units)))
                units.append((i, j, seg.text, seg.spans))
            if seg.pause_samples() > 0:
                parts.append(('pause', seg.pause_samples()))
        layout.append(parts)
    return units, layout


def _join_units(layout, waves, device):
    """per text: its units' float32 device waveforms with the pauses' zero samples between them, joined on the device"""
    out = []
    for parts in layout:
        ws = [waves[v] if kind == 'unit' else torch.zeros(v, dtype=torch.float32, device=device) for kind, v in parts]
        out.append(ws[0] if len(ws) == 1 else (torch.cat([w.reshape(-1) for w in ws]) if ws else torch.zeros(0, dtype=torch.float32, device=device)))
    return out


def _plan_loudness(loudness, peak_db, n):
    """loudness=None: None, and nothing of io_utils/loudness.py is imported or launched.  Else (targets, peaks): one LUFS target and one
    true-peak ceiling in dB per text"""
    if loudness is None:
        return None
    return ([float(v) for v in _per_text(loudness, n, 'loudness')], [float(v) for v in _per_text(peak_db, n, 'peak_db')])


def _normalize_padded(wav, lens, ids, plan, sample_rate, log=None):
    """one padded batch [B, 1, L] of device waveforms, row j being text ids[j] -> the same batch brought to its texts' loudness targets (measure,
    finish and apply: io_utils/loudness.py, no host synchronisation).  log: a dict that receives, under the batch's ids, its small per-row device
    results (zbar, gain, limited, silent) — a batch that is run again, after a tripped range guard, replaces its entry"""
    from .io_utils.loudness import meter
    B, L = wav.shape[0], wav.shape[-1]
    if B == 0 or L == 0:
        return wav
    x = wav.detach().reshape(B, L).contiguous()
    ld = torch.tensor([int(v) for v in lens], dtype=torch.int32).pin_memory().to(x.device, non_blocking=True)
    y, st = meter(x.device).normalize_device(x, ld, sample_rate, [plan[0][i] for i in ids], peak_db=[plan[1][i] for i in ids], inplace=False)
    if log is not None:
        log[tuple(ids)] = {k: st[k] for k in ('zbar', 'gain', 'limited', 'silent')}
    return y.reshape(B, 1, L)


def _loudness_report(log, n):
    """the per-text reports of the last call with a loudness target, read back from the device: [{lufs_in, gain_db, peak_limited, silent}] (None
    for a text that had no sample)"""
    import math
    from .io_utils.loudness import lufs
    out = [None] * n
    for ids, st in log.items():
        z, g = lufs(st['zbar'].cpu().numpy()), st['gain'].cpu().numpy()
        lim, sil = st['limited'].cpu().numpy(), st['silent'].cpu().numpy()
        for j, i in enumerate(ids):
            out[i] = {'lufs_in': float(z[j]), 'gain_db': 20.0 * math.log10(float(g[j])), 'peak_limited': bool(lim[j]), 'silent': bool(sil[j])}
    return out


def _normalize_in_groups(waves, plan, sample_rate, device, max_batch, log=None):
    """_normalize_waves over the whole list, `max_batch` texts per padded batch"""
    step = max(1, int(max_batch))
    out = list(waves)
    for s in range(0, len(out), step):
        out[s:s + step] = _normalize_waves(out[s:s + step], plan, sample_rate, device, log, first=s)
    return out


def _normalize_waves(waves, plan, sample_rate, device, log=None, first=0):
    """a list of 1-D device waveforms (texts first, first + 1, ...: sentences joined from their <break> segments are measured as the joined unit)
    -> the list at the texts' loudness targets, through one padded batch"""
    lens = [int(w.numel()) for w in waves]
    if not lens or max(lens) == 0:
        return waves
    x = torch.zeros((len(waves), 1, max(lens)), dtype=torch.float32, device=device)
    for i, w in enumerate(waves):
        x[i, 0, :lens[i]] = w.reshape(-1)
    y = _normalize_padded(x, lens, list(range(first, first + len(waves))), plan, sample_rate, log)
    return [y[i, 0, :lens[i]] for i in range(len(waves))]


def _control_rows(metas, texts, spans, n_phones):
    """the per-phone control arrays of one padded batch, in its row order: (dur_scale float64 [B, N], pitch_mul float32 [B, N], pitch_range
    float32 [B]); padding phones carry the identity"""
    from .io_utils.prosody import phone_controls
    B = len(metas)
    ds, pm, pr = np.ones((B, n_phones), np.float64), np.ones((B, n_phones), np.float32), np.ones((B,), np.float32)
    for b, (meta, text, sp) in enumerate(zip(metas, texts, spans)):
        c = phone_controls(meta, text, sp)
        k = len(c['dur_scale'])
        ds[b, :k], pm[b, :k], pr[b] = c['dur_scale'], c['pitch_mul'], c['pitch_range']
    return ds, pm, pr


class PhoneText2Feat:
    """Fallback front-end: 'text' is a whitespace-separated phoneme string; '|' separates words."""

    def __call__(self, text):
        words, phones, p2w = [], [], []
        for wi, w in enumerate(text.split('|')):
            words.append(w.strip())
            for p in w.split():
                phones.append(p)
                p2w.append(wi)
        return {'orig_text': text, 'words': words, 'phones': phones, 'phon2word': p2w}


class TTSCube:
    SAMPLE_RATE = 24000

    def __init__(self, model_path: str, phonemizer_path: str = None, text2feat=None, device='cuda:0', word_vectors=None):
        encodings = CubeganEncodings('{0}.encodings'.format(model_path))
        conf = yaml.load(open('{0}.yaml'.format(model_path)), yaml.Loader)
        cond_type = conf.get('conditioning')
        if cond_type in (None, 'none'):
            cond_type = None
        table = None
        if cond_type is not None and str(cond_type).startswith('fasttext'):
            from .io_utils.word_vectors import WordVectors
            if word_vectors is None:
                word_vectors = next((p for p in ('{0}.vectors.npz'.format(model_path), '{0}.vec'.format(model_path)) if os.path.exists(p)), None)
            if word_vectors is None:
                raise _lib.TTSCError("%s.yaml says conditioning: %s, but no word-vector table was given and neither %s.vec nor %s.vectors.npz exists; "
                                     "pass word_vectors= (a path or a WordVectors): the model cannot run without the vectors it was trained with"
                                     % (model_path, cond_type, model_path, model_path))
            table = WordVectors.resolve(word_vectors)
            if table.dim != 300:
                raise _lib.TTSCError('word_vectors: fasttext conditioning takes 300-d vectors, the table has %d' % table.dim)
        self._model = Cubegan(encodings, conditioning=cond_type, train=False)
        self._model.load('{0}.model'.format(model_path))
        self._collate = CubeganCollate(encodings, conditioning_type=cond_type, word_vectors=table)
        self._model.eval()
        self._model.to(device)
        self._text2feat = self._make_text2feat(phonemizer_path, text2feat, device)

    @staticmethod
    def _make_text2feat(phonemizer_path, text2feat, device):
        """the caller's front-end; else the word-level G2P (Text2Feat) when phonemizer_path holds one; else the sentence phonemizer (cube/api.py:31-32)
        when both of its files exist; else the phoneme-string reader"""
        if text2feat is not None:
            return text2feat
        g2p = TTSCube._g2p_files(phonemizer_path) if phonemizer_path is not None else None
        if g2p == 'complete':
            from .io_utils.io_text import Text2Feat
            return Text2Feat(phonemizer_path, device=device)
        if g2p == 'incomplete':         # a G2P's encodings without its lexicon or checkpoint: never the sentence tagger's files
            return PhoneText2Feat()
        if phonemizer_path is not None and all(os.path.exists('{0}.{1}'.format(phonemizer_path, ext)) for ext in ('encodings', 'model')):
            from .io_utils.io_text import Text2FeatBlizzard
            return Text2FeatBlizzard(phonemizer_path, device=device)
        return PhoneText2Feat()

    @staticmethod
    def _g2p_files(phonemizer_path):
        """the word-level G2P's files (the reference's en-* layout, cube/api.py:26-29 second branch): a JSON .encodings with a `token2int` key —
        the sentence tagger's has `grapheme2int` —, a .best or .model checkpoint and a .lexicon.
        -> 'complete', 'incomplete' (such an .encodings, but the lexicon or the checkpoint is missing) or None (not a G2P's encodings)"""
        import json
        f = lambda ext: '{0}.{1}'.format(phonemizer_path, ext)
        try:
            with open(f('encodings')) as fh:
                obj = json.load(fh)
        except (OSError, ValueError):
            return None
        if not (isinstance(obj, dict) and 'token2int' in obj):
            return None
        return 'complete' if os.path.exists(f('lexicon')) and (os.path.exists(f('best')) or os.path.exists(f('model'))) else 'incomplete'

    @staticmethod
    def _is_g2p(phonemizer_path):
        return TTSCube._g2p_files(phonemizer_path) == 'complete'

    @staticmethod
    def load(model_name: str, **kw):
        base_name = '{0}/.ttscube/models/{1}'.format(str(Path.home()), model_name)
        if not os.path.exists('{0}/cubegan.model'.format(base_name)):
            raise FileNotFoundError('%s/cubegan.{model,yaml,encodings} not found and this build has no network access to '
                                    'download it (cube/io_utils/repository.py:27-61); unpack the exported model there' % base_name)
        return TTSCube('{0}/cubegan'.format(base_name), '{0}/phonemizer'.format(base_name), **kw)      # (**kw: text2feat, device, word_vectors)

    def _example(self, text, speaker, feats=None):
        """The dummy-target example cube/api.py:47-57 builds around the front-end output (`feats`: that output, when the caller already has it)."""
        rez = {'meta': dict(self._text2feat(text) if feats is None else feats)}
        rez['meta']['speaker'] = speaker
        rez['pitch'] = np.zeros((100))
        rez['mgc'] = np.zeros((100, 80))
        rez['meta']['words_left'] = []
        rez['meta']['words_right'] = []
        rez['meta']['frame2phon'] = [0] * 100
        return rez

    def _attach_controls(self, X, metas, texts, spans):
        """the control tensors of one collated batch, built behind the collate in its row order (host tensors: Languasito2.inference converts and
        uploads them); a control that is at its identity in every row is left out, so that such a batch runs the uncontrolled launches"""
        ds, pm, pr = _control_rows(metas, texts, spans, X['x_char'].shape[1])
        if (ds != 1.0).any():
            X['x_dur_scale'] = torch.from_numpy(ds)
        if (pm != 1.0).any():
            X['x_pitch_mul'] = torch.from_numpy(pm)
        if (pr != 1.0).any():
            X['x_pitch_range'] = torch.from_numpy(pr)

    def __call__(self, text, speaker='none', rate=1.0, pitch=0.0, pitch_range=1.0, markup=False, loudness=None, peak_db=-1.0):
        """cube/api.py:45-66: one sentence -> int16 audio at 24 kHz.
        loudness (LUFS; None: the level the generator gives, nothing new runs) and peak_db (true-peak ceiling in dB): the sentence is brought
        to that integrated loudness on the device (io_utils/loudness.py) before the int16 conversion.
        rate (> 1 is faster; the duration scale 1 / rate is limited to [0.25, 4]), pitch (semitones), pitch_range (factor on the spread of the
        pitch around the sentence's voiced mean) and markup=True (`text` carries <prosody> / <break> tags: io_utils/prosody.py; the call-level
        values are then the outermost span) steer the duration and pitch launches of the model.  The pitch controls move the
        pitch INPUT of the conditioning recurrence; how closely the audio's F0 follows is a property of the trained model."""
        if loudness is not None:
            wav = self._synthesize_batch_device([text], speaker, 64, rate, pitch, pitch_range, markup, loudness, peak_db)[0]
            return np.asarray(wav.cpu().numpy() * 32767, dtype=np.int16)
        plan = _plan_prosody([text], rate, pitch, pitch_range, markup)
        if plan is None:
            return self._single(text, speaker)
        units, layout = plan
        if layout[0] == [('unit', 0)]:
            return self._single(units[0][2], speaker, units[0][3])
        wav = self._synthesize_batch_device([text], speaker, 64, rate, pitch, pitch_range, markup)[0]
        return np.asarray(wav.cpu().numpy() * 32767, dtype=np.int16)

    def _single(self, text, speaker, spans=None):
        """one sentence (or one segment of a marked-up one) on the single-sentence path; spans: its prosody spans, None = uncontrolled"""
        with torch.no_grad():
            ex = self._example(text, speaker)
            X = self._collate.collate_fn([ex])
            for key in X:
                if isinstance(X[key], torch.Tensor):
                    X[key] = X[key].to(self._model.get_device())
            if spans is not None:
                self._attach_controls(X, [ex['meta']], [text], [spans])
            # the generator's range guard runs deferred: nothing waits for the GPU until the audio is copied back — where a synchronisation happens
            # anyway — and the guard's verdict is collected right behind that copy; a tripped guard reruns the sentence with the self-repairing
            # synchronous check (re-calibration on this input)
            gen = self._model._generator
            tripped = False
            try:
                audio = self._model.inference(X, check='deferred')
                host = audio.detach().cpu()
            finally:
                # whatever happens between the deferred forward and here (an exception in the copy, a KeyboardInterrupt), the pending verdict is
                # collected: a stale one would be blamed on the next, unrelated call
                if gen.range_check_pending():
                    tripped = gen.finish_range_check(raise_on_trip=False)
            if tripped:
                host = self._model.inference(X, check='sync').detach().cpu()
            return np.asarray(host.numpy().squeeze() * 32767, dtype=np.int16)

    def synthesize_batch(self, texts, speaker='none', max_batch=64, rate=1.0, pitch=0.0, pitch_range=1.0, markup=False, loudness=None, peak_db=-1.0):
        """Many sentences -> list of int16 arrays (same order).  Sentences are sorted by phoneme count and run in
        padded batches of up to `max_batch`; ragged lengths are handled inside the kernels (masked BiLSTMs), so each
        result equals the single-sentence call — with word conditioning too: the collate's word counts (x_words_len) stop the word BiLSTMs at each
        sentence's own last word.
        rate / pitch / pitch_range / markup: as in `__call__`, each a scalar or one value per text; the segments of every marked-up text go
        through the same length-sorted groups as rows of their own, and entry i still equals the single call with text i's arguments.
        loudness / peak_db: as in `__call__`, a scalar or one value per text; measured and scaled on the device, batch by batch."""
        if loudness is not None or _plan_prosody(texts, rate, pitch, pitch_range, markup) is not None:
            return [np.asarray(w.cpu().numpy() * 32767, dtype=np.int16)
                    for w in self._synthesize_batch_device(texts, speaker, max_batch, rate, pitch, pitch_range, markup, loudness, peak_db)]
        out = [None] * len(texts)

        def collect(ids, wav, lens):
            wav = wav.detach().cpu().numpy()
            for j, i in enumerate(ids):
                out[i] = np.asarray(wav[j, 0, :lens[j]] * 32767, dtype=np.int16)

        self._run_groups(texts, speaker, max_batch, collect)
        return out

    def _synthesize_batch_device(self, texts, speaker='none', max_batch=64, rate=1.0, pitch=0.0, pitch_range=1.0, markup=False, loudness=None,
                                 peak_db=-1.0):
        """`synthesize_batch` without the copy to the host: -> list of 1-D float32 device tensors in (-1, 1), in input order, each trimmed to its
        own sample count (views of the padded batches; with <break>s the segments and their zero samples joined on the device).
        `np.asarray(t.cpu().numpy() * 32767, dtype=np.int16)` of an entry is that sentence's `synthesize_batch` result.  For callers that go on
        working on the device (story.StoryCube).  loudness / peak_db: every entry at its loudness target (a sentence without <break>s inside the
        padded batch it was generated in, one with <break>s as the joined unit)."""
        loud = _plan_loudness(loudness, peak_db, len(texts))
        if loud is not None:
            self._loud_log = (len(texts), {})
        plan = _plan_prosody(texts, rate, pitch, pitch_range, markup)
        if plan is not None:
            units, layout = plan
            speakers = speaker if isinstance(speaker, (list, tuple)) else [speaker] * len(texts)
            waves = [None] * len(units)

            def collect_units(ids, wav, lens):
                wav = wav.detach()
                for j, u in enumerate(ids):
                    waves[u] = wav[j, 0, :lens[j]]

            self._run_groups([u[2] for u in units], [speakers[u[0]] for u in units], max_batch, collect_units, spans=[u[3] for u in units])
            joined = _join_units(layout, waves, self._model.get_device())
            if loud is None:
                return joined
            return _normalize_in_groups(joined, loud, self.SAMPLE_RATE, self._model.get_device(), max_batch, self._loud_log[1])
        out = [None] * len(texts)

        def collect(ids, wav, lens):
            wav = wav.detach() if loud is None else _normalize_padded(wav, lens, ids, loud, self.SAMPLE_RATE, self._loud_log[1])
            for j, i in enumerate(ids):
                out[i] = wav[j, 0, :lens[j]]

        self._run_groups(texts, speaker, max_batch, collect)
        return out

    def loudness_report(self):
        """per text of the last call that had a loudness target: {lufs_in, gain_db, peak_limited, silent} (this reads the statistics back)"""
        n, log = getattr(self, '_loud_log', (0, {}))
        return _loudness_report(log, n)

    def _run_groups(self, texts, speaker, max_batch, collect, spans=None):
        """the grouping and the inference behind synthesize_batch: `collect(ids, wav [B, 1, L] on the device, sample counts)` is called once per
        padded batch, ids = the positions of its sentences in `texts`; after a tripped range guard it is called again for every batch.
        spans: per text, its prosody spans (io_utils/prosody.py) — the control tensors of a batch are attached behind its collate, so the
        controls of batch k + 1 travel with its text stack through the pipeline."""
        speakers = speaker if isinstance(speaker, (list, tuple)) else [speaker] * len(texts)
        # a front-end with a `batch` method (io_text.Text2FeatBlizzard) phonemizes the whole list in one padded call
        feats = self._text2feat.batch(list(texts)) if hasattr(self._text2feat, 'batch') else [None] * len(texts)
        ex = [self._example(t, s, f) for t, s, f in zip(texts, speakers, feats)]
        order = sorted(range(len(ex)), key=lambda i: len(ex[i]['meta']['phones']))
        groups = [order[s:s + max_batch] for s in range(0, len(order), max_batch)]

        def feed():
            for ids in groups:
                X = self._collate.collate_fn([ex[i] for i in ids])
                for key in X:
                    if isinstance(X[key], torch.Tensor):
                        X[key] = X[key].to(self._model.get_device())
                if spans is not None:
                    self._attach_controls(X, [ex[i]['meta'] for i in ids], [texts[i] for i in ids], [spans[i] for i in ids])
                yield X

        def collect_all(results):
            for ids, (wav, lens) in zip(groups, results):
                collect(ids, wav, lens)

        with torch.no_grad():
            if len(groups) > 1:
                # several padded batches: the text / frame stacks of batch k + 1 run under the generator of batch k (Cubegan.inference_pipelined);
                # per-batch results are the ones `inference` gives.  The pipeline runs the range guard deferred; a batch that left the calibrated
                # range raises there, and the whole list is then redone batch by batch with the self-repairing synchronous guard.
                try:
                    collect_all(self._model.inference_pipelined(feed()))
                    return
                except _lib.TTSCError as e:
                    if 'check="sync"' not in str(e):
                        raise
            collect_all(self._model.inference(X, return_lengths=True) for X in feed())

    @staticmethod
    def shard(items, rank, world_size):
        """Contiguous utterance shard for one rank (inference is embarrassingly parallel: no collectives)."""
        n = len(items)
        lo, hi = rank * n // world_size, (rank + 1) * n // world_size
        return items[lo:hi]


class TTSCubeTwoStage:
    """Text to speech over the two-stage path (NOT in the reference, whose only consumer of a trained Textcoder walks a processed dev set:
    io_utils/runtime.py::synthesize_devset): text -> phones -> CubenetTextcoder -> log10-mel -> natural-log mel -> vocoder.

    textcoder_path: the base scripts/train_textcoder.py writes — `<base>.yaml` (pframes, sample_rate, hop_size), `<base>.encodings`, `<base>.best`
    (else `<base>.last`).  vocoder: a HiFi-GAN generator checkpoint path (io_utils.runtime.load_generator_checkpoint: config.json beside it), or
    any object with synthesize_devset's `vocoder` contract (natural-log mel [B, 80, F] on the device -> audio [B, 1, L] on the device:
    io_utils.vocoder.GriffinLimVocoder / WaveRNNVocoder).  The front end is TTSCube's (phonemizer_path / text2feat / the phone-string reader).

    The PreNet's dropout is always on (cube/networks/modules.py:159-164), so a sentence's audio is a function of (text, speaker, seed): `seed` is
    the Philox key of its AR decode.  Sentence i of a `synthesize_batch` list gets key seed + i wherever it lands after length-sorting and
    grouping, and equals `tts(texts[i], seed=seed + i)` (DESIGN.md §9m states the limit of that equality)."""

    def __init__(self, textcoder_path: str, vocoder, phonemizer_path: str = None, text2feat=None, device='cuda:0'):
        from .io_utils.io_textcoder import TextcoderEncodings
        from .networks.textcoder import CubenetTextcoder
        conf = yaml.load(open('{0}.yaml'.format(textcoder_path)), yaml.Loader) or {}
        self.sample_rate = int(conf.get('sample_rate', 24000))
        self._device = torch.device(device)
        self._encodings = TextcoderEncodings('{0}.encodings'.format(textcoder_path))
        ckpt = next((p for p in ('{0}.best'.format(textcoder_path), '{0}.last'.format(textcoder_path)) if os.path.exists(p)), None)
        if ckpt is None:
            raise FileNotFoundError('%s.best / %s.last: no Textcoder checkpoint (scripts/train_textcoder.py writes them)' % (textcoder_path, textcoder_path))
        self._model = CubenetTextcoder(self._encodings, pframes=int(conf.get('pframes', 3)))
        self._model.load(ckpt)
        self._model.eval()
        self._model.to(self._device)
        if isinstance(vocoder, (str, os.PathLike)):
            from .io_utils.runtime import load_generator_checkpoint
            vocoder = load_generator_checkpoint(str(vocoder)).to(self._device)
        self._vocoder = vocoder
        import inspect
        try:
            fn = vocoder.forward if isinstance(vocoder, torch.nn.Module) else vocoder.__call__
            self._takes_frames = 'frames' in inspect.signature(fn).parameters
        except (TypeError, ValueError):
            self._takes_frames = False
        self._is_generator = hasattr(vocoder, 'finish_range_check') and hasattr(vocoder, 'range_check_pending')
        self._text2feat = TTSCube._make_text2feat(phonemizer_path, text2feat, device)
        self.last_stats = {}

    # ---- text -> batch dict ---------------------------------------------------------------------------------------------------------------
    def _phones(self, text, feats=None):
        return list((self._text2feat(text) if feats is None else feats)['phones'])

    def _speaker_id(self, speaker):
        """TextcoderCollate's id + 1; a speaker the encodings do not know is the padding row 0 ('none': TTSCube's default)"""
        return self._encodings.speaker2int[speaker] + 1 if speaker in self._encodings.speaker2int else 0

    def _collate(self, phones, speakers):
        """x_char (phone id + 1, unknown phones 0 — io_textcoder.TextcoderCollate), x_speaker, and x_len: id 0 is both padding and an unknown phone"""
        n = max(max((len(p) for p in phones), default=0), 1)
        x_char = torch.zeros((len(phones), n), dtype=torch.long)
        for b, ps in enumerate(phones):
            for j, ph in enumerate(ps):
                x_char[b, j] = self._encodings.phon2int[ph] + 1 if ph in self._encodings.phon2int else 0
        x_speaker = torch.tensor([[self._speaker_id(s)] for s in speakers], dtype=torch.long)
        return {'x_char': x_char, 'x_speaker': x_speaker, 'x_len': torch.tensor([len(p) for p in phones], dtype=torch.long)}

    # ---- mel -> audio ---------------------------------------------------------------------------------------------------------------------
    def _vocode(self, mel_cm, frames, check):
        """log10-mel [B, 80, Fmax] (zeros past frames[b]) -> list of B 1-D float32 device tensors, each its sentence's own samples (empty for a
        sentence without a frame).  mel -> torch.log(10 ** mel) as synthesize_devset does; with a vocoder whose call takes `frames=` the rows
        that have frames go in ONE ragged call, otherwise every sentence is vocoded on its own trimmed mel."""
        B = mel_cm.shape[0]
        out = [torch.zeros(0, dtype=torch.float32, device=mel_cm.device) for _ in range(B)]
        act = [b for b in range(B) if frames[b] > 0]
        if not act:
            return out
        ln = torch.log(10 ** mel_cm)
        voc = self._vocoder
        if not self._takes_frames:
            for b in act:
                out[b] = voc(ln[b:b + 1, :, :frames[b]].contiguous()).detach().reshape(-1)
            return out
        if len(act) < B:
            ln = ln.index_select(0, torch.tensor(act, dtype=torch.int64, device=ln.device))
        fr = [frames[b] for b in act]
        ln = ln[:, :, :max(fr)].contiguous()
        if self._is_generator:
            wav = voc(ln, frames=fr, check=check).detach()
            lens = [int(voc.out_len(f)) for f in fr]
        else:
            wav = voc(ln, frames=fr).detach()
            lens = list(getattr(voc, 'last_lengths', None) or [wav.shape[-1]] * len(act))
        for j, b in enumerate(act):
            out[b] = wav[j, 0, :lens[j]]
        return out

    def _run(self, X, seeds, members=None, max_rows=None):
        """one padded batch -> list of per-sentence device waveforms; the generator's range guard runs deferred and its verdict is collected right
        behind the forward's last use, as TTSCube.__call__ collects it — a tripped guard redoes the vocoding with the self-repairing check"""
        mel, frames, st = self._model.inference_batch(X, seeds=seeds, members=members, max_rows=max_rows, channel_major=True, return_stats=True)
        self.last_stats = st
        if not self._is_generator:
            return self._vocode(mel, frames, None)
        gen, tripped = self._vocoder, False
        try:
            wavs = self._vocode(mel, frames, 'deferred')
        finally:
            if gen.range_check_pending():
                tripped = gen.finish_range_check(raise_on_trip=False)
        if tripped:
            wavs = self._vocode(mel, frames, 'sync')
        return wavs

    @staticmethod
    def _seed(seed):
        return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)

    @staticmethod
    def _int16(wav):
        return np.asarray(wav.detach().cpu().numpy().reshape(-1) * 32767, dtype=np.int16)

    SEGMENT_KEY_STRIDE = 0x9E3779B97F4A7C15      # (odd: distinct segments of a text never share a key)

    @classmethod
    def _segment_key(cls, key, j):
        """the Philox key of segment j (between <break>s) of a text whose key is `key`: (key + j * 0x9E3779B97F4A7C15) mod 2**63 — segment 0, and
        so every text without a break, keeps `key` itself"""
        return (int(key) + int(j) * cls.SEGMENT_KEY_STRIDE) % (2 ** 63)

    @staticmethod
    def _refuse_pitch(pitch, pitch_range):
        vals = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v]
        if any(float(v) != 0.0 for v in vals(pitch)) or any(float(v) != 1.0 for v in vals(pitch_range)):
            raise ValueError('TTSCubeTwoStage: the Textcoder has no pitch input at inference, so pitch / pitch_range cannot be applied; rate and '
                             '<break> are supported')

    def __call__(self, text, speaker='none', seed=None, rate=1.0, markup=False, pitch=0.0, pitch_range=1.0, loudness=None, peak_db=-1.0):
        """one sentence -> int16 audio at the yaml's sample rate; `seed`: the key of the PreNet's dropout masks (None: drawn from torch's generator).
        rate / markup: as TTSCube.__call__ (durations and breaks only: a pitch argument, or a pitch / range attribute in the markup, raises
        ValueError — this model has no pitch input at inference).  loudness / peak_db: as TTSCube.__call__"""
        self._refuse_pitch(pitch, pitch_range)
        if loudness is not None or _plan_prosody([text], rate, 0.0, 1.0, markup) is not None:
            return self._int16(self._synthesize_batch_device([text], speaker, 32, self._seed(seed), rate=rate, markup=markup, loudness=loudness,
                                                             peak_db=peak_db)[0])
        with torch.no_grad():
            phones = self._phones(text)
            if not phones:                      # (nothing to say: no batch row is made of it)
                return np.zeros(0, dtype=np.int16)
            return self._int16(self._run(self._collate([phones], [speaker]), [self._seed(seed)])[0])

    def synthesize_batch(self, texts, speaker='none', max_batch=32, seed=None, members=None, max_rows=None, rate=1.0, markup=False, pitch=0.0,
                         pitch_range=1.0, loudness=None, peak_db=-1.0):
        """Many sentences -> list of int16 arrays (same order).  Sentences are sorted by phone count and run in padded batches of up to `max_batch`;
        sentence i gets key seed + i, so entry i equals `self(texts[i], seed=seed + i)` whatever the grouping.  members / max_rows: the AR launch
        shape (CubenetTextcoder._ar_decode_batch) — the defaults keep the single call's bits.  rate / markup: a scalar or one value per text;
        segment j of a marked-up text is a row of its own with key `_segment_key(seed + i, j)`.  loudness / peak_db: a scalar or one value per
        text, measured and scaled on the device."""
        self._refuse_pitch(pitch, pitch_range)
        return [self._int16(w) for w in self._synthesize_batch_device(texts, speaker, max_batch, seed, members, max_rows, rate, markup, loudness,
                                                                      peak_db)]

    def _synthesize_batch_device(self, texts, speaker='none', max_batch=32, seed=None, members=None, max_rows=None, rate=1.0, markup=False,
                                 loudness=None, peak_db=-1.0):
        """`synthesize_batch` without the copy to the host: list of 1-D float32 device tensors in [-1, 1], input order, each trimmed to its own samples.
        loudness / peak_db: every entry (a text with <break>s as the joined unit) at its loudness target, one padded batch per `max_batch` texts"""
        texts = list(texts)
        loud = _plan_loudness(loudness, peak_db, len(texts))
        speakers = speaker if isinstance(speaker, (list, tuple)) else [speaker] * len(texts)
        seed = self._seed(seed)
        plan = _plan_prosody(texts, rate, 0.0, 1.0, markup)
        if plan is None:
            units, layout = [(i, 0, t, None) for i, t in enumerate(texts)], [[('unit', i)] for i in range(len(texts))]
        else:
            units, layout = plan
            from .io_utils.prosody import Segment, markup_has_pitch
            if markup_has_pitch([Segment(u[2], u[3]) for u in units]):
                raise ValueError('TTSCubeTwoStage: the markup asks for a pitch or a range, and the Textcoder has no pitch input at inference; '
                                 'rate and <break> are supported')
        utexts = [u[2] for u in units]
        feats = self._text2feat.batch(utexts) if hasattr(self._text2feat, 'batch') else [self._text2feat(t) for t in utexts]
        phones = [list(f['phones']) for f in feats]
        keys = [self._segment_key(seed + u[0], u[1]) if u[1] else seed + u[0] for u in units]
        order = sorted((k for k in range(len(units)) if phones[k]), key=lambda k: len(phones[k]))
        out = [torch.zeros(0, dtype=torch.float32, device=self._device) for _ in units]      # (a sentence without a phone stays empty and takes no row)
        stats = {'launches': 0, 'max_steps': 0}
        with torch.no_grad():
            for s in range(0, len(order), max(1, int(max_batch))):
                ids = order[s:s + max(1, int(max_batch))]
                X = self._collate([phones[k] for k in ids], [speakers[units[k][0]] for k in ids])
                if plan is not None:
                    ds, _, _ = _control_rows([feats[k] for k in ids], [utexts[k] for k in ids], [units[k][3] for k in ids], X['x_char'].shape[1])
                    if (ds != 1.0).any():
                        X['x_dur_scale'] = torch.from_numpy(ds)
                for k, w in zip(ids, self._run(X, [keys[k] for k in ids], members, max_rows)):
                    out[k] = w
                stats = {'launches': stats['launches'] + self.last_stats['launches'], 'max_steps': max(stats['max_steps'], self.last_stats['max_steps'])}
        self.last_stats = stats
        out = out if plan is None else _join_units(layout, out, self._device)
        if loud is not None:
            self._loud_log = (len(texts), {})
            out = _normalize_in_groups(out, loud, self.sample_rate, self._device, max_batch, self._loud_log[1])
        return out

    shard = staticmethod(TTSCube.shard)
    loudness_report = TTSCube.loudness_report
