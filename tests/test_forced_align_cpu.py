"""CPU: the forced aligner without a kernel — build_lattice on hand-written cases, the TextGrid writer through the reader and the importer, the
float64 restatement (tests/forced_align_reference.py) against enumeration and on the generated corpus (tests/forced_align_signals.py), and
scripts/align_corpus.py's argument surface and files around an injected host aligner."""
import functools
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from tests import forced_align_reference as R
from tests import forced_align_signals as S
from tests.conftest import ROOT

N_SUB = 3
PHONES = ['sil'] + S.PHONES
PID = {p: i for i, p in enumerate(PHONES)}
# The largest boundary error of the float64 restatement on the generated corpus (seed 1234, 4 iterations), measured by
# test_float64_restatement_on_the_generated_corpus below, which prints it and fails if it is ever larger.  tests/test_forced_align_gpu.py allows
# the device this value plus one frame (10 ms): the float32 path can move a boundary by a frame at a near-tie.  DESIGN 9j quotes it.
REF_MAX_BOUNDARY_ERROR_S = 0.0320


def _script():
    spec = importlib.util.spec_from_file_location('align_corpus_script', os.path.join(ROOT, 'scripts', 'align_corpus.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lattice_of(item):
    return R.build_lattice([[PID[p] for p in S.LEXICON[w.upper()]] for w in item['words']], N_SUB)


def boundary_report(items, results):
    """items: the generated corpus, results: (word intervals, phone intervals) or None per item -> (infeasible ids, ids whose silences are not as
    generated, the signed errors of every inner boundary of the others in seconds, the number of boundaries of the truth)"""
    infeasible, wrong, errs, total = [], [], [], 0
    for it, res in zip(items, results):
        total += len(it['units']) - 1
        if res is None:
            infeasible.append(it['id'])
            continue
        ph = res[1]
        if [p[0] for p in ph] != [u[0] for u in it['units']]:
            wrong.append(it['id'])
            continue
        errs += [p[1] - u[2] / S.SAMPLE_RATE for p, u in zip(ph[1:], it['units'][1:])]
        assert ph[0][1] == 0.0 and ph[-1][2] == len(it['audio']) / S.SAMPLE_RATE
    return infeasible, wrong, errs, total


@functools.lru_cache(maxsize=None)
def corpus64():
    """the generated corpus, its float64 features and lattices and the float64 fit (computed once, shared, never modified)"""
    items = S.corpus()
    feats = [R.features(R.logmel10(it['audio'])) for it in items]
    lats = [lattice_of(it) for it in items]
    steps = R.fit(feats, lats, len(PHONES) * N_SUB, 4, dt=np.float64)
    return items, feats, lats, steps


# ---- build_lattice -----------------------------------------------------------------------------------------------------------------------------------

def test_build_lattice_on_hand_written_cases():
    from ttscube_amd.io_utils import forced_align as FA
    one = FA.build_lattice([[1, 2]], 2)                           # sil a b sil
    assert one['state'].tolist() == [0, 1, 2, 3, 4, 5, 0, 1] and one['skip'].tolist() == [-1] * 8
    assert one['start'].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and one['final'].tolist() == [0, 0, 0, 0, 0, 1, 0, 1]
    assert one['word'].tolist() == [-1, -1, 0, 0, 0, 0, -1, -1] and one['unit'].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    punct = FA.build_lattice([[1], [], [2]], 2)                   # the token without phones contributes no positions, and no silence of its own
    two = FA.build_lattice([[1], [2]], 2)                         # sil a sil b sil
    assert two['state'].tolist() == [0, 1, 2, 3, 0, 1, 4, 5, 0, 1]
    assert two['skip'].tolist() == [-1, -1, -1, -1, -1, -1, 3, -1, -1, -1]      # from the first position behind the inner silence to the last before it
    assert two['start'].tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and two['final'].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1]
    for k in ('state', 'skip', 'start', 'final', 'unit', 'phone'):
        assert np.array_equal(punct[k], two[k]), k
    assert punct['word'].tolist() == [-1, -1, 0, 0, -1, -1, 2, 2, -1, -1]
    assert one['state'].dtype == np.int32 and one['skip'].dtype == np.int32 and one['start'].dtype == np.uint8 and one['final'].dtype == np.uint8
    assert len(FA.build_lattice([[], []], 3)['state']) == 0
    with pytest.raises(ValueError):
        FA.build_lattice([[0]], 3)
    for prons in ([[1, 2]], [[1], [], [2]], [[3, 1], [2], [1, 1, 2]]):
        a, b = FA.build_lattice(prons, 3), R.build_lattice(prons, 3)
        assert all(np.array_equal(a[k], b[k]) for k in b)
    packed = FA.pack_lattices([one, two])
    assert packed['npos'].tolist() == [8, 10] and packed['state'].shape == (2, 10) and packed['state'][0, 8:].tolist() == [-1, -1]


def test_flat_alignment_is_uniform_over_all_positions():
    from ttscube_amd.io_utils import forced_align as FA
    al, ok = FA.flat_alignment([6, 3, 0, 8], [3, 4, 2, 0], 8)
    assert ok.tolist() == [1, 0, 0, 0]
    assert al[0].tolist() == [0, 0, 1, 1, 2, 2, -1, -1] and np.all(al[1:] == -1)
    assert np.array_equal(R.flat_alignment(6, 3), al[0, :6]) and R.flat_alignment(3, 4) is None


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------------

def test_restatement_is_optimal_against_enumeration():
    rng = np.random.default_rng(1234)
    M, D = 9, 3
    mean, var = rng.standard_normal((M, D)), rng.uniform(0.5, 2.0, (M, D))
    km = R.kernel_model(mean, var, np.float64)
    for prons, T in (([[1]], 3), ([[1]], 5), ([[1], [2]], 4), ([[1], [2]], 7), ([[2, 1], [1]], 8)):
        lat = R.build_lattice(prons, 1)
        x = rng.standard_normal((T, D))
        al, score, ok = R.viterbi(x, lat, *km)
        opt = R.brute_force(x, lat, *km)
        assert ok == (opt is not None), (prons, T)
        if ok:
            assert abs(float(score) - opt) <= 1e-12 * abs(opt) and R.path_ok(al, lat)
            assert abs(R.path_score64(x, al, lat, *km) - opt) <= 1e-12 * abs(opt)
    lat = R.build_lattice([[1], [2]], 2)                          # 10 positions, 4 of them mandatory
    assert R.viterbi(rng.standard_normal((3, D)), lat, *km)[2] == 0 and R.viterbi(rng.standard_normal((4, D)), lat, *km)[2] == 1


def test_float64_restatement_on_the_generated_corpus():
    items, feats, lats, steps = corpus64()
    assert 6 <= len(items) <= 10 and all(0.9 <= len(it['audio']) / S.SAMPLE_RATE <= 2.2 for it in items)
    gaps = [p for it in items for p in it['pause'][1:-1]]
    assert any(gaps) and not all(gaps)                            # silences between some words but not others
    assert all(all(ok) for ok in (st['oks'] for st in steps))     # every utterance is feasible, at the flat start and in every iteration
    scores = [st['score'] for st in steps[1:]]
    assert all(b > a for a, b in zip(scores, scores[1:])), scores
    km = R.kernel_model(steps[-1]['mean'], steps[-1]['var'], np.float64)
    results = []
    for it, x, lat in zip(items, feats, lats):
        al, _, ok = R.viterbi(x, lat, *km)
        results.append(R.intervals(al, lat, it['words'], PHONES, S.HOP, S.SAMPLE_RATE, len(it['audio']) / S.SAMPLE_RATE) if ok else None)
    infeasible, wrong, errs, total = boundary_report(items, results)
    assert not infeasible and not wrong, (infeasible, wrong)      # every silence is found present or absent as generated
    assert len(errs) == total                                     # no boundary is left out of the score
    worst = float(np.max(np.abs(errs)))
    print('float64 restatement: %d boundaries, largest error %.4f ms, mean signed error %.4f ms' % (total, 1e3 * worst, 1e3 * float(np.mean(errs))))
    assert worst <= REF_MAX_BOUNDARY_ERROR_S + 1e-9
    assert worst >= REF_MAX_BOUNDARY_ERROR_S - 0.0005             # the constant is the measured value, not a loose cap


# ---- TextGrid writer ---------------------------------------------------------------------------------------------------------------------------------

def test_textgrid_writer_round_trips_and_the_importer_reads_it(tmp_path):
    from ttscube_amd.io_utils import forced_align as FA
    from ttscube_amd.io_utils.corpus_import import read_item
    from ttscube_amd.io_utils.textgrid import TextGrid
    items, feats, lats, steps = corpus64()
    it, lat = items[0], lats[0]
    al = steps[-1]['aligns'][0]
    dur = len(it['audio']) / S.SAMPLE_RATE
    words, phones = FA.intervals(al, lat, it['words'], PHONES, S.HOP, S.SAMPLE_RATE, dur)
    assert (words, phones) == R.intervals(al, lat, it['words'], PHONES, S.HOP, S.SAMPLE_RATE, dur)
    text = it['text'] + ', "quoted" 1.5 [2]'
    tg = FA.to_textgrid({'duration': dur, 'words': words, 'phones': phones}, text)
    back = TextGrid.fromString(tg.toString())
    assert [t.name for t in back] == ['words', 'phones', 'text'] and back.minTime == 0.0 and back.maxTime == dur
    for tier, want in ((back[0], words), (back[1], phones), (back[2], [(text, 0.0, dur)])):
        assert [(iv.mark, iv.minTime, iv.maxTime) for iv in tier] == want            # equal floats, not close ones
        assert tier[0].minTime == 0.0 and tier[-1].maxTime == dur
        assert all(a.maxTime == b.minTime for a, b in zip(tier.intervals, tier.intervals[1:]))
    assert '' in [iv.mark for iv in back[1]]                      # silences are intervals with empty marks
    path = tmp_path / 'utt.TextGrid'
    FA.to_textgrid({'duration': dur, 'words': words, 'phones': phones}, it['text']).write(str(path))
    assert open(path, 'rb').read().decode('utf-8').startswith('File type = "ooTextFile"')
    item = read_item(str(tmp_path / 'utt'), 'spk')
    spoken = [p for p in item['phones'] if p.strip()]
    assert spoken == [p for w in it['words'] for p in S.LEXICON[w.upper()]]
    assert [w for w in item['words'] if w.isalpha()] == it['words'] and len(item['frame2phon']) == int(dur * 100)


# ---- scripts/align_corpus.py -------------------------------------------------------------------------------------------------------------------------

def test_script_argument_surface():
    A = _script()
    a = A.parse_args(['--input-folder', 'in', '--lexicon', 'lex'])
    assert (a.input_folder, a.lexicon, a.g2p, a.output_folder, a.model_out, a.model_in, a.iterations, a.batch, a.device, a.gpu_resample) == \
        ('in', 'lex', None, None, None, None, 4, 32, 'cuda:0', False)
    a = A.parse_args(['--input-folder', 'in', '--lexicon', 'lex', '--g2p', 'g', '--output-folder', 'o', '--model-out', 'm.npz', '--iterations', '2',
                      '--batch', '8', '--device', 'cuda:1', '--gpu-resample'])
    assert (a.g2p, a.output_folder, a.model_out, a.iterations, a.batch, a.device, a.gpu_resample) == ('g', 'o', 'm.npz', 2, 8, 'cuda:1', True)
    assert A.parse_args(['--input-folder', 'in', '--lexicon', 'lex', '--model-in', 'm.npz']).model_in == 'm.npz'
    for bad in (['--lexicon', 'lex'], ['--input-folder', 'in'], ['--input-folder', 'in', '--lexicon', 'lex', '--batch', '0'],
                ['--input-folder', 'in', '--lexicon', 'lex', '--iterations', '-1'],
                ['--input-folder', 'in', '--lexicon', 'lex', '--model-in', 'a', '--model-out', 'b']):
        with pytest.raises(SystemExit):
            A.parse_args(bad)


def test_script_lexicon_and_pronunciations(tmp_path):
    from ttscube_amd.io_utils.io_text import SimpleTokenizer
    A = _script()
    lex = tmp_path / 'lex'
    lex.write_text('asa\tAA S AA\nASA\tAA\nnot a lexicon line\nSHE\tSH  EH\n')
    d = A.read_lexicon(str(lex))
    assert d == {'ASA': ['AA', 'S', 'AA'], 'SHE': ['SH', 'EH']}    # the first entry of a word stands; lookup is upper-cased
    words, prons, unknown = A.pronounce('Asa, she who', d, SimpleTokenizer())
    assert words == ['Asa', ',', ' ', 'she', ' ', 'who'] and prons == [['AA', 'S', 'AA'], [], [], ['SH', 'EH'], [], []] and unknown == ['who']


def host_aligner(phones, device='cpu', model_in=None):
    """a ForcedAligner whose features, search and statistics are the float64 / float32 restatements on the host"""
    from ttscube_amd.io_utils import forced_align as FA

    def features(wavs):
        fs = [R.features(R.logmel10(w)).astype(np.float32) for w in wavs]
        F = max(f.shape[0] for f in fs)
        out = np.zeros((len(fs), F, 26), np.float32)
        for b, f in enumerate(fs):
            out[b, :f.shape[0]] = f
        return torch.from_numpy(out), torch.tensor([f.shape[0] for f in fs], dtype=torch.int32)

    def rows(lat):
        npos = lat['npos'].numpy()
        return [{k: lat[k][b, :npos[b]].numpy() for k in ('state', 'skip', 'start', 'final')} for b in range(len(npos))]

    def search(feat, nframes, lat, mean, ivar, cst):
        B, Tmax = feat.shape[:2]
        out = {'align': torch.full((B, Tmax), -1, dtype=torch.int32), 'score': torch.zeros(B), 'ok': torch.zeros(B, dtype=torch.int32)}
        for b, l in enumerate(rows(lat)):
            T = int(nframes[b])
            al, sc, ok = R.viterbi(feat[b, :T].numpy(), l, mean.numpy(), ivar.numpy(), cst.numpy(), np.float32)
            if ok:
                out['align'][b, :T], out['score'][b], out['ok'][b] = torch.from_numpy(al), float(sc), 1
        return out

    def statistics(feat, nframes, align, ok, lat, count, total, sumsq):
        n = nframes.numpy()
        c, s, q = count.numpy(), total.numpy(), sumsq.numpy()     # (views: the tables are updated in place)
        R.accumulate([feat[b, :n[b]].numpy() for b in range(len(n))], [align[b, :n[b]].numpy() for b in range(len(n))], ok.numpy().tolist(), rows(lat),
                     c, s, q)

    if model_in:
        return FA.ForcedAligner.load(model_in, device='cpu', features=features, search=search, statistics=statistics)
    return FA.ForcedAligner(phones, n_sub=N_SUB, device='cpu', features=features, search=search, statistics=statistics)


def test_script_writes_textgrids_with_an_injected_host_aligner(tmp_path):
    """the whole script around host stand-ins for the kernels' callers: four files of the corpus, one more with a word the lexicon lacks, one too
    short for its transcript; then --model-in reproduces the TextGrids without training"""
    from ttscube_amd.io_utils.audio import save_wav
    from ttscube_amd.io_utils.corpus_import import read_item
    from ttscube_amd.io_utils.textgrid import TextGrid
    A = _script()
    items = S.corpus()[:4]
    src, dst, dst2 = tmp_path / 'in', tmp_path / 'out', tmp_path / 'out2'
    src.mkdir()
    (tmp_path / 'lex').write_text(S.lexicon_text())
    for k, it in enumerate(items):
        save_wav(str(src / (it['id'] + '.wav')), it['audio'], S.SAMPLE_RATE)
        (src / (it['id'] + ('.lab' if k == 1 else '.txt'))).write_text(it['text'] + '\n')
    save_wav(str(src / 'zz_unknown.wav'), items[0]['audio'], S.SAMPLE_RATE)
    (src / 'zz_unknown.txt').write_text('asa xyzzy\n')
    save_wav(str(src / 'zz_short.wav'), items[0]['audio'][:2400], S.SAMPLE_RATE)          # 10 frames for 33 or more positions
    (src / 'zz_short.txt').write_text(items[0]['text'] + '\n')
    save_wav(str(src / 'zz_no_text.wav'), items[0]['audio'], S.SAMPLE_RATE)
    out = io.StringIO()
    model = tmp_path / 'aligner.npz'
    assert A.main(['--input-folder', str(src), '--lexicon', str(tmp_path / 'lex'), '--output-folder', str(dst), '--model-out', str(model),
                   '--batch', '3', '--device', 'cpu'], make_aligner=host_aligner, out=out) == 0
    log = out.getvalue()
    assert 'Found 5 files to align, 1 skipped' in log and 'Skipped zz_unknown: unknown words: xyzzy' in log and 'Skipped zz_short: infeasible' in log
    assert 'Wrote 4 TextGrid files' in log and log.count('iteration ') == 4
    assert sorted(os.listdir(dst)) == sorted([it['id'] + e for it in items for e in ('.TextGrid', '.wav')])
    assert model.exists()
    for it in items:
        tg = TextGrid.fromFile(str(dst / (it['id'] + '.TextGrid')))
        assert tg[2][0].mark == it['text'] and [iv.mark for iv in tg[0] if iv.mark] == it['words']
        assert [iv.mark for iv in tg[1] if iv.mark] == [p for w in it['words'] for p in S.LEXICON[w.upper()]]
        rec = read_item(str(dst / it['id']), 'spk')
        assert [w for w in rec['words'] if w.isalpha()] == it['words']
    out2 = io.StringIO()
    assert A.main(['--input-folder', str(src), '--lexicon', str(tmp_path / 'lex'), '--output-folder', str(dst2), '--model-in', str(model),
                   '--device', 'cpu'], make_aligner=host_aligner, out=out2) == 0
    assert 'iteration' not in out2.getvalue()
    for it in items:
        assert open(dst / (it['id'] + '.TextGrid')).read() == open(dst2 / (it['id'] + '.TextGrid')).read()
