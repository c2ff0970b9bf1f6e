"""GPU: the two-stage text-to-speech path — ttsc_melar_decode_ragged (per-row Philox keys, forced split), CubenetTextcoder.inference_batch,
api.TTSCubeTwoStage and scripts/synthesize.py.  The contract: a sentence gives the same bits alone and in any batch, at any row, in any AR launch.
Every test uses the small `_Enc` model of tests/test_meldecoder_gpu.py with fill_state_dict weights; the sentences (and the condition on their
duration logits that makes the frame counts immune to fp32 rounding) live in tests/test_twostage_cpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from tests import test_twostage_cpu as TS
from tests.test_meldecoder_gpu import _ar_net, _ar_reference, _check_ar, _decode
from tests.test_oracle_meldecoder import textcoder_pipeline_bound

pytestmark = pytest.mark.gpu

KEY_HIGH = 0x5EED0000ABCD1234


def _key_masks(key, S, P=256):
    """the masks of one row with Philox key `key`: bit (r[unit & 3] & 1) of philox4x32-10(counter (unit >> 2, t, 0, layer), key)  -> [S, 2, 1, P]"""
    from oracle import wavernn_ref as O
    L = O.lib()
    r = (C.c_uint32 * 4)()
    out = np.zeros((S, 2, 1, P), dtype=np.float32)
    for t in range(S):
        for layer in range(2):
            for q in range(P // 4):
                L.wr_philox(q, t, 0, layer, key & 0xffffffff, key >> 32, r)
                out[t, layer, 0, 4 * q:4 * q + 4] = [v & 1 for v in r]
    return torch.from_numpy(out)


def _ragged(net, h, steps, keys=None, members=0, masks=None):
    """ttsc_melar_decode_ragged through _ar_decode, into a NaN-filled buffer -> [B, S, O] on the host"""
    B, S = h.shape[:2]
    out = torch.full((B, S, 80 * net._pframes), float('nan'), device='cuda')
    with torch.no_grad():
        net._ar_decode(h.cuda(), None if masks is None else masks.cuda(), steps=steps, seeds=keys if keys is not None else [0] * B, members=members, out=out)
    return out.cpu().numpy()


# ---- kernel level --------------------------------------------------------------------------------------------------------------------------
# (pframes, B, S, steps, keys, twin rows): two rows share a key — and the overlay states, so that their outputs must agree —, one key has high bits set
_CASES = {
    'pf3': (3, 5, 64, [64, 0, 1, 33, 64], [11, KEY_HIGH, 7, 2 ** 63 - 1, 11], (0, 4)),
    'pf1': (1, 3, 40, [40, 0, 17], [KEY_HIGH, 5, KEY_HIGH], (0, 2)),
}
_REF = {}


def _case(name):
    """inputs, host-rebuilt masks and the float64 loop with its bound: computed once per case, shared by the four split factors, never modified"""
    if name not in _REF:
        pf, B, S, steps, keys, twins = _CASES[name]
        net, sd = _ar_net(pf, 90 + pf)
        rng = np.random.RandomState(B * 1000 + S + pf)
        h = torch.from_numpy(rng.uniform(-1, 1, size=(B, S, 1024)).astype(np.float32))
        h[twins[1]] = h[twins[0]]
        by_key = {k: _key_masks(k, S) for k in set(keys)}
        masks = torch.cat([by_key[k] for k in keys], dim=2)                    # [S, 2, B, 256]
        y64, bound = _ar_reference(sd, h, masks, steps, pf)
        _REF[name] = (net, h, masks, y64, bound)
    return _REF[name]


@pytest.mark.parametrize('G', [1, 2, 4, 8])
@pytest.mark.parametrize('name', ['pf3', 'pf1'])
def test_ragged_ar_launch_gives_every_row_its_solo_bits(name, G, monkeypatch):
    """ttsc_melar_decode_ragged at a forced split G (melar_kernel / melar_split_kernel) into a NaN-filled buffer:
    (1) row b is bit-identical to ttsc_melar_decode(B = 1, seed = keys[b], steps = [steps[b]]) at TTSC_MELAR_SPLIT = G; permuting the rows permutes
    the outputs and nothing else; rows past steps[b] are exactly zero;
    (2) Philox mode is bit-identical to the same launch fed the masks rebuilt on the host with counter (unit >> 2, t, 0, layer) and key keys[b]
    (every split member draws the same masks); two rows with equal keys and equal overlay states agree on their common steps;
    (3) every valid step is within _ar_reference's bound (4 x the oracle's fp32-vs-float64 deviation + 1e-6) of the float64 loop;
    (4) no hand-off timed out."""
    from ttscube_amd import _lib
    pf, B, S, steps, keys, twins = _CASES[name]
    net, h, masks, y64, bound = _case(name)
    y = _ragged(net, h, steps, keys, G)
    assert _lib.lib().ttsc_melar_split_status() == 0, 'G=%d: a split hand-off timed out' % G
    _check_ar(y, y64, bound, steps, '%s G=%d' % (name, G))                      # (3), and exact zeros past steps[b]
    monkeypatch.setenv('TTSC_MELAR_SPLIT', str(G))
    for b in range(B):
        solo = _decode(net, h[b:b + 1], None, [steps[b]], seed=keys[b])
        assert np.array_equal(solo[0], y[b]), 'G=%d: row %d != ttsc_melar_decode(B=1, seed=keys[%d])' % (G, b, b)
    monkeypatch.delenv('TTSC_MELAR_SPLIT')
    perm = list(np.random.RandomState(B + G).permutation(B))
    yp = _ragged(net, h[perm], [steps[i] for i in perm], [keys[i] for i in perm], G)
    assert np.array_equal(yp, y[perm]), 'G=%d: permuting the rows changed a row' % G
    ym = _ragged(net, h, steps, None, G, masks=masks)
    assert np.array_equal(ym, y), 'G=%d: in-kernel Philox masks != host-rebuilt masks (first step %s)' % (G, np.argwhere(ym != y)[:1, 1])
    n = min(steps[twins[0]], steps[twins[1]])
    assert n > 0 and np.array_equal(y[twins[0], :n], y[twins[1], :n])
    assert _lib.lib().ttsc_melar_split_status() == 0, 'G=%d: a split hand-off timed out' % G


def test_ragged_ar_default_split_is_the_dispatchers():
    """members = 0 takes the rule of ttsc_melar_decode for this B (ttsc_melar_members) — the bits of the forced launch at that factor"""
    pf, B, S, steps, keys, _ = _CASES['pf1']
    net, h, masks, y64, bound = _case('pf1')
    G = net.ar_members(B)
    assert G in (1, 2, 4, 8) and G * B <= torch.cuda.get_device_properties(0).multi_processor_count
    assert np.array_equal(_ragged(net, h, steps, keys, 0), _ragged(net, h, steps, keys, G))


def test_ragged_ar_refuses_a_split_that_cannot_be_co_resident():
    """B = CUs // 8 + 1 rows at members = 8: 8 * B workgroups that spin on each other exceed the CUs — an argument error, nothing is launched
    (the buffer is still all NaN); so are a members value that is no split factor and missing keys"""
    from ttscube_amd import _lib
    net, _ = _ar_net(3, 93)
    B = torch.cuda.get_device_properties(0).multi_processor_count // 8 + 1
    S = 2
    h = torch.zeros((B, S, 1024), device='cuda')
    out = torch.full((B, S, 240), float('nan'), device='cuda')
    with torch.no_grad():
        for members in (8, 3):
            with pytest.raises(_lib.TTSCError):
                net._ar_decode(h, None, steps=[S] * B, seeds=list(range(B)), members=members, out=out)
        xg1 = net._ar_xg1(h)
        st = torch.full((B,), S, dtype=torch.int32, device='cuda')
        P = _lib.dev_ptr
        rc = _lib.lib().ttsc_melar_decode_ragged(net._melar_handle(), P(xg1), B, S, None, None, P(st), 1, P(out), _lib.current_stream())   # no keys, no masks
        assert rc != 0
        rc = _lib.lib().ttsc_melar_decode_ragged(net._melar_handle(), P(xg1), B, S, None, P(st), None, 1, P(out), _lib.current_stream())    # no steps
        assert rc != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert _lib.lib().ttsc_melar_split_status() == 0


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
_NET = {}


def _net():
    if 'n' not in _NET:
        _NET['n'] = _ar_net(TS.PFRAMES, TS.NET_SEED)
        from tests.test_meldecoder_gpu import _Enc
        assert (len(_Enc.phon2int), len(_Enc.speaker2int), _Enc.max_pitch, _Enc.max_duration) == (
            len(TS.Enc.phon2int), len(TS.Enc.speaker2int), TS.Enc.max_pitch, TS.Enc.max_duration)
    return _NET['n']


def _oracle_row(sd, sent, key, S):
    """float64 oracle pipeline of one sentence with the masks of `key` -> (AR output [S, O] float64, per-step bound [S], fp32 oracle post-net mel)"""
    X = TS.solo_batch(sent)
    mk = _key_masks(key, S)
    bound = textcoder_pipeline_bound(sd, X, mk, TS.PFRAMES, S)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        h64, _ = M.textcoder_overlay(sd64, X['x_char'], X['x_speaker'], TS.PFRAMES)
        y64 = M.textcoder_ar_decode(sd64, h64, mk.double(), pframes=TS.PFRAMES).reshape(S, -1).numpy()
        mel32, _ = M.textcoder_inference(sd, X['x_char'], X['x_speaker'], mk, pframes=TS.PFRAMES)
    return y64, bound, mel32


def _within_bound(mel_ar_row, y64, bound, what):
    S = y64.shape[0]
    err = np.abs(mel_ar_row[:S * TS.PFRAMES].double().cpu().numpy().reshape(S, -1) - y64).max(axis=1)
    bad = np.flatnonzero(err > bound)
    assert not len(bad), '%s: AR step %d error %.3g > bound %.3g' % (what, bad[0], err[bad[0]], bound[bad[0]])


def test_inference_batch_equals_the_solo_calls():
    """five sentences of 13, 6, 9, 1 and 11 phones (one ends in an out-of-vocabulary phone): inference_batch(X, seeds) gives every row the frame
    count and the mel of inference(X_b, seed = seeds[b]) bit for bit — also in three AR launches (max_rows = 2) and with the list permuted —, zeros
    past its frames; each row's AR output within textcoder_pipeline_bound of the float64 oracle pipeline run with the host-rebuilt masks, its
    post-net mel within the 1e-4 RMS gate of the fp32 oracle."""
    net, sd = _net()
    sents = TS.sentences_five()
    ks = [5, KEY_HIGH, 77, 5, 123456789]
    with torch.no_grad():
        solo = [net.inference(TS.solo_batch(s), seed=k) for s, k in zip(sents, ks)]
        mel, frames, st = net.inference_batch(TS.padded_batch(sents), seeds=ks, return_stats=True)
        assert st['launches'] == 1 and st['rows'] == list(range(5))
        for b in range(5):
            F = solo[b].shape[1]
            assert F > 0 and frames[b] == F
            assert torch.equal(mel[b, :F], solo[b][0]), 'row %d of the batch != its solo call (max |d| %.3g)' % (b, float((mel[b, :F] - solo[b][0]).abs().max()))
            assert not bool(mel[b, F:].any())
        mel2, frames2, st2 = net.inference_batch(TS.padded_batch(sents), seeds=ks, max_rows=2, return_stats=True)
        assert st2['launches'] == 3 and frames2 == frames and torch.equal(mel2, mel)
        perm = [3, 0, 4, 2, 1]
        melp, framesp = net.inference_batch(TS.padded_batch([sents[i] for i in perm]), seeds=[ks[i] for i in perm])
        assert framesp == [frames[i] for i in perm] and torch.equal(melp, mel[perm])
        # the channel-major hand-back is the same mel
        melc, _ = net.inference_batch(TS.padded_batch(sents), seeds=ks, channel_major=True)
        assert torch.equal(melc.permute(0, 2, 1), mel)
    for b, (s, k) in enumerate(zip(sents, ks)):
        S = frames[b] // TS.PFRAMES
        y64, bound, mel32 = _oracle_row(sd, s, k, S)
        _within_bound(st['mel_ar'][b], y64, bound, 'row %d' % b)
        assert mel32.shape[1] == frames[b]
        assert float((mel[b, :frames[b]].cpu() - mel32[0]).pow(2).mean().sqrt()) < 1e-4


def test_inference_batch_of_forty_sentences_in_two_ar_launches():
    """forty sentences of 3 to 8 phones — more rows than one AR launch holds at the solo split: frame counts equal the solo calls, every row within
    the float64 bound at the AR output, and the AR STAGE bit-identical to the solo decode when both are fed the same overlay states (the text-side
    LSTM dispatcher may pick another split for forty rows than for one: summation order)."""
    from ttscube_amd import _lib
    from ttscube_amd.networks.modules import _expand_rows, align_durations
    net, sd = _net()
    sents = TS.sentences_forty()
    ks = [1000 + 7 * i for i in range(40)]
    X = TS.padded_batch(sents)
    max_rows = torch.cuda.get_device_properties(0).multi_processor_count // net.ar_members(1)
    with torch.no_grad():
        mel, frames, st = net.inference_batch(X, seeds=ks, return_stats=True)
        assert st['launches'] == -(-40 // max_rows) and st['launches'] >= 2
        assert frames == [int(net.inference(TS.solo_batch(s), seed=k).shape[1]) for s, k in zip(sents, ks)]
        # the AR stage alone, on the batch path's own overlay states
        lengths = _lib.DevLengths([len(s[0]) for s in sents], device='cuda')
        h, out_dur = net._text_stack(X['x_char'].cuda(), X['x_speaker'].cuda(), lengths)
        h, steps = _expand_rows(h, align_durations(out_dur, lengths), stride=TS.PFRAMES)
        assert [n * TS.PFRAMES for n in steps] == frames
        h = net._lstm('_rnn_overlay')(h, lengths=_lib.DevLengths(steps, device='cuda'))
        y, n_launch = net._ar_decode_batch(h, steps, seeds=ks)
        assert n_launch == st['launches']
        for b in range(40):
            solo = net._ar_decode(h[b:b + 1, :steps[b]].contiguous(), seed=ks[b])
            assert torch.equal(y[b, :frames[b]], solo[0]), 'AR stage: row %d != its solo decode' % b
            assert not bool(y[b, frames[b]:].any())
    for b, (s, k) in enumerate(zip(sents, ks)):
        y64, bound, _ = _oracle_row(sd, s, k, frames[b] // TS.PFRAMES)
        _within_bound(st['mel_ar'][b], y64, bound, 'row %d' % b)


def _one_frame_per_phone(module):
    """push the duration head to `one frame per phone` (bias of class 1 far above the logits): a sentence of n phones then has n // pframes AR
    steps — none at all for one or two phones — whatever the arithmetic does"""
    with torch.no_grad():
        module._dur_output.linear_layer.bias[1] += 1000.0


def test_inference_batch_rows_without_a_frame_are_launched_nowhere():
    """a copy of the small model whose every phone lasts one frame: the sentences of 1 and 2 phones have no AR step — their mel is empty, as
    `inference` returns [1, 0, 80], and their neighbours keep the bits of their solo calls; a batch of such sentences alone is empty"""
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    _, sd = _net()
    net = CubenetTextcoder(TS.Enc(), pframes=TS.PFRAMES)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    _one_frame_per_phone(net)
    sents = TS._sentences([13, 2, 9, 1, 11], 5)
    ks = [3, 4, 5, 6, 7]
    with torch.no_grad():
        mel, frames, st = net.inference_batch(TS.padded_batch(sents), seeds=ks, return_stats=True)
        assert frames == [12, 0, 9, 0, 9] and st['rows'] == [0, 2, 4] and st['launches'] == 1 and mel.shape == (5, 12, 80)
        for b, (s, k) in enumerate(zip(sents, ks)):
            solo = net.inference(TS.solo_batch(s), seed=k)
            assert solo.shape == (1, frames[b], 80) and torch.equal(mel[b, :frames[b]], solo[0]) and not bool(mel[b, frames[b]:].any())
        mel0, frames0 = net.inference_batch(TS.padded_batch([sents[1], sents[3]]), seeds=[1, 2])
        assert frames0 == [0, 0] and mel0.shape == (2, 0, 80)


# ---- public interface ----------------------------------------------------------------------------------------------------------------------
def _model_dir(tmp_path):
    """a model directory as scripts/train_textcoder.py and scripts/train_hifigan.py leave it: <base>.yaml / .encodings / .best, vocoder checkpoint
    with config.json beside it"""
    import yaml
    from oracle import hifigan_ref as R
    from ttscube_amd.io_utils.io_textcoder import TextcoderEncodings
    _, sd = _net()
    base = str(tmp_path / 'textcoder')
    yaml.dump({'sample_rate': 24000, 'pframes': TS.PFRAMES, 'hop_size': 240}, open(base + '.yaml', 'w'))
    enc = TextcoderEncodings()
    enc.phon2int, enc.speaker2int, enc.max_pitch, enc.max_duration = dict(TS.Enc.phon2int), dict(TS.Enc.speaker2int), TS.Enc.max_pitch, TS.Enc.max_duration
    enc.save(base + '.encodings')
    torch.save(sd, base + '.best')
    vdir = tmp_path / 'vocoder'
    vdir.mkdir()
    torch.save({'generator': R.synthetic_state_dict(dict(R.CONFIG_V1), seed=55)}, str(vdir / 'g_00000001'))
    (vdir / 'config.json').write_text(json.dumps(dict(R.CONFIG_V1)))
    return base, str(vdir / 'g_00000001')


def test_two_stage_api_batch_equals_single_calls(tmp_path):
    """TTSCubeTwoStage on a model directory written here, phone-string front end: synthesize_batch(texts, seed = s, max_batch = 3)[i] is
    tts(texts[i], seed = s + i), for the list permuted too; a sentence without a phone gives an empty array and leaves its neighbours alone; the wav
    synthesize_devset writes for an item with the host-rebuilt masks of key k holds the samples of tts(text, seed = k); GriffinLimVocoder as `vocoder` runs."""
    import scipy.io.wavfile
    from ttscube_amd.api import TTSCubeTwoStage
    from ttscube_amd.io_utils.runtime import synthesize_devset
    from ttscube_amd.io_utils.vocoder import GriffinLimVocoder
    base, vck = _model_dir(tmp_path)
    tts = TTSCubeTwoStage(base, vck)
    assert tts.sample_rate == 24000
    sents = TS.sentences_five()
    texts = [TS.phone_text(s) for s in sents]
    spk = [str(s[1] - 1) for s in sents]
    assert 'zz' in texts[TS.OOV_ROW]
    s0 = 4242
    single = [tts(t, speaker=p, seed=s0 + i) for i, (t, p) in enumerate(zip(texts, spk))]
    got = tts.synthesize_batch(texts, speaker=spk, seed=s0, max_batch=3)
    for i in range(5):
        assert got[i].dtype == np.int16 and len(got[i]) > 0 and np.array_equal(got[i], single[i]), 'sentence %d' % i
    perm = [2, 4, 0, 3, 1]
    gotp = tts.synthesize_batch([texts[i] for i in perm], speaker=[spk[i] for i in perm], seed=s0, max_batch=3)
    for j, i in enumerate(perm):
        assert np.array_equal(gotp[j], tts(texts[i], speaker=spk[i], seed=s0 + j)), 'permuted list, position %d' % j
    # a sentence without a phone: empty, and the others keep their keys (their position in the list) and their bits
    gap = tts.synthesize_batch([texts[0], '', texts[2]], speaker=[spk[0], spk[0], spk[2]], seed=s0, max_batch=3)
    assert len(gap[1]) == 0 and gap[1].dtype == np.int16 and np.array_equal(gap[0], single[0]) and np.array_equal(gap[2], single[2])
    assert len(tts('', seed=1)) == 0
    # a sentence WITH a phone but without a frame (every phone one frame long, pframes = 3): empty too, between two untouched neighbours
    short = TTSCubeTwoStage(base, vck)
    _one_frame_per_phone(short._model)
    trio = [texts[0], texts[3], texts[2]]
    got3 = short.synthesize_batch(trio, speaker=[spk[0], spk[3], spk[2]], seed=s0, max_batch=3)
    assert len(got3[1]) == 0 and len(short(texts[3], speaker=spk[3], seed=s0 + 1)) == 0
    for j in (0, 2):
        assert len(got3[j]) == 240 * (len(sents[[0, 3, 2][j]][0]) // 3 * 3) + 64
        assert np.array_equal(got3[j], short(trio[j], speaker=[spk[0], spk[3], spk[2]][j], seed=s0 + j))
    # synthesize_devset with the masks of key k == tts(text, seed = k)
    k, b = KEY_HIGH, 1
    frames = len(tts(texts[b], speaker=spk[b], seed=k)) // 240                     # (the generator emits 240 F + 64 samples)
    masks = _key_masks(k, frames // TS.PFRAMES)

    class OneItem:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {'meta': {'id': 'utt0'}}

    class Collate:
        def collate_fn(self, exs):
            return TS.solo_batch(sents[b])

    out_dir = str(tmp_path / 'wavs')
    assert synthesize_devset(tts._model, Collate(), OneItem(), tts._vocoder, output_path=out_dir, forced_synthesis=False, dropout_masks=[masks]) == 1
    rate, wav = scipy.io.wavfile.read(os.path.join(out_dir, 'utt0.wav'))
    assert rate == 24000 and wav.dtype == np.int16 and np.array_equal(wav, tts(texts[b], speaker=spk[b], seed=k))
    # a vocoder without `frames=`: one call per sentence on the trimmed mel
    gl = TTSCubeTwoStage(base, GriffinLimVocoder(n_iter=4))
    a = gl.synthesize_batch(texts[:2], speaker=spk[:2], seed=s0, max_batch=2)
    for i in range(2):
        assert a[i].dtype == np.int16 and len(a[i]) == 240 * ((len(single[i]) - 64) // 240 - 1) and np.isfinite(a[i].astype(np.float64)).all()
        assert np.array_equal(a[i], gl(texts[i], speaker=spk[i], seed=s0 + i))


def test_synthesize_script_writes_the_same_bytes_at_every_batch(tmp_path):
    import importlib.util
    from tests.conftest import ROOT
    spec = importlib.util.spec_from_file_location('_synthesize_script_gpu', os.path.join(ROOT, 'scripts', 'synthesize.py'))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    base, vck = _model_dir(tmp_path)
    (tmp_path / 'in.txt').write_text('\n'.join(TS.phone_text(s) for s in TS.sentences_script()) + '\n')
    blobs = {}
    for batch in (1, 4):
        out = tmp_path / ('out%d' % batch)
        assert S.main(['--textcoder', base, '--vocoder', vck, '--input', str(tmp_path / 'in.txt'), '--output-folder', str(out), '--speaker', TS.SCRIPT_SPEAKER,
                       '--batch', str(batch), '--seed', '9']) == 0
        assert sorted(os.listdir(str(out))) == ['%05d.wav' % i for i in range(1, 6)]
        blobs[batch] = [open(str(out / ('%05d.wav' % i)), 'rb').read() for i in range(1, 6)]
    assert blobs[1] == blobs[4] and all(len(b) > 44 for b in blobs[1])
