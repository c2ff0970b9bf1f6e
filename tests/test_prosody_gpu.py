"""GPU: prosody control — the two controlled kernels of csrc/prosody.hip against the numpy restatement (tests/prosody_reference.py),
exactly; their identity with the uncontrolled kernels, bit for bit; and the controls through Languasito2 / Cubegan / TTSCube / TTSCubeTwoStage:
rate, pitch, pitch range, markup with breaks, the ragged pipelined batch path."""
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import hifigan_ref as R
from oracle import meldecoder_ref as M
from tests import prosody_reference as PR

pytestmark = pytest.mark.gpu

CANARY = -7


def _ptr(t):
    from ttscube_amd import _lib
    return _lib.dev_ptr(t) if t is not None else None


# ---- ttsc_align_durations_ctl ---------------------------------------------------------------------------------------------------------------
def _logits(B, N, D, seed):
    """random duration logits; about a fifth of the phones get d = 0"""
    rng = np.random.RandomState(seed)
    lg = rng.randn(B, N, D).astype(np.float32)
    zero = rng.rand(B, N) < 0.2
    lg[..., 0][zero] = 9.0
    return lg, rng


def _align_ctl(lg, lengths, q, ds, dcap, fcap, ctl=True):
    """one launch on buffers filled with a canary -> (durs [B, N], f2p [B, fcap], flen [B]) as numpy"""
    from ttscube_amd import _lib
    B, N, D = lg.shape
    dev = torch.device('cuda:0')
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt) if a is not None else None
    logits, len_t, q_t, ds_t = t(lg, torch.float32), t(lengths, torch.int32), t(q, torch.int32), t(ds, torch.int32)
    durs = torch.full((B, N), CANARY, dtype=torch.int32, device=dev)
    f2p = torch.full((B, fcap), CANARY, dtype=torch.int32, device=dev)
    flen = torch.full((B,), CANARY, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        if ctl:
            _lib.check(_lib.lib().ttsc_align_durations_ctl(_ptr(logits), _ptr(len_t), B, N, D, _ptr(durs), _ptr(f2p), _ptr(flen), fcap, _ptr(q_t), _ptr(ds_t),
                                                           dcap, _lib.current_stream()), 'ttsc_align_durations_ctl')
        else:
            _lib.check(_lib.lib().ttsc_align_durations(_ptr(logits), _ptr(len_t), B, N, D, _ptr(durs), _ptr(f2p), _ptr(flen), fcap, _lib.current_stream()),
                       'ttsc_align_durations')
    torch.cuda.synchronize()
    return durs.cpu().numpy(), f2p.cpu().numpy(), flen.cpu().numpy()


LENS_B5 = [1, 255, 256, 257, 300]      # the 256-phone pass boundary of the kernel


@pytest.mark.parametrize('D', [8, 101])
@pytest.mark.parametrize('batch', ['b1', 'b5'])
@pytest.mark.parametrize('pattern', ['quarter', 'four', 'random', 'set', 'dcap', 'fcap'])
def test_align_durations_ctl_equals_the_restatement(D, batch, pattern):
    """durs, f2p[:, :flen] and flen, exact integer equality; nothing is written behind a row's flen entries"""
    B, N, lengths = (1, 37, None) if batch == 'b1' else (5, 300, np.asarray(LENS_B5, np.int32))
    lg, rng = _logits(B, N, D, seed=D * 10 + B)
    ds, dcap, fcap = None, None, None
    if pattern == 'quarter':
        q = PR.q16(np.full((B, N), 0.25))
    elif pattern == 'four':
        q = PR.q16(np.full((B, N), 4.0))
    else:
        q = PR.q16(np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=(B, N))))
    if pattern == 'set':
        ds = np.full((B, N), -1, np.int32)
        pick = rng.rand(B, N) < 0.2
        ds[pick] = rng.randint(0, 2 * D, size=int(pick.sum()))
        ds[:, 0] = 0                                           # (0 among the values: the phone is dropped)
        ds[:, N // 3] = 3 * D
    if dcap is None:
        dcap = -(-(D - 1) * int(q.max()) // 65536)
        if ds is not None:
            dcap = max(dcap, int(ds.max()))
    if pattern == 'dcap':
        dcap = max(2, (D - 1) // 2)                            # (half the largest argmax at scales up to 4: engages on many phones)
    fcap = N * dcap
    want = PR.align_durations(lg, lengths, q, ds, dcap)
    if pattern == 'fcap':
        fcap = max(1, int(want[2].max()) // 2)                 # (smaller than the longest row's total: flen clamps, the tail is dropped)
        want = PR.align_durations(lg, lengths, q, ds, dcap, fcap)
        assert (want[2] == fcap).any()
    if pattern == 'dcap':
        assert sum(PR.durations_row(np.argmax(lg[b], axis=1)[:(N if lengths is None else lengths[b])], q[b], None, dcap)[3] for b in range(B)) > 0
    durs, f2p, flen = _align_ctl(lg, lengths, q, ds, dcap, fcap)
    assert np.array_equal(flen, want[2])
    assert np.array_equal(durs, want[0])
    for b in range(B):
        assert np.array_equal(f2p[b, :flen[b]], want[1][b]), 'row %d' % b
        assert (f2p[b, flen[b]:] == CANARY).all(), 'row %d: written behind its frames' % b


@pytest.mark.parametrize('D', [8, 101])
def test_align_durations_ctl_identity_is_the_uncontrolled_kernel_bit_for_bit(D):
    """scale 65536 and dur_set -1 (as tensors, and as NULL pointers) give ttsc_align_durations' buffers on the same logits — every word of them"""
    lengths = np.asarray(LENS_B5, np.int32)
    lg, _ = _logits(5, 300, D, seed=77 + D)
    fcap = 300 * (D - 1)
    base = _align_ctl(lg, lengths, None, None, 0, fcap, ctl=False)
    assert base[2].max() > 0
    one, none = np.full((5, 300), 65536, np.int32), np.full((5, 300), -1, np.int32)
    for q, ds in ((one, none), (None, None), (one, None), (None, none)):
        got = _align_ctl(lg, lengths, q, ds, D - 1, fcap)
        for a, b in zip(got, base):
            assert np.array_equal(a, b)


# ---- ttsc_cond_input_ctl --------------------------------------------------------------------------------------------------------------------
MAX_PITCH = 280.0


def _cond_case(C, seed=5):
    """B = 4: row 0 without a frame, row 1 without a voiced frame, row 2 with range 1 (and fewer frames than the batch), row 3 with range 1.3;
    multipliers between 0.4 and 2.5, so that voiced frames reach both clamps"""
    rng = np.random.RandomState(seed)
    B, N, F, fcap = 4, 9, 150, 200
    flen = np.asarray([0, 150, 97, 150], np.int32)
    f2p = np.zeros((B, fcap), np.int32)
    for b in range(B):
        f2p[b, :flen[b]] = np.sort(rng.randint(0, N, size=flen[b]))
    g = rng.randn(B, N, C).astype(np.float32)
    op = rng.rand(B, F, 2).astype(np.float32)
    op[1, :, 1] *= 0.49                                        # (row 1: every frame unvoiced)
    mul = np.exp(rng.uniform(np.log(0.4), np.log(2.5), size=(B, N))).astype(np.float32)
    prange = np.asarray([1.3, 1.3, 1.0, 1.3], np.float32)
    return g, f2p, flen, op, mul, prange


def _cond_ctl(g, f2p, flen, op, mul, prange, ctl=True):
    from ttscube_amd import _lib
    dev = torch.device('cuda:0')
    B, N, C = g.shape
    F, fcap, Cp = op.shape[1], f2p.shape[1], (C + 1 + 3) // 4 * 4
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g_t, f2p_t, flen_t, op_t = t(g), t(f2p), t(flen), t(op)
    pitch = torch.full((B, F), float('nan'), device=dev)
    gin = torch.full((B, F, Cp), float('nan'), device=dev)
    with _lib.on_device(dev):
        if ctl:
            mul_t, rng_t = t(mul), t(prange)
            _lib.check(_lib.lib().ttsc_cond_input_ctl(_ptr(g_t), _ptr(f2p_t), _ptr(flen_t), _ptr(op_t), MAX_PITCH, B, N, C, Cp, fcap, F, _ptr(pitch), _ptr(gin),
                                                      _ptr(mul_t), _ptr(rng_t), _lib.current_stream()), 'ttsc_cond_input_ctl')
        else:
            _lib.check(_lib.lib().ttsc_cond_input(_ptr(g_t), _ptr(f2p_t), _ptr(flen_t), _ptr(op_t), MAX_PITCH, B, N, C, Cp, fcap, F, _ptr(pitch), _ptr(gin),
                                                  _lib.current_stream()), 'ttsc_cond_input')
    torch.cuda.synchronize()
    return pitch.cpu().numpy(), gin.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('C', [6, 8])       # the scalar and the float4 copy of the gathered row
def test_cond_input_ctl_equals_the_restatement_bit_for_bit(C):
    g, f2p, flen, op, mul, prange = _cond_case(C)
    pitch, gin = _cond_ctl(g, f2p, flen, op, mul, prange)
    want_p, want_g = PR.cond_input(g, [f2p[b] for b in range(4)], flen, op, MAX_PITCH, mul, prange, gin.shape[2])
    assert np.array_equal(_bits(pitch), _bits(want_p))
    assert np.array_equal(_bits(gin), _bits(want_g))
    voiced = np.rint(op[..., 1]) == 1
    assert (pitch[voiced] == np.float32(MAX_PITCH)).any() and (pitch[voiced] == 0).any()          # both clamps were reached
    assert (pitch[1] == 0).all() and (pitch[~voiced] == 0).all()
    # every row alone gives the row it has in the batch
    for b in range(4):
        p1, g1 = _cond_ctl(g[b:b + 1], f2p[b:b + 1], flen[b:b + 1], op[b:b + 1], mul[b:b + 1], prange[b:b + 1])
        assert np.array_equal(_bits(p1[0]), _bits(pitch[b])) and np.array_equal(_bits(g1[0]), _bits(gin[b])), 'row %d' % b
    # the documented summation order against a plain sequential float64 sum of the voiced frames: within one float32 ulp of the pitch
    b = 3
    vuv = np.rint(op[b, :, 1]).astype(np.float32)
    p0 = (op[b, :, 0] * np.float32(MAX_PITCH)).astype(np.float32) * vuv
    seq = np.float64(0)
    for v in p0[:flen[b]][vuv[:flen[b]] == 1]:
        seq += np.float64(v)
    rows = PR.frame_rows(f2p[b], int(flen[b]), op.shape[1])
    alt = PR.pitch_row(op[b], int(flen[b]), MAX_PITCH, mul[b][rows], prange[b], mean=np.float32(seq / np.count_nonzero(vuv[:flen[b]] == 1)))
    assert (np.abs(alt.astype(np.float64) - pitch[b]) <= np.spacing(np.maximum(np.abs(alt), np.abs(pitch[b])))).all()


@pytest.mark.parametrize('C', [6, 8])
def test_cond_input_ctl_identity_is_the_uncontrolled_kernel_bit_for_bit(C):
    g, f2p, flen, op, _, _ = _cond_case(C, seed=6)
    base_p, base_g = _cond_ctl(g, f2p, flen, op, None, None, ctl=False)
    got_p, got_g = _cond_ctl(g, f2p, flen, op, np.ones((4, 9), np.float32), np.ones((4,), np.float32))
    assert np.array_equal(_bits(got_p), _bits(base_p)) and np.array_equal(_bits(got_g), _bits(base_g))
    assert not np.isnan(got_g).any()


# ---- model level: the seeded model directory of tests/test_api_gpu.py (16 phones, max_duration 7, PhoneText2Feat) --------------------------------
class _Enc:
    def __init__(self):
        self.phon2int = {p: i for i, p in enumerate('a b c d e f g h i j k l m n o p'.split())}
        self.speaker2int = {'s0': 0, 's1': 1}
        self.max_pitch = 280
        self.max_duration = 7


def _make_model_dir(tmp_path):
    """<dir>/cubegan.{yaml,encodings,model}: the helper of tests/test_api_gpu.py"""
    from ttscube_amd.io_utils.io_cubegan import CubeganEncodings
    from ttscube_amd.networks.cubegan import Cubegan
    enc = CubeganEncodings()
    e = _Enc()
    enc.phon2int, enc.speaker2int, enc.max_pitch, enc.max_duration = e.phon2int, e.speaker2int, e.max_pitch, e.max_duration
    base = os.path.join(str(tmp_path), 'cubegan')
    enc.save(base + '.encodings')
    yaml.dump({'sample_rate': 24000, 'hop_size': 240, 'conditioning': None}, open(base + '.yaml', 'w'))
    model = Cubegan(enc, conditioning=None, train=True)
    lsd = M.fill_state_dict(M.named_shapes(model._languasito), 5)
    gsd = R.synthetic_state_dict(dict(R.CONFIG_V1), seed=6)
    sd = model.state_dict()
    sd.update({'_languasito.' + k: v for k, v in lsd.items()})
    sd.update({'_generator.' + k: v for k, v in gsd.items()})
    model.load_state_dict(sd, strict=True)
    del model._mpd, model._msd, model._dummy
    model.save(base + '.model')
    return base


@pytest.fixture(scope='module')
def tts(tmp_path_factory):
    from ttscube_amd.api import TTSCube
    return TTSCube(_make_model_dir(tmp_path_factory.mktemp('prosody_model')), None)


TEXT = 'a b c | d e f g | h a'


def _aux(tts, text, speaker='s1', **ctl):
    """Languasito2.inference(return_aux=True) on one sentence with the call-level controls attached as TTSCube attaches them
    -> (durations [n], frames, X)"""
    from ttscube_amd.io_utils.prosody import Prosody
    ex = tts._example(text, speaker)
    X = tts._collate.collate_fn([ex])
    if ctl:
        tts._attach_controls(X, [ex['meta']], [text], [[(0, len(text), Prosody(**ctl))]])
    _, durs, flens = tts._model._languasito.inference(X, return_aux=True)
    return np.asarray(durs)[0], int(flens[0]), X


def test_identity_arguments_are_the_uncontrolled_call(tts):
    a = tts(TEXT, speaker='s1')
    b = tts(TEXT, speaker='s1', rate=1.0, pitch=0.0, pitch_range=1.0)
    assert a.dtype == b.dtype == np.int16 and np.array_equal(a, b)
    assert np.array_equal(tts(TEXT, speaker='s1', markup=True), a)           # (tag-free markup too)


@pytest.mark.parametrize('rate', [0.5, 2.0])
def test_rate_scales_the_durations_as_the_restatement_says(tts, rate):
    d0, f0, _ = _aux(tts, TEXT)
    assert f0 == d0.sum() > 0
    d1, f1, X = _aux(tts, TEXT, rate=rate)
    want, emitted, _, _ = PR.durations_row(d0, PR.q16(np.full(len(d0), 1.0 / rate)))
    assert np.array_equal(d1, want) and f1 == emitted and f1 != f0
    assert X['y_frame2phone'].tolist() == [np.repeat(np.arange(len(d0)), want).tolist()]
    audio = tts(TEXT, speaker='s1', rate=rate)
    assert audio.shape == (240 * emitted + 64,)


def test_pitch_and_range_move_the_pitch_input_as_the_restatement_says(tts):
    _, f0, X0 = _aux(tts, TEXT)
    p0 = X0['y_pitch'].cpu().numpy()[0]
    voiced = p0 != 0                 # (a voiced frame's pitch is sigmoid * 280: never 0)
    assert voiced.any() and p0.shape == (f0,)
    _, f1, X1 = _aux(tts, TEXT, rate=1.0, pitch=3.0, pitch_range=1.3)
    assert f1 == f0 and 'x_dur_scale' not in X1 and 'x_pitch_mul' in X1 and 'x_pitch_range' in X1
    mul = np.full(f0, np.float32(2.0 ** (3.0 / 12.0)), np.float32)
    want = PR.pitch_from_p0(p0, voiced, f0, 280.0, mul, np.float32(1.3))
    got = X1['y_pitch'].cpu().numpy()[0]
    assert np.array_equal(_bits(got), _bits(want)) and not np.array_equal(got, p0)
    # and a pitch alone leaves the mean out of it
    _, _, X2 = _aux(tts, TEXT, pitch=-2.0)
    mul = np.full(f0, np.float32(2.0 ** (-2.0 / 12.0)), np.float32)
    assert np.array_equal(_bits(X2['y_pitch'].cpu().numpy()[0]), _bits(PR.pitch_from_p0(p0, voiced, f0, 280.0, mul, np.float32(1.0))))
    assert len(tts(TEXT, speaker='s1', pitch=3.0, pitch_range=1.3)) == 240 * f0 + 64


def test_controlled_rows_of_a_pipelined_batch_equal_the_single_calls(tts):
    """five texts, a different control each (one of them none at all), max_batch = 2: three padded batches through Cubegan.inference_pipelined —
    the controls of batch k + 1 travel with its text stack"""
    rng = np.random.RandomState(0)
    syms = 'a b c d e f g h i j k l m n o p'.split()
    texts = [' '.join(rng.choice(syms, size=n)) for n in (9, 3, 14, 6, 11)]
    rates, pitches, ranges = [0.8, 1.0, 1.6, 1.0, 0.5], [0.0, 2.0, -3.0, 0.0, 1.0], [1.0, 1.3, 1.0, 1.0, 0.7]
    batch = tts.synthesize_batch(texts, speaker='s0', max_batch=2, rate=rates, pitch=pitches, pitch_range=ranges)
    plain = tts.synthesize_batch(texts, speaker='s0', max_batch=2)
    for i, t in enumerate(texts):
        solo = tts(t, speaker='s0', rate=rates[i], pitch=pitches[i], pitch_range=ranges[i])
        assert batch[i].shape == solo.shape and np.array_equal(batch[i], solo), i
        assert np.array_equal(batch[i], plain[i]) == (i == 3), i               # (the controls did something, except where none was given)


def test_markup_breaks_and_nested_prosody(tts):
    text = 'a b c | d<break time="300ms"/> e f g <break time="0.5s"/>h a'
    got = tts(text, speaker='s1', markup=True)
    parts = [tts(t, speaker='s1') for t in ('a b c | d', ' e f g ', 'h a')]
    want = np.concatenate([parts[0], np.zeros(round(0.3 * 24000), np.int16), parts[1], np.zeros(round(0.5 * 24000), np.int16), parts[2]])
    assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(tts.synthesize_batch(['h a', text], speaker='s1', markup=[False, True], max_batch=2)[1], want)
    nested = tts('<prosody rate="2"><prosody rate="0.625" pitch="+2st" range="1.3">a b c | d e</prosody></prosody>', speaker='s1', markup=True)
    flat = tts('a b c | d e', speaker='s1', rate=1.25, pitch=2.0, pitch_range=1.3)
    assert np.array_equal(nested, flat) and not np.array_equal(flat, tts('a b c | d e', speaker='s1'))
    # a span over some of the words only: those phones, and no others, change their durations
    d0, _, _ = _aux(tts, 'a b c | d e f g | h a')
    from ttscube_amd.io_utils.prosody import parse_markup
    seg, = parse_markup('a b c | <prosody rate="0.5">d e f g</prosody> | h a')
    ex = tts._example(seg.text, 's1')
    X = tts._collate.collate_fn([ex])
    tts._attach_controls(X, [ex['meta']], [seg.text], [seg.spans])
    _, d1, _ = tts._model._languasito.inference(X, return_aux=True)
    q = PR.q16(np.asarray([1, 1, 1, 2, 2, 2, 2, 1, 1], np.float64))
    assert np.array_equal(np.asarray(d1)[0], PR.durations_row(d0, q)[0])
    with pytest.raises(ValueError, match='offset 2'):
        tts('a <loud>b</loud>', markup=True)


def test_story_takes_the_controls_for_every_paragraph(tts):
    from ttscube_amd.story import StoryCube
    music = (0.1 * np.sin(np.arange(4000) / 20.0)).astype(np.float32)
    story = StoryCube(None, cube=tts, music=music)
    text = 'a b c d\n\ne f g'
    plain, fast = story(text, speaker='s1'), story(text, speaker='s1', rate=2.0, pitch=1.0)
    want = sum(len(tts(p, speaker='s1', rate=2.0, pitch=1.0)) for p in text.split('\n\n'))
    assert len(plain['audio']) - len(fast['audio']) == sum(len(tts(p, speaker='s1')) for p in text.split('\n\n')) - want > 0


# ---- two-stage path --------------------------------------------------------------------------------------------------------------------------
def test_two_stage_rate_breaks_and_pitch_refusal(tmp_path):
    from tests import test_twostage_cpu as TS
    from tests.test_twostage_gpu import _model_dir
    from ttscube_amd.api import TTSCubeTwoStage
    from ttscube_amd.networks.modules import align_durations
    base, vck = _model_dir(tmp_path)
    tts = TTSCubeTwoStage(base, vck)
    sent = TS.sentences_five()[0]
    text, spk, seed = TS.phone_text(sent), str(sent[1] - 1), 4242
    today = tts(text, speaker=spk, seed=seed)
    assert len(today) > 64
    assert np.array_equal(tts(text, speaker=spk, seed=seed, rate=1.0, markup=False), today)       # the identity call: sample for sample
    assert np.array_equal(tts(text, speaker=spk, seed=seed, markup=True), today)
    # rate: the frame count is the restatement's on the model's own argmax durations, cut to whole AR steps
    X = TS.solo_batch(sent)
    with torch.no_grad():
        _, out_dur = tts._model._text_stack(X['x_char'].cuda(), X['x_speaker'].cuda(), None)
        d0 = align_durations(out_dur, None).durations()[0]
    assert 240 * (int(d0.sum()) // TS.PFRAMES * TS.PFRAMES) + 64 == len(today)
    for rate in (0.5, 2.0):
        _, emitted, _, _ = PR.durations_row(d0, PR.q16(np.full(len(d0), 1.0 / rate)))
        frames = emitted // TS.PFRAMES * TS.PFRAMES
        got = tts(text, speaker=spk, seed=seed, rate=rate)
        assert len(got) == (240 * frames + 64 if frames else 0) and len(got) != len(today), rate
        assert np.array_equal(tts.synthesize_batch([text, text], speaker=spk, seed=seed - 1, rate=[1.0, rate])[1], got)
    # a break: two rows, the second with the documented key of segment 1
    words = text.split()
    a, b = ' '.join(words[:6]), ' '.join(words[6:])
    got = tts(a + '<break time="100ms"/>' + b, speaker=spk, seed=seed, markup=True)
    want = np.concatenate([tts(a, speaker=spk, seed=seed), np.zeros(2400, np.int16), tts(b, speaker=spk, seed=TTSCubeTwoStage._segment_key(seed, 1))])
    assert np.array_equal(got, want)
    assert TTSCubeTwoStage._segment_key(seed, 0) == seed
    # no pitch input at inference: refused, not dropped
    for kw in ({'pitch': 1.0}, {'pitch_range': 1.2}):
        with pytest.raises(ValueError, match='pitch'):
            tts(text, speaker=spk, seed=seed, **kw)
    with pytest.raises(ValueError, match='pitch'):
        tts('<prosody pitch="+2st">%s</prosody>' % text, speaker=spk, seed=seed, markup=True)
    with pytest.raises(ValueError, match='pitch'):
        tts._model.inference_batch(dict(TS.padded_batch([sent]), x_pitch_mul=np.ones((1, len(sent[0])), np.float32)), seeds=[seed])
