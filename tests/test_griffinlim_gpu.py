"""GPU: the LDS FFT kernels (csrc/stft_fft.hip) behind io_utils/stft.py and the rest of MelVocoder, against the float64 restatement
tests/griffinlim_reference.py.  Signals and spectra go to the device rounded to float32 once; the restatement gets what the device gets where the
check is about the transform (1), and the unrounded case where the bound is stated against the case's own signal (2, 3).

Measured deviations are printed before every assertion (pytest -s shows them; DESIGN.md §9h records them)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import griffinlim_reference as R
from ttscube_amd import _lib
from ttscube_amd.io_utils import stft
from ttscube_amd.io_utils.vocoder import GriffinLimVocoder, MelVocoder

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -24
ALL = list(range(len(R.CASES)))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).to(DEV)


def _rel2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ---- 1. STFT --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', ALL)
def test_stft_meets_the_radix_fft_bound(i):
    """per frame ||S^ - S||_2 <= 8 u log2(n_fft) ||S||_2: Higham Thm 24.2 (eta ~ 7u with float32 twiddles) plus one rounding for the window"""
    c = R.case(i)
    y32 = c['y'].astype(np.float32)
    S = R.stft(y32.astype(np.float64), c['n_fft'], c['hop'])
    got = stft.stft(_dev(y32), n_fft=c['n_fft'], hop=c['hop'])
    assert got.dtype == torch.complex64 and tuple(got.shape) == (c['F'], c['nb'])
    got = got.cpu().numpy().astype(np.complex128)
    err = np.linalg.norm(got - S, axis=1) / np.linalg.norm(S, axis=1)
    bound = 8 * U * math.log2(c['n_fft'])
    print('stft case %d: worst frame %.3e, bound %.3e' % (i, err.max(), bound))
    assert np.all(got[:, [0, -1]].imag == 0.0)
    assert err.max() <= bound


# ---- 2. iSTFT of a consistent spectrum -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 2, 3, 4, 5, 6, 7, 8])
def test_istft_of_a_consistent_spectrum(i):
    """||y^ - y||_2 <= (8 log2 n_fft + ceil(n_fft / hop) + 4) u sqrt(env_max / env_min) ||y||_2: the frame error of (1), ||frames||_2 <=
    sqrt(env_max) ||y||_2, and a least-squares inverse of norm 1 / sqrt(env_min)"""
    c = R.case(i)
    n, hop = c['n_fft'], c['hop']
    env = R.envelope(n, hop, c['F'])[n // 2:n // 2 + c['L']]
    got = stft.istft(_dev(c['S'], torch.complex64), hop=hop)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c['L'],)
    err = _rel2(got.cpu().numpy(), c['y'])
    bound = (8 * math.log2(n) + -(-n // hop) + 4) * U * math.sqrt(env.max() / env.min())
    print('istft case %d: %.3e, bound %.3e' % (i, err, bound))
    assert err <= bound


# ---- 3. Griffin-Lim against the float64 restatement -----------------------------------------------------------------------------------
def _measured_bound(y32, y64, well_conditioned=True):
    """16 x what the float32 restatement itself loses on this case; the condition under which that is a meaningful yardstick is asserted"""
    if well_conditioned:
        assert np.abs(y32 - y64).max() <= 1e-5 * np.abs(y64).max()
    return 16 * _rel2(y32, y64)


@pytest.mark.parametrize('n_iter', [0, 1, 8])
@pytest.mark.parametrize('i', ALL)
def test_griffinlim_against_the_restatement(i, n_iter):
    c = R.case(i)
    y64 = R.griffinlim_case(i, n_iter)
    bound = _measured_bound(R.griffinlim_case(i, n_iter, np.float32), y64)
    got = stft.griffinlim(_dev(c['mag']), n_iter=n_iter, hop=c['hop'], angles=_dev(c['angles'], torch.complex64))
    assert got.dtype == torch.float32 and tuple(got.shape) == (c['L'],)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = _rel2(got, y64)
    print('griffinlim case %d n_iter %d: %.3e, float32 restatement %.3e, bound %.3e' % (i, n_iter, err, bound / 16, bound))
    assert err <= bound


def test_istft_with_an_envelope_of_zero():
    """case 1, hop = n_fft: the samples at the frame joins have envelope 0 and stay undivided (exact zeros).  Same 16 x rule as above, but the
    1e-5 max-norm condition cannot be asserted for THIS input: beside a join the envelope is window[1]^2 = 2.3e-8, and the consistent spectrum's
    frames are that small there too, so the division returns the float32 transform's absolute error (~1e-8) at full scale — the float32
    restatement itself is 2.2e-4 of the peak off at those samples (the Griffin-Lim runs of case 1 start from random phases, whose frames are
    not small there; they meet the condition)."""
    c = R.case(1)
    y64 = R.istft(c['S'], c['hop'])
    y32 = R.istft(c['S'].astype(np.complex64), c['hop'], np.float32)
    bound = _measured_bound(y32, y64, well_conditioned=False)
    got = stft.istft(_dev(c['S'], torch.complex64), hop=c['hop']).cpu().numpy()
    err = _rel2(got, y64)
    print('istft case 1: %.3e, float32 restatement %.3e (max-norm %.3e of the peak), bound %.3e'
          % (err, bound / 16, np.abs(y32 - y64).max() / np.abs(y64).max(), bound))
    assert np.all(got[c['n_fft'] // 2::c['hop']] == 0.0)                  # q = t + n_fft/2 a multiple of n_fft: window[0]^2 = 0
    assert err <= bound


# ---- 4. monotone projections ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 2, 4, 5])
def test_projections_do_not_increase_the_inconsistency(i):
    c = R.case(i)
    mag, ang = _dev(c['mag']), _dev(c['angles'], torch.complex64)
    e = []
    for k in (0, 1, 2, 4, 8):
        y = stft.griffinlim(mag, n_iter=k, hop=c['hop'], angles=ang)
        e.append(float(torch.linalg.norm((mag - stft.stft(y, n_fft=c['n_fft'], hop=c['hop']).abs()).double())))
    print('inconsistency case %d:' % i, ' '.join('%.6e' % v for v in e))
    for a, b in zip(e, e[1:]):
        assert b <= a + 1e-4 * e[0], e
    assert e[-1] < e[0]


# ---- 5. bits ----------------------------------------------------------------------------------------------------------------------------
def _ragged():
    """cases 4 and 5 and a 7-frame row at n_fft 1024 / hop 256"""
    rng = np.random.RandomState(7)
    t = np.arange(256 * 6)
    y7 = 0.4 * np.sin(2 * np.pi * 0.02 * t) + 0.1 * rng.randn(t.size)
    rows = []
    for y, a in ((R.case(4)['y'], R.case(4)['angles']), (R.case(5)['y'], R.case(5)['angles']),
                 (y7, np.exp(2j * np.pi * rng.rand(513, 7)).T)):
        S = R.stft(y, 1024, 256)
        rows.append(dict(y=y.astype(np.float32), S=S.astype(np.complex64), mag=np.abs(S).astype(np.float32), ang=a.astype(np.complex64), F=S.shape[0]))
    return rows


def _stack(rows, key, order, shape, dtype):
    out = np.full((len(order),) + shape, np.nan, dtype=dtype)
    for k, r in enumerate(order):
        a = rows[r][key]
        out[(k,) + tuple(slice(0, s) for s in a.shape)] = a
    return out


@pytest.mark.parametrize('what', ['stft', 'istft', 'griffinlim'])
def test_rows_have_the_bits_they_have_alone(what):
    rows = _ragged()
    Fmax, Lmax = 10, 2304

    def alone(r):
        if what == 'stft':
            return stft.stft(_dev(r['y']), n_fft=1024, hop=256).cpu().numpy()
        if what == 'istft':
            return stft.istft(_dev(r['S'], torch.complex64), hop=256).cpu().numpy()
        return stft.griffinlim(_dev(r['mag']), n_iter=2, hop=256, angles=_dev(r['ang'], torch.complex64)).cpu().numpy()

    def batch(order):
        frames = [rows[r]['F'] for r in order]
        if what == 'stft':
            out = stft.stft(_dev(_stack(rows, 'y', order, (Lmax,), np.float32)), lengths=[256 * (f - 1) for f in frames], n_fft=1024, hop=256)
        elif what == 'istft':
            out = stft.istft(_dev(_stack(rows, 'S', order, (Fmax, 513), np.complex64), torch.complex64), frames=frames, hop=256)
        else:
            out = stft.griffinlim(_dev(_stack(rows, 'mag', order, (Fmax, 513), np.float32)), frames=frames, n_iter=2, hop=256,
                                  angles=_dev(_stack(rows, 'ang', order, (Fmax, 513), np.complex64), torch.complex64))
        return out.cpu().numpy()

    single = [alone(r) for r in rows]
    for order in ((0, 1, 2), (2, 0, 1)):
        first, second = batch(order), batch(order)
        assert not np.isnan(first.view(np.float32)).any()
        np.testing.assert_array_equal(first.view(np.float32), second.view(np.float32))
        for k, r in enumerate(order):
            n = single[r].shape[0]
            np.testing.assert_array_equal(first[k, :n].view(np.float32), single[r].view(np.float32))
            assert np.all(first[k, n:] == 0)
    assert any(s.shape[0] < (Fmax if what == 'stft' else Lmax) for s in single)


# ---- 6. degenerate data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_iter', [0, 3])
def test_zero_magnitude_gives_zero_audio(n_iter):
    c = R.case(0)
    y = stft.griffinlim(torch.zeros((c['F'], c['nb']), device=DEV), n_iter=n_iter, hop=c['hop'], angles=_dev(c['angles'], torch.complex64))
    assert tuple(y.shape) == (c['L'],) and bool((y == 0).all())


def test_negative_magnitudes_count_as_their_absolute_value():
    c = R.case(3)
    sign = np.where(np.random.RandomState(1).rand(c['F'], c['nb']) < 0.5, -1.0, 1.0)
    ang = _dev(c['angles'], torch.complex64)
    for n_iter in (0, 2):
        a = stft.griffinlim(_dev(c['mag']), n_iter=n_iter, hop=c['hop'], angles=ang)
        b = stft.griffinlim(_dev(c['mag'] * sign), n_iter=n_iter, hop=c['hop'], angles=ang)
        assert torch.equal(a, b)


def test_tiny_and_mixed_scale_signals_stay_finite():
    """the phase normalisation neither underflows (|z| ~ 1e-20, squares are 0 in float32) nor overflows (|z| ~ 1e19, squares are inf)"""
    c = R.case(8)
    for scale in (1.0, 1e-18, 1e39):
        y = stft.griffinlim(_dev(c['mag'] * scale), n_iter=3, hop=c['hop'], angles=_dev(c['angles'], torch.complex64))
        assert bool(torch.isfinite(y).all()), scale


# ---- 7. the MelVocoder mirror ---------------------------------------------------------------------------------------------------------
def test_melvocoder_mirrors_the_tensor_functions():
    c = R.case(5)
    v = MelVocoder(device=DEV)
    y = c['y'].astype(np.float32)
    S = v.fft(y, 16000, use_preemphasis=False)
    assert S.dtype == np.complex64 and S.shape == (c['F'], c['nb'])
    np.testing.assert_array_equal(S, stft.stft(_dev(y), n_fft=1024, hop=256).cpu().numpy())
    Sp = v.fft(y, 16000)
    np.testing.assert_array_equal(Sp, stft.stft(_dev(v._preemphasis(y)), n_fft=1024, hop=256).cpu().numpy())
    assert np.abs(Sp - S).max() > 0
    back = v.ifft(S, 16000)
    assert back.dtype == np.float32 and back.shape == (c['L'],)
    np.testing.assert_array_equal(back, stft.istft(_dev(S, torch.complex64), hop=256).cpu().numpy())
    mag = np.abs(S)
    np.random.seed(5)
    a = v.griffinlim(mag, n_iter=2)
    np.random.seed(5)
    ang = np.exp(2j * np.pi * np.random.rand(c['nb'], c['F'])).T          # the reference draws on the transposed [nb, F] spectrogram
    b = stft.griffinlim(_dev(mag), n_iter=2, hop=256, angles=_dev(ang, torch.complex64)).cpu().numpy()
    assert a.dtype == np.float32 and a.shape == (c['L'],)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(v.griffinlim(mag, n_iter=2, angles=ang), b)
    np.testing.assert_array_equal(v.griffinlim(mag[None], n_iter=2, angles=ang[None])[0], b)


def test_melspectrogram_with_preemphasis():
    v = MelVocoder(device=DEV)
    y = R.case(6)['y'].astype(np.float32)
    a = v.melspectrogram(y, 24000, 80, 240, use_preemphasis=True)
    b = v.melspectrogram(v._preemphasis(y), 24000, 80, 240)
    assert a.shape == (7, 80)
    np.testing.assert_array_equal(a, b)
    assert np.abs(a - v.melspectrogram(y, 24000, 80, 240)).max() > 0


def test_griffinlim_vocoder_contract():
    c = R.case(6)
    mel10 = MelVocoder(device=DEV).melspectrogram(c['y'].astype(np.float32), 24000, 80, 240)        # [7, 80] log10-mel
    mel = torch.log(10 ** torch.from_numpy(mel10.T[None].copy()).to(DEV))                              # runtime.py:77: natural-log [1, 80, 7]
    voc = GriffinLimVocoder(n_iter=4, device=DEV)
    state = np.random.get_state()[1].copy()
    a, b = voc(mel), voc(mel)
    assert a.is_cuda and tuple(a.shape) == (1, 1, c['L']) and a.dtype == torch.float32
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) <= 1.0 and float(a.abs().max()) > 0.0
    assert torch.equal(a, b)
    np.testing.assert_array_equal(np.random.get_state()[1], state)       # its own generator, not numpy's global one


def test_mel_to_linear_is_the_clamped_pseudo_inverse():
    rng = np.random.RandomState(2)
    mel = rng.uniform(-3.0, 0.5, size=(2, 5, 80)).astype(np.float32)
    got = stft.mel_to_linear(_dev(mel), 24000, 80).cpu().numpy()
    x = (10.0 ** mel.astype(np.float64)).reshape(-1, 80)
    P = stft.mel_pinv(24000, 80)
    ref = np.maximum(0.0, x @ P.T).reshape(2, 5, 513)
    assert got.shape == ref.shape and got.min() >= 0.0
    # fp32 dot products of 80 terms: 80 products and sums, the rounding of P and of 10**mel: 88 u sum |p| |x| per entry
    bound = 88 * U * (np.abs(x) @ np.abs(P).T).reshape(2, 5, 513)
    assert np.all(np.abs(got - ref) <= bound)


# ---- 8. argument errors surface through the C ABI -------------------------------------------------------------------------------------
def test_argument_errors_through_the_c_abi():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    s = _lib.current_stream()
    short = (C.c_int32 * 2)(10, 3)
    fdev = C.c_void_p(torch.tensor([10, 3], dtype=torch.int32, device=DEV).data_ptr())
    bad = [(1000, 250, 8, None, None), (4096, 1024, 8, None, None), (1024, 0, 8, None, None), (1024, 1025, 8, None, None),
           (1024, 256, 3, None, None), (1024, 256, 10, short, fdev), (1024, 256, 10, short, None)]
    for n_fft, hop, Fmax, fh, fd in bad:
        B = 2 if fh is not None else 1
        for rc in (L.ttsc_stft_analyze(p, 1 << 14, fh, fd, B, Fmax, n_fft, hop, p, p, s),
                   L.ttsc_stft_synthesize(p, fh, fd, B, Fmax, n_fft, hop, p, p, s),
                   L.ttsc_stft_project(p, 1 << 14, p, fh, fd, B, Fmax, n_fft, hop, p, p, s),
                   L.ttsc_stft_overlap_add(p, fh, fd, B, Fmax, n_fft, hop, p, 0, p, max(hop, 1) * (Fmax - 1), s)):
            assert rc == -1
            with pytest.raises(_lib.TTSCError):
                _lib.check(rc, 'stft')
    assert L.ttsc_stft_reflect_pad(p, None, None, 1, 512, 1024, p, 512 + 1024, s) == -1        # 512 samples < 513
    assert L.ttsc_stft_reflect_pad(p, None, None, 1, 600, 1000, p, 1600, s) == -1
    assert L.ttsc_stft_analyze(p, 1024, None, None, 1, 4, 1024, 256, p, p, s) == -1            # Lpad too small for 4 frames
    assert L.ttsc_stft_overlap_add(p, None, None, 1, 4, 1024, 256, p, 1, p, 768, s) == -1      # the padded form has 768 + 1024 samples
    torch.cuda.synchronize()
    for fn, kw in ((stft.stft, dict(n_fft=1000)), (stft.stft, dict(hop=0)), (stft.stft, dict(hop=2000)), (stft.stft, dict(lengths=[700]))):
        with pytest.raises(_lib.TTSCError):
            fn(buf[:4096].view(1, -1), **kw)
    with pytest.raises(_lib.TTSCError):
        stft.griffinlim(buf[:3 * 513].view(3, 513), n_iter=1, hop=256)
    with pytest.raises(_lib.TTSCError):
        stft.istft(torch.zeros((2, 10, 513), dtype=torch.complex64, device=DEV), frames=[10, 3], hop=256)
