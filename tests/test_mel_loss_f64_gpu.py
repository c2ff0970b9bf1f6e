"""GPU: the mel-spectrogram of the 45 x mel-L1 loss (io_utils/melspec.py: DFT and mel projection as ttsc_linear_forward GEMMs, csrc/stft.hip
element-wise kernels) and MelVocoder's log10 features against the float64 oracle (oracle/gan_step_ref.py), forward and VJP of a fixed random
cotangent (not through the L1 loss, whose sign flips make any bound loose).

Every case asserts the DFT path it reaches (melspec.gemm_plan, the expressions _MelFn itself runs on): one GEMM over all B * Fp rows of a
batch or one launch per utterance (B = 1, or Fp == F when n_fft == hop), float4 or scalar row loads (hop % 4, per-utterance row alignment).
  forward  per element, log domain: |got - ref| <= TAU_MEL * ((mel . (A_f + |X|)) / max(lin, 1e-5) + |ref|), A_f = sum_n |frame_n hann_n|
           (oracle.gan_step_ref.log_mel_bound); elements whose lin sits within that bound of the 1e-5 clamp are excluded and counted (< 1 %)
  VJP      per utterance: relative L2 error and max|err| / max|ref| <= 4 x the float32 yardstick's + 1e-6
Measured on an MI355X: forward worst err / bound 0.27-3.5 * 2^-24 / TAU_MEL (i.e. <= 0.11 of the bound); VJP relative L2 6.5e-7 .. 9.7e-6 against a
yardstick of 7.3e-7 .. 3.0e-5 (n_fft = hop = 256: 7.0e-5 against 3.0e-5), max-relative 7.7e-7 .. 7.5e-5.
Batch vs solo: the batched DFT reads each utterance's frames from a different layout than a solo call, and the code claims no bit identity
between the two — both are held to float64 instead.  Straddle rows (the batched DFT's rows past an utterance's end, reading the next
utterance's samples) must carry nothing: a NaN-filled neighbour leaves the other utterances' values and gradients exact to the bounds."""
import numpy as np
import pytest
import torch

from oracle import gan_step_ref as R

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 1e-6
MEASURED = {}


def _signal(B, L, kind, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(L) / 24000.0
    y = np.stack([0.4 * np.sin(2 * np.pi * rng.uniform(80, 4000) * t + rng.uniform(0, 6)) + 0.05 * rng.randn(L) for _ in range(B)])
    if kind == 'silence':
        y[:, :max(L // 4, 1)] = 0.0         # leading digital silence: frames of exact zeros, lin at the clamp
    elif kind == 'full':
        y = np.sign(y + 1e-9 * rng.randn(B, L))   # full scale +-1
    elif kind == 'faint':
        y = 1e-4 * y
    return torch.from_numpy(y.astype(np.float32))


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), v)


def _check_forward(got, f, label, scale=1.0):
    """got [B, n_mels, F] (GPU result on the host), f the float64 oracle's dict"""
    ref = f['out']
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), label
    bound = R.log_mel_bound(f, R.TAU_MEL, scale)
    melA = bound / R.TAU_MEL - ref.abs()
    near = (f['lin'].transpose(1, 2) - 1e-5).abs() <= R.TAU_MEL * melA * f['lin'].transpose(1, 2).clamp(min=1e-5) / scale
    err = (got.double() - ref).abs()
    ratio = (err / bound)[~near]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _note('fwd ' + label, worst * R.TAU_MEL * 2 ** 24)
    assert worst <= 1.0, '%s forward: err / bound %.3g' % (label, worst)
    assert int(near.sum()) <= 0.01 * near.numel(), (label, int(near.sum()))


def _check_vjp(got, ref, yard, label, skip=()):
    for b in range(ref.shape[0]):
        if b in skip:
            continue
        g, r, y = got[b].double(), ref[b], yard[b].double()
        assert bool(torch.isfinite(g).all()), (label, b)
        rn, rm = float(r.norm()), float(r.abs().max())
        e2, ey2 = float((g - r).norm()) / rn, float((y - r).norm()) / rn
        em, eym = float((g - r).abs().max()) / rm, float((y - r).abs().max()) / rm
        _note('vjp l2 ' + label, e2)
        _note('vjp max ' + label, em)
        _note('yard l2 ' + label, ey2)
        assert e2 <= FACTOR * ey2 + FLOOR, '%s utt %d: rel L2 %.3e > 4 x %.3e + 1e-6' % (label, b, e2, ey2)
        assert em <= FACTOR * eym + FLOOR, '%s utt %d: max %.3e > 4 x %.3e + 1e-6' % (label, b, em, eym)


# (B, L, hop, n_fft, win, fmin, fmax, signal, path): path = (batched, vector)
CASES = [
    (1, 12000, 240, 1024, 1024, 0, 12000, 'silence', (False, True)),     # B = 1: per-utterance loop, one launch
    (2, 12000, 240, 1024, 1024, 0, 12000, 'full', (True, True)),
    (2, 12007, 240, 1024, 1024, 0, 12000, 'silence', (True, True)),      # straddle rows, L not a multiple of the hop
    (3, 5003, 240, 1024, 1024, 0, 12000, 'faint', (True, True)),
    (16, 48000, 240, 1024, 1024, 0, 12000, 'silence', (True, True)),     # the validation shape (networks/training.py)
    (1, 393, 240, 1024, 1024, 0, 12000, 'plain', (False, True)),         # shortest legal input: pad + 1 samples, one frame
    (2, 393, 240, 1024, 1024, 0, 12000, 'plain', (True, True)),
    (2, 12000, 256, 1024, 1024, 0, 12000, 'silence', (True, True)),
    (2, 12000, 275, 1024, 1024, 0, 12000, 'silence', (True, False)),     # hop % 4 != 0: scalar GEMM loads
    (1, 12007, 275, 1024, 1024, 0, 12000, 'plain', (False, False)),
    (2, 12000, 240, 1024, 800, 80, None, 'silence', (True, True)),       # win < n_fft, fmin > 0, fmax = None
    (3, 10240, 256, 256, 256, 0, 12000, 'plain', (False, True)),         # n_fft == hop, L % hop == 0: Fp == F per-utterance loop, B > 1
    (2, 2500, 250, 250, 250, 0, 12000, 'silence', (False, False)),       # ... with K = n_fft = 250 (not a multiple of 4): scalar
]


@pytest.mark.parametrize('B,L,hop,n_fft,win,fmin,fmax,kind,path', CASES)
def test_mel_forward_and_vjp_against_float64(B, L, hop, n_fft, win, fmin, fmax, kind, path):
    from ttscube_amd.io_utils import melspec as MS
    y = _signal(B, L, kind, seed=B * 7 + L)
    pad = int((n_fft - hop) / 2)
    plan = MS.gemm_plan(B, L + 2 * pad, n_fft, hop)
    assert (plan['batched'], plan['vector']) == path, plan
    label = 'B%d L%d hop%d n%d w%d %s' % (B, L, hop, n_fft, win, kind)
    a = y.cuda().requires_grad_(True)
    out = MS.mel_spectrogram(a, n_fft, 80, 24000, hop, win, fmin, fmax)
    f = R.mel_forward(y, n_fft, 80, 24000, hop, win, fmin, fmax)
    _check_forward(out.detach().cpu(), f, label)
    g = torch.randn(f['out'].shape, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    got, = torch.autograd.grad(out, a, g.float().cuda())
    ref = R.mel_vjp(f, g, n_fft, hop)
    yard = R.mel_vjp(R.mel_forward(y, n_fft, 80, 24000, hop, win, fmin, fmax, dtype=torch.float32), g, n_fft, hop, dtype=torch.float32)
    _check_vjp(got.cpu(), ref, yard, label)


@pytest.mark.parametrize('B,L,hop', [(3, 12007, 240), (3, 12000, 275), (2, 393, 240)])
def test_straddle_rows_carry_nothing(B, L, hop):
    """utterance 1 is all NaN: the batched DFT's rows past utterance 0's end read it, and nothing of it may reach utterance 0 or 2"""
    from ttscube_amd.io_utils import melspec as MS
    pad = int((1024 - hop) / 2)
    assert MS.gemm_plan(B, L + 2 * pad, 1024, hop)['batched']
    y = _signal(B, L, 'silence', seed=5)
    y[1] = float('nan')
    a = y.cuda().requires_grad_(True)
    out = MS.mel_spectrogram(a, 1024, 80, 24000, hop, 1024, 0, 12000)
    keep = [b for b in range(B) if b != 1]
    f = R.mel_forward(y[keep], 1024, 80, 24000, hop, 1024, 0, 12000)
    _check_forward(out.detach()[keep].cpu(), f, 'straddle L%d hop%d' % (L, hop))
    g = torch.randn((B,) + tuple(f['out'].shape[1:]), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got, = torch.autograd.grad(out, a, g.float().cuda())
    ref = R.mel_vjp(f, g[keep], 1024, hop)
    yard = R.mel_vjp(R.mel_forward(y[keep], 1024, 80, 24000, hop, 1024, 0, 12000, dtype=torch.float32), g[keep], 1024, hop, dtype=torch.float32)
    _check_vjp(got[keep].cpu(), ref, yard, 'straddle L%d hop%d' % (L, hop))


@pytest.mark.parametrize('B,L,kind', [(1, 24000, 'silence'), (3, 12007, 'full'), (2, 5003, 'faint'), (2, 4800, 'zero')])
def test_melvocoder_log10_forward_against_float64(B, L, kind):
    """MelVocoder.melspectrogram (log10, eps = 0, centred frames), an all-zero input included (every element at the clamp: exactly -5)"""
    from ttscube_amd.io_utils.vocoder import MelVocoder
    y = torch.zeros(B, L) if kind == 'zero' else _signal(B, L, kind, seed=L)
    got = torch.from_numpy(MelVocoder().melspectrogram(y.numpy(), sample_rate=24000, num_mels=80, hop_size=240))
    f = R.mel_forward(y, 1024, 80, 24000, 240, 1024, 0.0, None, pad=512, eps=0.0, scale=1.0 / R.LN10)
    _check_forward(got.transpose(1, 2), f, 'log10 B%d L%d %s' % (B, L, kind), scale=1.0 / R.LN10)
    if kind == 'zero':
        assert got.unique().numel() == 1 and abs(float(got[0, 0, 0]) + 5.0) < 1e-6


def test_zz_report_measured():
    """prints the worst measured errors of this module (forward: in units of 2^-24 of the bound's scale; VJP: relative)"""
    for k in sorted(MEASURED):
        print('MEASURED %-40s %.3e' % (k, MEASURED[k]))
