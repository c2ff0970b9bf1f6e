"""GPU parity: Languasito2 / CubenetTextcoder mirrors (HIP conv + GEMM + LSTM kernels) vs the reference-generated
goldens and the oracle.  Gates: <=1e-4 RMS and identical durations; Textcoder with injected masks."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + '.npz'))
    shapes = [(k, tuple(s)) for k, s in json.loads(str(z['shapes']))]
    return z, shapes, M.fill_state_dict(shapes, int(z['seed']))


@pytest.mark.parametrize('name', ['languasito2_a', 'languasito2_b'])
def test_languasito2_matches_reference_golden(golden_dir, name):
    from ttscube_amd.networks.modules import Languasito2
    z, shapes, sd = _load(golden_dir, name)
    cfg = json.loads(str(z['cfg']))
    net = Languasito2(cfg['num_phones'], cfg['num_speakers'], cfg['max_pitch'], cfg['max_duration'], cond_type=None)
    assert M.named_shapes(net) == shapes           # state_dict layout == the reference's (names, shapes, order)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    X = {'x_char': torch.from_numpy(z['x_char']), 'x_speaker': torch.from_numpy(z['x_speaker']), 'y_frame2phone': [[0]]}
    cond = net.inference(X).cpu()
    durs = np.bincount(np.asarray(X['y_frame2phone'][0], dtype=np.int64), minlength=z['x_char'].shape[1])
    assert list(durs) == list(z['durs'])
    assert cond.shape == z['cond'].shape
    assert float((cond - torch.from_numpy(z['cond'])).pow(2).mean().sqrt()) < 1e-4
    assert float((X['y_pitch'].cpu() - torch.from_numpy(z['pitch'])).abs().max()) < 1e-2


def test_languasito2_padded_batch_equals_per_utterance():
    """New capability (reference is B=1): a zero-padded batch reproduces each utterance run alone."""
    from ttscube_amd.networks.modules import Languasito2
    net = Languasito2(30, 2, 250, 8)
    net.load_state_dict(M.fill_state_dict(M.named_shapes(net), 77), strict=True)
    net = net.cuda().eval()
    rng = np.random.RandomState(1)
    lens = [13, 6, 9]
    x = np.zeros((3, 13), dtype=np.int64)
    for b, n in enumerate(lens):
        x[b, :n] = rng.randint(1, 31, size=n)
    spk = torch.tensor([[1], [2], [1]])
    cond, durs, flens = net.inference({'x_char': torch.from_numpy(x), 'x_speaker': spk}, return_aux=True)
    for b, n in enumerate(lens):
        solo = net.inference({'x_char': torch.from_numpy(x[b:b + 1, :n]), 'x_speaker': spk[b:b + 1]})
        assert solo.shape[1] == flens[b]
        assert float((cond[b, :flens[b]] - solo[0]).abs().max()) < 1e-5
        assert bool((cond[b, flens[b]:] == 0).all())


def test_textcoder_matches_reference_golden(golden_dir):
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    z, shapes, sd = _load(golden_dir, 'textcoder_a')

    class Enc:
        phon2int = {str(i): i for i in range(40)}
        speaker2int = {str(i): i for i in range(2)}
        max_pitch = 200
        max_duration = int(z['max_duration'])

    net = CubenetTextcoder(Enc())
    assert M.named_shapes(net) == shapes
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    X = {'x_char': torch.from_numpy(z['x_char']), 'x_speaker': torch.from_numpy(z['x_speaker'])}
    mel = net.inference(dict(X), dropout_masks=torch.from_numpy(z['masks']).unsqueeze(2)).cpu()
    assert mel.shape == z['mel'].shape
    assert float((mel - torch.from_numpy(z['mel'])).pow(2).mean().sqrt()) < 1e-4
    # persistent AR kernel == step-wise launches (same masks), and the Philox-dropout production path runs
    with torch.no_grad():
        h, out_dur = net._text_stack(X['x_char'].cuda(), X['x_speaker'].cuda(), None)
        durs = torch.argmax(out_dur, dim=-1).cpu().numpy().reshape(-1)
        from ttscube_amd.networks.modules import _expand_rows
        f2p = [p for p, d in enumerate(durs) for _ in range(int(d))]
        h, _ = _expand_rows(h, [f2p], stride=3)
        h = net._lstm('_rnn_overlay')(h)
        mk = torch.from_numpy(z['masks']).unsqueeze(2)
        a = net._ar_decode(h, mk)
        b = net._ar_decode_stepwise(h, mk)
        assert float((a - b).abs().max()) < 1e-4
        free = net.inference(dict(X))
        assert free.shape == mel.shape and bool(torch.isfinite(free).all())
    Xt = dict(X)
    Xt['y_frame2phone'] = [list(z['f2p_tf'])]
    Xt['y_mgc'] = torch.from_numpy(z['y_mgc'])
    o_dur, o_pitch, o_mel, o_post = net(Xt, dropout_masks=torch.from_numpy(z['masks_tf']))
    assert float((o_dur.cpu() - torch.from_numpy(z['tf_dur'])).abs().max()) < 1e-4
    assert float((o_mel.cpu() - torch.from_numpy(z['tf_mel'])).pow(2).mean().sqrt()) < 1e-4
    assert float((o_post.cpu() - torch.from_numpy(z['tf_post'])).pow(2).mean().sqrt()) < 1e-4


@pytest.mark.parametrize('B,N,D,stride', [(1, 30, 102, 1), (5, 67, 102, 1), (3, 300, 17, 3), (2, 1, 5, 1), (4, 513, 9, 3)])
def test_device_side_alignment_matches_host_loops(B, N, D, stride):
    """csrc/align.hip (ttsc_align_durations + ttsc_expand_rows) against the reference's host procedure: argmax -> nested
    loops -> index gather with the reference's padding rule (modules.py:946-953,1043-1053; textcoder.py:160-166,291-302)."""
    from ttscube_amd.networks.modules import _expand_rows, align_durations
    rng = np.random.RandomState(B * 1000 + N)
    logits = rng.randn(B, N, D).astype(np.float32)
    logits[:, ::7, :] = 0.25                      # ties: argmax must return the FIRST maximum (index 0)
    logits[0, :min(3, N), 0] = 50.0               # leading zero-length phones
    lens = [N] + [int(rng.randint(1, N + 1)) for _ in range(B - 1)]
    al = align_durations(torch.from_numpy(logits).cuda(), lens if B > 1 else None)
    durs = logits.argmax(-1)
    want_f2p = []
    for b in range(B):
        a = []
        for p in range(lens[b]):
            a.extend([p] * int(durs[b, p]))
        want_f2p.append(a)
    assert al.tolist() == want_f2p and al == want_f2p
    got_d = al.durations()
    for b in range(B):
        assert list(got_d[b, :lens[b]]) == list(durs[b, :lens[b]]) and not got_d[b, lens[b]:].any()
    assert al.flens == [len(a) for a in want_f2p]
    x = torch.from_numpy(rng.randn(B, N, 40).astype(np.float32)).cuda()
    got, flens = _expand_rows(x, al, stride=stride)
    want, wlens = _expand_rows(x, want_f2p, stride=stride)      # the host (list of lists) path = the reference's gather
    assert flens == wlens and torch.equal(got, want)
    x3 = torch.from_numpy(rng.randn(B, N, 7).astype(np.float32)).cuda()  # C not a multiple of 4: scalar copy path
    assert torch.equal(_expand_rows(x3, al, stride=stride)[0], _expand_rows(x3, want_f2p, stride=stride)[0])


def test_cond_input_launch_gives_the_bits_of_the_elementwise_graph(monkeypatch):
    """ttsc_cond_input (round 6): voiced flag, pitch, row expansion, pitch feature and the GEMM's zero columns of Languasito2's conditioning input in ONE launch —
    the conditioning and y_pitch of a sentence and of a ragged batch must equal, bit for bit, what the nine elementwise launches of the reference's graph give
    (TTSC_COND_INPUT_FUSED=0)."""
    from ttscube_amd.networks import modules as MD
    net = MD.Languasito2(30, 2, 250, 8)
    net.load_state_dict(M.fill_state_dict(M.named_shapes(net), 78), strict=True)
    net = net.cuda().eval()
    rng = np.random.RandomState(3)
    lens = [17, 5, 11]
    x = np.zeros((3, 17), dtype=np.int64)
    for b, n in enumerate(lens):
        x[b, :n] = rng.randint(1, 31, size=n)
    spk = torch.tensor([[1], [2], [1]])
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(MD, 'COND_INPUT_FUSED', fused)
        Xb = {'x_char': torch.from_numpy(x), 'x_speaker': spk}
        Xs = {'x_char': torch.from_numpy(x[:1]), 'x_speaker': spk[:1]}
        outs[fused] = (net.inference(Xb).clone(), Xb['y_pitch'].clone(), net.inference(Xs).clone(), Xs['y_pitch'].clone())
    for a, b in zip(outs[True], outs[False]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert float(outs[True][1].abs().max()) > 0      # (voiced frames exist: the pitch path is exercised)


# ---- the AR decoder (csrc/melar.hip) against a float64 restatement over long horizons -----------------------------------------------
class _Enc:
    phon2int = {str(i): i for i in range(40)}
    speaker2int = {str(i): i for i in range(2)}
    max_pitch = 200
    max_duration = 9


def _ar_reference(sd, h, masks, steps, pframes):
    """oracle.meldecoder_ref.textcoder_ar_decode in float64 and in float32 -> (y64 [B, S, O], bound [S]).  The bound of a step is
    4 x the largest fp32-vs-float64 deviation of a valid row up to that step + 1e-6: what fp32 arithmetic alone costs over the horizon.
    Measured at S = 300 (B = 5 / 2, pframes 3 / 1): the fp32 deviation stays between 1e-7 and 3e-7 at every step on the CPUs tried
    (the envelope at step 300: 2.4e-7 / 1.8e-7 on one, 3.0e-7 / 2.4e-7 on another); it does not grow with the horizon.  The kernel's
    error at S = 300 was 5e-7 to 7.3e-7 at every split factor."""
    B, S = h.shape[:2]
    with torch.no_grad():
        y32 = M.textcoder_ar_decode(sd, h, masks, steps, pframes).reshape(B, S, -1).double()
        sd64 = {k: v.double() for k, v in sd.items()}
        y64 = M.textcoder_ar_decode(sd64, h.double(), masks.double(), steps, pframes).reshape(B, S, -1)
    return y64.numpy(), 4.0 * np.maximum.accumulate((y32 - y64).abs().amax(dim=(0, 2)).numpy()) + 1e-6


def _check_ar(y, y64, bound, steps, what):
    """every valid row of every step within the step's bound; every row past an utterance's steps exactly 0.0"""
    B, S = y.shape[:2]
    n = np.full(B, S) if steps is None else np.asarray(steps)
    valid = np.arange(S)[None, :] < n[:, None]                              # [B, S]
    err = np.where(valid, np.abs(y - y64).max(axis=2), 0.0).max(axis=0)      # [S]
    bad = np.flatnonzero(err > bound)
    assert not len(bad), '%s: step %d error %.3g > bound %.3g (worst step %d: %.3g)' % (
        what, bad[0], err[bad[0]], bound[bad[0]], int(np.argmax(err / bound)), float(err.max()))
    assert not np.any(y[~valid]), '%s: non-zero rows past steps[b]' % what
    return float(err.max())


def _philox_masks(seed, S, B, P=256):
    """The masks the kernel draws in Philox mode: bit (r[unit & 3] & 1) of philox4x32-10(counter (unit >> 2, t, b, layer), key seed)."""
    import ctypes as C
    from oracle import wavernn_ref as O
    L = O.lib()
    r = (C.c_uint32 * 4)()
    out = np.zeros((S, 2, B, P), dtype=np.float32)
    for t in range(S):
        for layer in range(2):
            for b in range(B):
                for q in range(P // 4):
                    L.wr_philox(q, t, b, layer, seed & 0xffffffff, seed >> 32, r)
                    out[t, layer, b, 4 * q:4 * q + 4] = [v & 1 for v in r]
    return torch.from_numpy(out)


def _ar_net(pframes, seed):
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    net = CubenetTextcoder(_Enc(), pframes=pframes)
    sd = M.fill_state_dict(M.named_shapes(net), seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _decode(net, h, masks, steps, seed=None):
    """the kernel's output [B, S, O] written into a NaN-filled buffer (so that a row the kernel skips cannot pass as zero)"""
    B, S = h.shape[:2]
    out = torch.full((B, S, 80 * net._pframes), float('nan'), device='cuda')
    with torch.no_grad():
        net._ar_decode(h.cuda(), None if masks is None else masks.cuda(), steps=steps, seed=seed, out=out)
    return out.cpu().numpy()


@pytest.mark.parametrize('pframes,B,S,steps,philox', [
    (3, 1, 1, None, False), (3, 2, 2, [2, 1], True), (3, 5, 64, [64, 0, 1, 33, 64], True), (3, 5, 300, [300, 1, 0, 300, 157], False),
    (1, 2, 300, [300, 0], False), (1, 5, 64, [0, 64, 1, 64, 20], True),
])
def test_ar_decoder_sweep_against_float64(pframes, B, S, steps, philox, monkeypatch):
    """ttsc_melar_decode at split factor G = 1 (melar_kernel), 2, 4 and 8 (melar_split_kernel), injected masks:
    (1) every step of every valid row within the fp32 bound of the float64 loop, (2) rows past steps[b] exactly 0.0, (3) each utterance
    of the batch bit-identical to its solo decode at the same G, (5) no hand-off of the split launches timed out; and (4) in Philox
    mode the output is bit-identical to the same kernel fed the masks rebuilt on the host (counter (unit >> 2, t, b, layer), key seed):
    every split member must draw the same PreNet masks."""
    from ttscube_amd import _lib
    net, sd = _ar_net(pframes, 90 + pframes)
    rng = np.random.RandomState(B * 1000 + S + pframes)
    h = torch.from_numpy(rng.uniform(-1, 1, size=(B, S, 1024)).astype(np.float32))
    masks = torch.from_numpy((rng.uniform(size=(S, 2, B, 256)) > 0.5).astype(np.float32))
    y64, bound = _ar_reference(sd, h, masks, steps, pframes)
    seed = 0x5EED0000ABCD1234
    pm = _philox_masks(seed, S, B) if philox else None
    for G in (1, 2, 4, 8):
        monkeypatch.setenv('TTSC_MELAR_SPLIT', str(G))
        y = _decode(net, h, masks, steps)
        _check_ar(y, y64, bound, steps, 'G=%d' % G)
        for b in range(B):
            solo = _decode(net, h[b:b + 1], masks[:, :, b:b + 1], None if steps is None else [steps[b]])
            assert np.array_equal(solo[0], y[b]), 'G=%d: utterance %d of the batch != its solo decode' % (G, b)
        if philox:
            yp = _decode(net, h, None, steps, seed=seed)
            ym = _decode(net, h, pm, steps)
            assert np.array_equal(yp, ym), 'G=%d: in-kernel Philox masks != host-rebuilt masks (first step %s)' % (
                G, np.argwhere(yp != ym)[:1, 1])
        assert _lib.lib().ttsc_melar_split_status() == 0, 'G=%d: a split hand-off timed out' % G


def test_ar_decoder_crosses_to_the_single_workgroup_kernel(monkeypatch):
    """B = 130 without TTSC_MELAR_SPLIT: 2 x 130 workgroups exceed the chip's 256 CUs, so the dispatcher picks melar_kernel — its
    output is bit-identical to TTSC_MELAR_SPLIT=1 and within the float64 bound (ragged steps, 0 / 1 / S included)."""
    from ttscube_amd import _lib
    net, sd = _ar_net(3, 95)
    B, S = 130, 32
    rng = np.random.RandomState(130)
    h = torch.from_numpy(rng.uniform(-1, 1, size=(B, S, 1024)).astype(np.float32))
    masks = torch.from_numpy((rng.uniform(size=(S, 2, B, 256)) > 0.5).astype(np.float32))
    steps = [int(v) for v in rng.randint(0, S + 1, size=B)]
    steps[:3] = [0, 1, S]
    y64, bound = _ar_reference(sd, h, masks, steps, 3)
    monkeypatch.delenv('TTSC_MELAR_SPLIT', raising=False)
    y = _decode(net, h, masks, steps)
    _check_ar(y, y64, bound, steps, 'B=130 default')
    monkeypatch.setenv('TTSC_MELAR_SPLIT', '1')
    assert np.array_equal(_decode(net, h, masks, steps), y)
    assert _lib.lib().ttsc_melar_split_status() == 0


def _overlay_states(net, X):
    from ttscube_amd.networks.modules import _expand_rows
    with torch.no_grad():
        h, out_dur = net._text_stack(X['x_char'].cuda(), X['x_speaker'].cuda(), None)
        durs = torch.argmax(out_dur, dim=-1).cpu().numpy().reshape(-1)
        f2p = [p for p, d in enumerate(durs) for _ in range(int(d))]
        h, _ = _expand_rows(h, [f2p], stride=net._pframes)
        return net._lstm('_rnn_overlay')(h)


@pytest.mark.parametrize('name', ['textcoder_long', 'textcoder_pf1'])
def test_textcoder_long_matches_reference_golden(golden_dir, name, monkeypatch):
    """The reference's own AR run (tools/gen_golden_meldecoder.py, masks replayed): ~100 steps of three frames / 300 steps of one
    frame.  Every AR step of the kernel (pre-postnet rows, default split and G = 1) is within 4 x the fp32 drift of the whole
    pipeline (oracle in float32 vs float64, envelope up to that step) + 1e-6 of the reference; the post-net mel within 1e-4 RMS."""
    from tests.test_oracle_meldecoder import textcoder_pipeline_bound
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    z, shapes, sd = _load(golden_dir, name)
    pf = int(z['pframes'])

    class Enc(_Enc):
        max_duration = int(z['max_duration'])

    net = CubenetTextcoder(Enc(), pframes=pf)
    assert M.named_shapes(net) == shapes
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    X = {'x_char': torch.from_numpy(z['x_char']), 'x_speaker': torch.from_numpy(z['x_speaker'])}
    mk = torch.from_numpy(z['masks']).unsqueeze(2)                          # [S, 2, 1, 256]
    ref = z['mel_ar'].astype(np.float64)                                    # [1, S, O]
    S = ref.shape[1]
    bound = textcoder_pipeline_bound(sd, X, mk, pf, S)
    h = _overlay_states(net, X)
    assert h.shape[1] == S
    for G in (None, 1):
        if G is None:
            monkeypatch.delenv('TTSC_MELAR_SPLIT', raising=False)
        else:
            monkeypatch.setenv('TTSC_MELAR_SPLIT', str(G))
        y = _decode(net, h.cpu(), mk, None)
        err = np.abs(y - ref).max(axis=(0, 2))
        bad = np.flatnonzero(err > bound)
        assert not len(bad), 'G=%s: step %d of %d error %.3g > bound %.3g' % (G, bad[0], S, err[bad[0]], bound[bad[0]])
    mel = net.inference(dict(X), dropout_masks=mk).cpu()
    assert mel.shape == z['mel'].shape
    assert float((mel - torch.from_numpy(z['mel'])).pow(2).mean().sqrt()) < 1e-4
