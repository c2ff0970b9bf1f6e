"""GPU parity of the ragged WaveRNN decode (``ttsc_wavernn_decode_ragged`` through ``WaveRNN.decode(lengths=...)``): every row of a
ragged batch equals, bit for bit, the C oracle's decode of that row's valid prefix ALONE (its own T / Tl, its own seed, standing at
batch position ``stream``), under both decode kernels; nothing is stored beyond a row's length; the padding holds NaN."""
import numpy as np
import pytest
import torch

from oracle import wavernn_ref as O

pytestmark = pytest.mark.gpu

OMODE = {'noise': O.MODE_NOISE, 'philox': O.MODE_PHILOX, 'argmax': O.MODE_ARGMAX}
FRAMES11 = [1, 3, 2, 1, 4, 4, 2, 3, 1, 2, 4]


@pytest.fixture(params=['tile', 'stream'])
def wr_kernel(request, monkeypatch):
    """Run the test twice: with the multi-workgroup tile kernel allowed (its default) and with the single-workgroup streaming kernel
    forced (TTSC_WR_TILE=0) — both must be bit-exact."""
    if request.param == 'tile':
        monkeypatch.delenv('TTSC_WR_TILE', raising=False)
    else:
        monkeypatch.setenv('TTSC_WR_TILE', '0')
    monkeypatch.delenv('TTSC_WR_BT', raising=False)
    return request.param


def _net(H, N, lowres, sd, output='mulaw'):
    from ttscube_amd.networks.modules import WaveRNN
    net = WaveRNN(num_layers=N, layer_size=H, upsample=240 if lowres else 24, upsample_low=10, use_lowres=lowres, output=output)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.cuda().eval()


def _noise(output, B, L, seed):
    """injected sampler noise [B, L, W] in the layout of include/ttscube_math.h (Gumbel terms; MOL: 10 Gumbel + 1 logistic; Beta: per
    gamma variate one uniform and four (normal, uniform) rounds)"""
    rng = np.random.RandomState(seed)
    W = O.NOISE_WIDTH[output]
    u = rng.uniform(1e-6, 1 - 1e-6, size=(B, L, W))
    if output in ('mulaw', 'raw'):
        return (-np.log(-np.log(u))).astype(np.float32)
    if output == 'mol':
        nz = -np.log(-np.log(u))
        nz[..., 10] = np.log(u[..., 10]) - np.log(1 - u[..., 10])
        return nz.astype(np.float32)
    assert output == 'beta'
    nz = u.copy()
    for v in range(2):
        for i in range(4):
            nz[..., v * 9 + 1 + 2 * i] = rng.randn(B, L)
    return nz.astype(np.float32)


_ORACLE = {}   # one oracle run per case, shared by the two kernel variants (and never modified)


def _problem(key, H, N, lowres, output, frames, low_len, mode, seeds, streams):
    """inputs with NaN padding + the oracle's alone-run of every row"""
    if key in _ORACLE:
        return _ORACLE[key]
    B, T = len(frames), max(frames)
    up = 240 if lowres else 24
    sd = O.synthetic_state_dict(H=H, num_layers=N, use_lowres=lowres, seed=900 + H + N, S=O.SAMPLE_SIZE[output])
    mel, x_low = O.synthetic_inputs(B, T, seed=31 + B, upsample=up)
    Tl = x_low.shape[1] if lowres else 0
    L = min(T * up, Tl * 10) if lowres else T * up
    Lb = [min(frames[b] * up, low_len[b] * 10) if lowres else frames[b] * up for b in range(B)]
    noise = _noise(output, B, L, seed=17) if mode == 'noise' else None
    rows = []
    for b in range(B):
        ridx, rwav, rlog = O.decode(sd, mel[b:b + 1, :frames[b]], x_low[b:b + 1, :low_len[b]] if lowres else None, num_layers=N, H=H,
                                    use_lowres=lowres, upsample=up, output=output, mode=OMODE[mode],
                                    noise=noise[b:b + 1, :Lb[b]] if noise is not None else None, seed=seeds[b], b_offset=streams[b],
                                    want_logits=True)
        assert ridx.shape == (1, Lb[b])
        rows.append((ridx[0], rwav[0], rlog[0]))
    # everything beyond a row's own lengths is NaN: no such element may reach an output
    mel = mel.copy()
    for b in range(B):
        mel[b, frames[b]:] = np.nan
        if lowres:
            x_low[b, low_len[b]:] = np.nan
        if noise is not None:
            noise[b, Lb[b]:] = np.nan
    _ORACLE[key] = (sd, mel, x_low if lowres else None, noise, L, Lb, rows)
    return _ORACLE[key]


def _check(key, H, N, lowres, output, frames, low_len, mode, want_kernel, seeds=None, streams=None):
    B = len(frames)
    rng = np.random.RandomState(B + H)
    seeds = seeds if seeds is not None else [int(s) * 0x100000001 + b for b, s in enumerate(rng.randint(1, 2 ** 31, size=B))]
    streams = streams if streams is not None else [int(s) for s in rng.randint(0, 20, size=B)]
    sd, mel, x_low, noise, L, Lb, rows = _problem(key, H, N, lowres, output, frames, low_len, mode, seeds, streams)
    net = _net(H, N, lowres, sd, output)
    X = {'mel': torch.from_numpy(mel)}
    if lowres:
        X['x_low'] = torch.from_numpy(x_low)
    idx, wav, logits, out_len = net.decode(X, mode=mode, noise=noise, seed=5, want_logits=True, lengths=frames,
                                           low_lengths=low_len if lowres else None, seeds=seeds, streams=streams)
    assert net.last_kernel == want_kernel
    assert out_len == Lb and idx.shape == (B, L) and logits.shape == (B, L, O.SAMPLE_SIZE[output])
    idx, wav, logits = idx.cpu().numpy(), wav.cpu().numpy(), logits.cpu().numpy()
    for b in range(B):
        ridx, rwav, rlog = rows[b]
        n = Lb[b]
        bad = np.argwhere(idx[b, :n] != ridx)
        assert not len(bad), 'row %d (frames %d): first index mismatch at step %d' % (b, frames[b], bad[0, 0])
        assert np.array_equal(wav[b, :n], rwav), 'row %d: samples' % b
        assert np.array_equal(logits[b, :n], rlog), 'row %d: logits' % b
        assert not idx[b, n:].any() and not wav[b, n:].any() and not logits[b, n:].any(), 'row %d: stores beyond L_b' % b


def _want(wr_kernel, N=1):
    return 'tile' if (wr_kernel == 'tile' and N <= 2) else 'stream'


# ---- 1. rows against the oracle run alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['noise', 'philox', 'argmax'])
def test_rows_equal_oracle_alone(mode, wr_kernel):
    fr = FRAMES11
    _check(('hr64', mode), 64, 1, True, 'mulaw', fr, [24 * f for f in fr], mode, _want(wr_kernel))


@pytest.mark.parametrize('mode', ['noise', 'philox'])
def test_length_from_the_low_resolution_side(mode, wr_kernel):
    """two rows whose x_low ends before 24 * frames: L_b comes from low_len, and the convolutions' end padding and the interpolation's
    end clamp sit inside the (NaN-filled) buffer"""
    fr = FRAMES11
    ll = [24 * f for f in fr]
    ll[1], ll[4] = 24 * 3 - 7, 24 * 4 - 30
    _check(('hr64low', mode), 64, 1, True, 'mulaw', fr, ll, mode, _want(wr_kernel))


@pytest.mark.parametrize('mode', ['noise', 'philox', 'argmax'])
def test_low_resolution_net(mode, wr_kernel):
    _check(('lr64', mode), 64, 1, False, 'mulaw', FRAMES11, None, mode, _want(wr_kernel))


@pytest.mark.parametrize('mode', ['noise', 'philox'])
def test_two_layers(mode, wr_kernel):
    fr = FRAMES11
    _check(('hr64n2', mode), 64, 2, True, 'mulaw', fr, [24 * f for f in fr], mode, _want(wr_kernel, 2))


@pytest.mark.parametrize('mode', ['noise', 'philox'])
def test_h512(mode, wr_kernel):
    fr = [1, 2, 2, 1, 1, 2, 1, 2, 1]
    _check(('hr512', mode), 512, 1, True, 'mulaw', fr, [24 * f for f in fr], mode, _want(wr_kernel))


@pytest.mark.parametrize('bt', [2, 4, 8])
def test_streaming_kernel_utterance_tiles(bt, monkeypatch):
    """wr_decode_kernel<2/4/8, ragged>: B = 11 is no multiple of the tile; a workgroup steps to the longest of ITS rows"""
    monkeypatch.setenv('TTSC_WR_TILE', '0')
    monkeypatch.setenv('TTSC_WR_BT', str(bt))
    fr = FRAMES11
    _check(('hr64', 'philox'), 64, 1, True, 'mulaw', fr, [24 * f for f in fr], 'philox', 'stream')


# ---- 2. per-group bounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['philox', 'noise'])
def test_per_group_bounds(mode, wr_kernel):
    """a whole tile of eight rows shorter than its neighbour, and a last tile of one row"""
    fr = [1] * 8 + [3] * 8 + [2]
    _check(('groups', mode), 64, 1, True, 'mulaw', fr, [24 * f for f in fr], mode, _want(wr_kernel))


# ---- 3. dense stays dense -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lowres,N', [(True, 1), (False, 1), (True, 2)])
def test_full_lengths_equal_the_dense_call(lowres, N, wr_kernel):
    B, T = 11, 2
    sd = O.synthetic_state_dict(H=64, num_layers=N, use_lowres=lowres, seed=41)
    net = _net(64, N, lowres, sd)
    mel, x_low = O.synthetic_inputs(B, T, seed=2, upsample=240 if lowres else 24)
    X = {'mel': torch.from_numpy(mel)}
    if lowres:
        X['x_low'] = torch.from_numpy(x_low)
    for mode in ('philox', 'argmax'):
        a = net.decode(X, mode=mode, seed=0xD15EA5E, want_logits=True)
        assert net.last_kernel == _want(wr_kernel, N)
        b = net.decode(X, mode=mode, seed=1, want_logits=True, lengths=[T] * B, low_lengths=[24 * T] * B if lowres else None,
                       seeds=[0xD15EA5E] * B, streams=list(range(B)))
        assert net.last_kernel == _want(wr_kernel, N)
        assert b[3] == [T * (240 if lowres else 24)] * B
        for x, y in zip(a, b[:3]):
            assert torch.equal(x, y)
        # ... and the tables default to the launch seed and the row index
        c = net.decode(X, mode=mode, seed=0xD15EA5E, want_logits=True, lengths=[T] * B, low_lengths=[24 * T] * B if lowres else None)
        for x, y in zip(a, c[:3]):
            assert torch.equal(x, y)


# ---- 4. continuous heads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('output', ['mol', 'beta'])
@pytest.mark.parametrize('mode', ['philox', 'noise'])
def test_continuous_heads(output, mode, wr_kernel):
    fr = FRAMES11
    _check(('cont', output, mode), 64, 1, True, output, fr, [24 * f for f in fr], mode, _want(wr_kernel))


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------
def test_bad_tables_raise_before_any_launch(wr_kernel):
    from ttscube_amd._lib import TTSCError
    B, T = 3, 2
    sd = O.synthetic_state_dict(H=64, num_layers=1, use_lowres=True, seed=41)
    net = _net(64, 1, True, sd)
    mel, x_low = O.synthetic_inputs(B, T, seed=2)
    X = {'mel': torch.from_numpy(mel), 'x_low': torch.from_numpy(x_low)}
    good = dict(lengths=[1, 2, 2], low_lengths=[24, 48, 40])
    net.last_kernel = None
    for bad in (dict(lengths=[1, 0, 2]), dict(low_lengths=[24, 48, 0]), dict(lengths=[1, 3, 2]), dict(low_lengths=[24, 49, 40]),
                dict(low_lengths=None), dict(lengths=[1, 2]), dict(low_lengths=[24, 48, 40, 40]), dict(seeds=[1, 2]),
                dict(streams=[0, 1, 2, 3])):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(TTSCError):
            net.decode(X, mode='argmax', **kw)
        assert net.last_kernel is None   # no launch was recorded
    with pytest.raises(TTSCError):
        net.decode(X, mode='argmax', seeds=[1, 2, 3])   # tables without lengths
    lr = _net(64, 1, False, O.synthetic_state_dict(H=64, num_layers=1, use_lowres=False, seed=42))
    with pytest.raises(TTSCError):
        lr.decode({'mel': torch.from_numpy(mel)}, mode='argmax', lengths=[1, 2, 0])
    out = net.decode(X, mode='argmax', **good)
    assert out[3] == [240, 480, 400]
