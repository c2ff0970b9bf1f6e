"""GPU: exact ties of the categorical Gumbel-max through the real decode kernels.

The arg-max over the 256 classes exists three times — the oracle's sequential scan (oracle/wavernn_ref.c), the streaming kernel's strided
per-lane scan + 64-lane butterfly (wavernn.hip) and the tile kernel's three levels: 4 classes per lane, 8 lanes per member, 8 members
(wavernn_tile.hip) — and all three promise "first maximum wins".  With random noise an exact tie never happens, so here the output layer is
zeroed (every logit is exactly 0, the score IS the injected noise) and the noise carries an exact maximum on a chosen set of classes."""
import numpy as np
import pytest
import torch

from oracle import wavernn_ref as O

pytestmark = pytest.mark.gpu

H, B, T, UP = 64, 3, 3, 24          # B = 3: a tile of 8 with idle rows; 3 mel frames x 24 = 72 steps, one launch
L = T * UP
TOP = 3.0
# the classes that share the exact maximum, cycled over the steps of every row (None: the signed-zero case below)
TIE_SETS = [
    (1, 2),                          # one lane's four classes in the tile kernel
    (1, 30),                         # two lanes of one member
    (31, 32), (5, 250),              # across members
    (10, 74),                        # the same lane on different trips of the streaming scan
    (10, 11),                        # neighbouring lanes of the streaming scan
    (7, 8, 200),
    (0, 255),
    tuple(range(256)),               # all equal
    None,                            # maxima +0.0 on the higher class (130) and -0.0 on the lower (20), everything else negative
]


@pytest.fixture(params=['tile', 'stream'])
def wr_kernel(request, monkeypatch):
    """the multi-workgroup tile kernel (the default at these sizes) or the single-workgroup streaming kernel (TTSC_WR_TILE=0)"""
    if request.param == 'tile':
        monkeypatch.delenv('TTSC_WR_TILE', raising=False)
    else:
        monkeypatch.setenv('TTSC_WR_TILE', '0')
    return request.param


def _net(N, sd, output):
    from ttscube_amd.networks.modules import WaveRNN
    net = WaveRNN(num_layers=N, layer_size=H, upsample=UP, upsample_low=10, use_lowres=False, output=output)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.cuda().eval()


def _state_dict(N, bias):
    sd = O.synthetic_state_dict(H=H, num_layers=N, use_lowres=False, seed=77 + N)
    sd['_output.linear_layer.weight'] = np.zeros_like(sd['_output.linear_layer.weight'])
    sd['_output.linear_layer.bias'] = np.asarray(bias, dtype=np.float32)
    return sd


def _tie_noise():
    """noise [B, L, 256] and the class every step must pick"""
    s = np.arange(256)
    noise = np.empty((B, L, 256), dtype=np.float32)
    want = np.empty((B, L), dtype=np.uint8)
    for b in range(B):
        for t in range(L):
            g = -(1.0 + ((s * 7 + t * 3 + b * 5) % 50))          # negative integers: exact, and never the maximum
            tie = TIE_SETS[(t + 4 * b) % len(TIE_SETS)]
            if tie is None:
                g[20], g[130], low = -0.0, 0.0, 20
            else:
                g[list(tie)], low = TOP, min(tie)
            noise[b, t], want[b, t] = g, low
    return noise, want


@pytest.mark.parametrize('output', ['mulaw', 'raw'])
@pytest.mark.parametrize('N', [1, 2])
def test_exact_ties_pick_the_lowest_class(N, output, wr_kernel):
    sd = _state_dict(N, np.zeros(256))
    net = _net(N, sd, output)
    mel, _ = O.synthetic_inputs(B, T, seed=5, upsample=UP)
    noise, want = _tie_noise()
    assert {tuple(np.flatnonzero(noise[b, t] == noise[b, t].max())) for b in range(B) for t in range(L)} >= {c for c in TIE_SETS if c}
    ridx, rwav, rlog = O.decode(sd, mel, None, num_layers=N, H=H, use_lowres=False, upsample=UP, output=output, mode=O.MODE_NOISE,
                                noise=noise, want_logits=True)
    assert not rlog.any() and np.array_equal(ridx, want)          # every logit is exactly 0; the oracle's scan takes the first maximum
    idx, wav, logits = net.decode({'mel': torch.from_numpy(mel)}, mode='noise', noise=noise, want_logits=True)
    assert net.last_kernel == wr_kernel
    idx = idx.cpu().numpy()
    bad = np.argwhere(idx != want)
    assert bad.size == 0, 'tie resolved to another class at (row, step) %s: got %s, lowest of the set is %s' % (
        bad[:4].tolist(), idx[idx != want][:4].tolist(), want[idx != want][:4].tolist())
    assert np.array_equal(idx, ridx)
    assert np.array_equal(wav.cpu().numpy().view(np.uint32), rwav.view(np.uint32))
    assert np.array_equal(logits.cpu().numpy().view(np.uint32), rlog.view(np.uint32))


def test_argmax_mode_ties(wr_kernel):
    """no noise at all: a bias with two equal maxima gives the lower class, an all-equal bias gives class 0"""
    mel, _ = O.synthetic_inputs(B, T, seed=6, upsample=UP)
    two = np.full(256, -1.0)
    two[[40, 41]] = 2.0
    for bias, cls in ((two, 40), (np.full(256, 0.5), 0)):
        sd = _state_dict(1, bias)
        net = _net(1, sd, 'mulaw')
        ridx, rwav, _ = O.decode(sd, mel, None, num_layers=1, H=H, use_lowres=False, upsample=UP, mode=O.MODE_ARGMAX)
        idx, wav, _ = net.decode({'mel': torch.from_numpy(mel)}, mode='argmax')
        assert net.last_kernel == wr_kernel
        assert (ridx == cls).all() and (idx.cpu().numpy() == cls).all()
        assert np.array_equal(wav.cpu().numpy(), rwav)
