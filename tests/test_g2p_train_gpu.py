"""GPU: G2P training (networks/g2p_train.py, csrc/g2p_train.hip).

  * the decoder kernels against the float64 formulation of tests/g2p_train_reference.py with injected masks (logits <= 1e-5, d enc and every
    decoder / attention / output gradient <= 1e-4 relative, the same bits twice);
  * loss edge cases (an all-PAD word, all targets PAD, a label outside the table);
  * words do not see each other (B = 3 launch against B = 1 launches, bit for bit);
  * the encoder's inter-layer dropout against float64 torch, and dropout 0 giving the bits it gave before;
  * the Philox path (all three mask families: the attention and decoder masks rebuilt on the host from the documented counters and injected give
    the Philox run's bits, the encoder's mask read from its zeros; another seed another mask; the kept fractions);
  * reference parity (tests/golden/g2p_train_{a,b}.npz, made by the reference itself): logits, loss, gradient fingerprints, parameters after two steps;
  * the learn_batch surface, and the trainer script end to end.
Gates: the project's gates for training tests (test_textcoder_train_gpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import meldecoder_ref as M
from oracle.fingerprint import compare
from tests import g2p_train_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _net(G, L, Em, H, D, seed):
    """a Seq2Seq of the given sizes (attention width = D, as the constructor wires it) with seeded weights, on the GPU in train mode"""
    from ttscube_amd.networks.seq2seq import Seq2Seq
    net = Seq2Seq(G, L, embedding_size=Em, encoder_size=H, decoder_size=D)
    net.load_state_dict(M.fill_state_dict(M.named_shapes(net), seed), strict=True)
    return net.cuda().train()


def _dec_masks(B, N, T, A, D, gen):
    return {'init': (torch.rand(B, 1, D, generator=gen) > 0.33).float(), 'att': [(torch.rand(B, N, A, generator=gen) > 0.1).float() for _ in range(T)],
            'dec': [(torch.rand(B, 1, D, generator=gen) > 0.33).float() for _ in range(T)]}


DEC_KEYS = ['attention.attn.conv.weight', 'attention.attn.conv.bias', 'attention.v', 'output_emb.weight', 'output.weight', 'output.bias'] + \
           ['decoder.%s_l%d' % (n, l) for l in (0, 1) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


# (B, N, T, L), (Em, H, D = A): one position / start step plus one step; L % 4 != 0 with PAD rows inside the teacher feed; the reference's sizes;
# N beyond the LDS-resident cap of g2p.hip (the training kernels keep no such cap: they read the encoder rows from global memory at every N)
@pytest.mark.parametrize('B,N,T,L,Em,H,D', [(1, 1, 1, 5, 4, 4, 8), (3, 5, 4, 7, 4, 4, 8), (2, 6, 3, 45, 100, 200, 200), (2, 30, 2, 45, 100, 200, 200)])
def test_decoder_kernels_match_float64(B, N, T, L, Em, H, D):
    from ttscube_amd.networks.g2p_train import decoder_forward_train
    gen = torch.Generator().manual_seed(B * 100 + N)
    net = _net(9, L, Em, H, D, 5)
    enc = torch.randn(B, N, 2 * H, generator=gen) * 0.5
    y = torch.randint(1, L, (B, T), generator=gen)
    if B > 1 and T > 2:
        y[1, 1:] = 0                       # ragged: PAD labels inside the teacher feed
        y[B - 1, T - 1] = 0
    masks = _dec_masks(B, N, T, D, D, gen)
    w = torch.randn(B, T, L, generator=gen)
    runs = []
    for _ in range(2):
        net.zero_grad()
        e = enc.cuda().requires_grad_(True)
        lg = decoder_forward_train(net, e, y.cuda(), masks)
        (lg * w.cuda()).sum().backward()
        runs.append([lg.detach().cpu(), e.grad.cpu()] + [dict(net.named_parameters())[k].grad.cpu().clone() for k in DEC_KEYS])
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)           # fixed-order accumulation: the same bits twice
    P = R.leaves(net.state_dict())
    e64 = enc.double().requires_grad_(True)
    lr = R.decoder_reference(P, e64, y, masks)
    (lr * w.double()).sum().backward()
    assert _rel(runs[0][0], lr.detach()) <= 1e-5
    assert _rel(runs[0][1], e64.grad) <= 1e-4
    for k, got in zip(DEC_KEYS, runs[0][2:]):
        want = P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])      # (T = 1 feeds no embedding back: autograd leaves None)
        assert _rel(got, want) <= 1e-4, k
    assert float(runs[0][2 + DEC_KEYS.index('output_emb.weight')][0].abs().max()) == 0.0     # the PAD row gets no gradient


def test_loss_edge_cases_and_bad_labels():
    from ttscube_amd import _lib
    from ttscube_amd.networks.g2p_train import g2p_loss, seq2seq_forward_train
    from ttscube_amd.networks.seq2seq import check_status
    gen = torch.Generator().manual_seed(4)
    net = _net(9, 7, 4, 4, 8, 6)
    net.eval()                             # no dropout: the comparison below is about the loss
    x = torch.randint(1, 9, (3, 5), generator=gen).cuda()
    y = torch.randint(1, 7, (3, 4), generator=gen)
    y[1, :] = 0                            # a word whose labels are all PAD
    P = R.leaves(net.state_dict())
    lr = R.loss_reference(R.seq2seq_reference(P, x.cpu(), y), y)
    lr.backward()
    loss = g2p_loss(seq2seq_forward_train(net, x, y.cuda()), y.cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(lr.detach())) <= 1e-5 * max(1.0, abs(float(lr.detach())))
    for k, p in net.named_parameters():
        assert _rel(p.grad.cpu(), P[k].grad) <= 1e-4, k
    # the all-PAD word alone: loss 0 (ttsc_masked_ce's convention) and zero gradients everywhere
    net.zero_grad()
    y0 = torch.zeros(1, 4, dtype=torch.long).cuda()
    loss = g2p_loss(seq2seq_forward_train(net, x[1:2], y0), y0)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in net.parameters())
    # a label outside the table: zeros are fed, the status word raises, and the process goes on
    bad = y.clone()
    bad[0, 1] = 7
    seq2seq_forward_train(net, x, bad.cuda())
    with pytest.raises(_lib.TTSCError, match='label'):
        check_status('test')
    seq2seq_forward_train(net, x, y.cuda())
    check_status('test')


def test_words_do_not_see_each_other():
    from ttscube_amd.networks.g2p_train import G2pDecoderFn, _decoder_masks
    gen = torch.Generator().manual_seed(8)
    B, N, T, L, Em, H, D = 3, 6, 3, 45, 100, 200, 200
    net = _net(9, L, Em, H, D, 7)
    enc = (torch.randn(B, N, 2 * H, generator=gen) * 0.5).cuda()
    y = torch.randint(1, L, (B, T), generator=gen).to(torch.int32).cuda()
    masks = _dec_masks(B, N, T, D, D, gen)
    dh2 = torch.randn(B, T, D, generator=gen).cuda()
    seen = {}
    import ttscube_amd.networks.g2p_train as GT
    orig = GT.gemm_hip

    def run(sl):
        """launch words `sl`; keep the kernels' own outputs: d enc before the projection's share, d pe and the per-step rows"""
        m = {'init': masks['init'][sl], 'att': [a[sl] for a in masks['att']], 'dec': [a[sl] for a in masks['dec']]}
        n = enc[sl].shape[0]
        am, dm = _decoder_masks(m, n, T, enc.device)
        e = enc[sl].clone().requires_grad_(True)
        d = net.decoder
        rows = []

        def spy(a, b, *args, **kw):
            rows.append(a.detach().clone())          # the left operands: gate-gradient rows, d q rows, d pe
            if kw.get('accumulate'):
                seen['denc'] = kw['out'].detach().clone()
            return orig(a, b, *args, **kw)
        GT.gemm_hip = spy
        try:
            h2 = G2pDecoderFn.apply(e, y[sl].contiguous(), am, dm, 0, 0.1, 0.33, net.attention.attn.conv.weight, net.attention.attn.conv.bias,
                                    net.attention.v, net.output_emb.weight, d.weight_ih_l0, d.weight_hh_l0, d.bias_ih_l0, d.bias_hh_l0, d.weight_ih_l1,
                                    d.weight_hh_l1, d.bias_ih_l1, d.bias_hh_l1)
            h2.backward(dh2[sl].contiguous())
        finally:
            GT.gemm_hip = orig
        return h2.detach(), seen['denc'], rows

    h_all, denc_all, rows_all = run(slice(0, B))
    for b in range(B):
        h_b, denc_b, rows_b = run(slice(b, b + 1))
        assert torch.equal(h_all[b:b + 1], h_b)
        assert torch.equal(denc_all.reshape(B, -1)[b], denc_b.reshape(-1))
        assert len(rows_b) == len(rows_all)
        for ra, rb in zip(rows_all, rows_b):
            per = ra.shape[0] // B
            assert torch.equal(ra[b * per:(b + 1) * per], rb)


def test_encoder_interlayer_dropout_matches_float64_and_zero_dropout_is_unchanged():
    from ttscube_amd import _lib
    from ttscube_amd.networks.lstm_autograd import lstm_forward_train
    gen = torch.Generator().manual_seed(12)
    m = torch.nn.LSTM(6, 8, 2, dropout=0.33, bidirectional=True, batch_first=True)
    sd = M.fill_state_dict(M.named_shapes(m), 3)
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = torch.randn(3, 5, 6, generator=gen)
    mask = (torch.rand(3, 5, 16, generator=gen) > 0.33).float()
    dy = torch.randn(3, 5, 16, generator=gen)
    xg = x.cuda().requires_grad_(True)
    yk = lstm_forward_train(m, xg, dropout_masks=[mask.cuda()])
    yk.backward(dy.cuda())
    P = R.leaves({'e.' + k: v for k, v in sd.items()})
    x64 = x.double().requires_grad_(True)
    yr = R.bilstm_reference(P, 'e.', x64, 2, [mask], 0.33)
    yr.backward(dy.double())
    assert _rel(yk.detach().cpu(), yr.detach()) <= 1e-5
    assert _rel(xg.grad.cpu(), x64.grad) <= 1e-4
    for k, p in m.named_parameters():
        assert _rel(p.grad.cpu(), P['e.' + k].grad) <= 1e-4, k
    with pytest.raises(_lib.TTSCError, match='dropout'):
        lstm_forward_train(m, xg)          # dropout above 0 and no mask source
    # dropout 0: the new arguments are not looked at, and the bits are those of the call without them
    m.dropout = 0.0
    a = lstm_forward_train(m, x.cuda())
    b = lstm_forward_train(m, x.cuda(), dropout_masks=[mask.cuda()], dropout_seed=5)
    assert torch.equal(a, b)
    m.dropout = 0.33
    m.eval()
    assert torch.equal(a, lstm_forward_train(m, x.cuda()))          # eval mode drops nothing, as torch.nn.LSTM


def test_philox_masks_are_shared_by_both_passes():
    from ttscube_amd.networks.g2p_train import G2pDecoderFn
    from ttscube_amd.networks.lstm_autograd import HipDropoutFn
    gen = torch.Generator().manual_seed(21)
    B, N, T, L, Em, H, D = 4, 6, 5, 45, 100, 200, 200
    net = _net(9, L, Em, H, D, 9)
    enc = (torch.randn(B, N, 2 * H, generator=gen) * 0.5).cuda()
    y = torch.randint(1, L, (B, T), generator=gen).to(torch.int32).cuda()
    dh2 = torch.randn(B, T, D, generator=gen).cuda()
    d = net.decoder

    def run(am, dm, seed):
        e = enc.clone().requires_grad_(True)
        net.zero_grad()
        seen = {}
        h2 = G2pDecoderFn.apply(e, y, am, dm, seed, 0.1, 0.33, net.attention.attn.conv.weight, net.attention.attn.conv.bias, net.attention.v,
                                net.output_emb.weight, d.weight_ih_l0, d.weight_hh_l0, d.bias_ih_l0, d.bias_hh_l0, d.weight_ih_l1, d.weight_hh_l1,
                                d.bias_ih_l1, d.bias_hh_l1)
        saved = dict(zip(sorted(['gates0', 'cells0', 'h1', 'h1m', 'gates1', 'cells1', 'h2', 'aq', 'att']), h2.grad_fn.saved_tensors[13:]))
        h2.backward(dh2)
        return h2.detach(), e.grad.clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None], saved

    h_a, de_a, g_a, sv = run(None, None, 1234)
    # the decoder mask from the forward's zeros (the attention family: test_philox_attention_and_decoder_masks_rebuilt_on_the_host)
    dm = (sv['h1m'] != 0).float()
    keep = float(dm.mean())
    n = dm.numel()
    assert abs(keep - 0.67) <= 5 * np.sqrt(0.33 * 0.67 / n), keep
    h_b, _, _, _ = run(None, None, 1235)
    assert not torch.equal(h_a, h_b)                                   # another seed, another mask
    h_c, de_c, g_c, _ = run(None, None, 1234)
    assert torch.equal(h_a, h_c) and torch.equal(de_a, de_c) and all(torch.equal(p, q) for p, q in zip(g_a, g_c))
    # with the attention dropout off, the run with the recovered decoder mask injected equals the Philox run bit for bit, gradients included:
    # the backward drew the forward's masks
    net.attention.dropout_prob = 0.0

    def run0(dmask):
        e = enc.clone().requires_grad_(True)
        net.zero_grad()
        h2 = G2pDecoderFn.apply(e, y, None, dmask, 77, 0.0, 0.33, net.attention.attn.conv.weight, net.attention.attn.conv.bias, net.attention.v,
                                net.output_emb.weight, d.weight_ih_l0, d.weight_hh_l0, d.bias_ih_l0, d.bias_hh_l0, d.weight_ih_l1, d.weight_hh_l1,
                                d.bias_ih_l1, d.bias_hh_l1)
        h1m = h2.grad_fn.saved_tensors[13 + sorted(['gates0', 'cells0', 'h1', 'h1m', 'gates1', 'cells1', 'h2', 'aq', 'att']).index('h1m')]
        h2.backward(dh2)
        return h2.detach(), e.grad.clone(), [p.grad.clone() for p in net.parameters() if p.grad is not None], h1m
    p1 = run0(None)
    p2 = run0((p1[3] != 0).float())
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1]) and all(torch.equal(p, q) for p, q in zip(p1[2], p2[2]))
    # the element-wise dropout of the encoder: forward and adjoint draw the same mask
    x = torch.randn(4, 9, 400, generator=gen).cuda() + 3.0              # (no zeros: the mask is readable from the output)
    dy = torch.randn(4, 9, 400, generator=gen).cuda()
    xg = x.clone().requires_grad_(True)
    yk = HipDropoutFn.apply(xg, None, 0.33, 555, 0)
    yk.backward(dy)
    mk = (yk != 0).float()
    xm = x.clone().requires_grad_(True)
    ym = HipDropoutFn.apply(xm, mk, 0.33, 0, 0)
    ym.backward(dy)
    assert torch.equal(yk, ym) and torch.equal(xg.grad, xm.grad)
    assert abs(float(mk.mean()) - 0.67) <= 5 * np.sqrt(0.33 * 0.67 / mk.numel())
    assert not torch.equal(mk, (HipDropoutFn.apply(x, None, 0.33, 556, 0) != 0).float())


def _philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint32 arrays (include/ttscube_math.h: ttsc_philox4x32) -> the four output words"""
    m32 = np.uint64(0xffffffff)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c


def _host_keep(elements, rows, words, tag, seed, p):
    """the {0,1} mask the kernels draw (include/ttscube_hip.h): counter (element >> 2, row, word, tag), key = seed, word element & 3,
    kept when ttsc_u01(word) = ((word >> 9) + 0.5) / 2^23 >= p in fp32"""
    el = np.asarray(elements, dtype=np.uint64)
    r = _philox4x32(el >> np.uint64(2), rows, words, tag, seed & 0xffffffff, seed >> 32)
    w = np.choose((el & np.uint64(3)).astype(np.int64), np.broadcast_arrays(*r, el)[:4])
    u = ((w >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
    return (u >= np.float32(p)).astype(np.float32)


def test_philox_attention_and_decoder_masks_rebuilt_on_the_host():
    """The masks of both decoder families rebuilt on the host from the documented counters and INJECTED give the bits of the Philox run, in h2,
    d enc and every parameter gradient: the forward and the backward (which recomputes the energies) both drew exactly these masks."""
    from ttscube_amd.networks import g2p_train as GT
    gen = torch.Generator().manual_seed(31)
    B, N, T, L, Em, H, D = 3, 6, 4, 45, 100, 200, 200
    A, R_ = D, T + 1
    net = _net(9, L, Em, H, D, 11)
    enc = (torch.randn(B, N, 2 * H, generator=gen) * 0.5).cuda()
    y = torch.randint(1, L, (B, T), generator=gen).to(torch.int32).cuda()
    dh2 = torch.randn(B, T, D, generator=gen).cuda()
    d = net.decoder
    TAG_ATT, TAG_DEC = 0x47324100 + GT.STREAM_DEC, 0x47324400 + GT.STREAM_DEC          # csrc/g2p_train.hip: family tag + stream id

    def host_masks(seed):
        b, t, i, j = np.meshgrid(np.arange(B), np.arange(T), np.arange(N), np.arange(A), indexing='ij')
        am = _host_keep(i * A + j, t + 1, b, TAG_ATT, seed, 0.1)                        # step t is row t + 1
        b, r, j = np.meshgrid(np.arange(B), np.arange(R_), np.arange(D), indexing='ij')
        dm = _host_keep(j, r, b, TAG_DEC, seed, 0.33)
        return torch.from_numpy(am).cuda(), torch.from_numpy(dm).cuda()

    def run(am, dm, seed):
        e = enc.clone().requires_grad_(True)
        net.zero_grad()
        h2 = GT.G2pDecoderFn.apply(e, y, am, dm, seed, 0.1, 0.33, net.attention.attn.conv.weight, net.attention.attn.conv.bias, net.attention.v,
                                   net.output_emb.weight, d.weight_ih_l0, d.weight_hh_l0, d.bias_ih_l0, d.bias_hh_l0, d.weight_ih_l1, d.weight_hh_l1,
                                   d.bias_ih_l1, d.bias_hh_l1)
        h1m = h2.grad_fn.saved_tensors[13 + sorted(['gates0', 'cells0', 'h1', 'h1m', 'gates1', 'cells1', 'h2', 'aq', 'att']).index('h1m')]
        h2.backward(dh2)
        return [h2.detach(), e.grad.clone()] + [p.grad.clone() for p in net.parameters() if p.grad is not None], h1m

    seed = (77 << 32) + 1234                                    # both key words in use
    am, dm = host_masks(seed)
    got, h1m = run(None, None, seed)
    assert torch.equal((h1m != 0).float(), dm)                  # the decoder family, read from the forward's zeros
    want, _ = run(am, dm, 0)
    assert len(got) == len(want) > 10
    for k, (a, c) in enumerate(zip(got, want)):
        assert torch.equal(a, c), k
    # the wrong attention mask does change the bits (the comparison above can tell): one flipped element
    am2 = am.clone()
    am2[1, 2, 3, 5] = 1 - am2[1, 2, 3, 5]
    other, _ = run(am2, dm, 0)
    assert not torch.equal(other[0], want[0]) and not torch.equal(other[1], want[1])
    # kept fractions within 5 standard deviations for the element counts used; another seed, another attention mask
    assert abs(float(am.mean()) - 0.9) <= 5 * np.sqrt(0.1 * 0.9 / am.numel()), float(am.mean())
    assert abs(float(dm.mean()) - 0.67) <= 5 * np.sqrt(0.33 * 0.67 / dm.numel()), float(dm.mean())
    am3, dm3 = host_masks(seed + 1)
    assert not torch.equal(am3, am)
    got3, _ = run(None, None, seed + 1)
    want3, _ = run(am3, dm3, 0)
    assert all(torch.equal(a, c) for a, c in zip(got3, want3))
    # the attention family alone decides the bits when the decoder mask is held: the Philox run of seed + 1 differs from (am, dm3) injected
    mixed, _ = run(am, dm3, 0)
    assert not torch.equal(mixed[0], got3[0])


# ---- reference parity ---------------------------------------------------------------------------------------------------------------
def _golden(name):
    from ttscube_amd.networks.g2p import G2P
    z = np.load(os.path.join(GOLD, name + '.npz'))
    g2p = G2P()
    with open(os.path.join(GOLD, 'g2p.encodings')) as f:
        enc = json.load(f)
    g2p.token2int, g2p.label2int, g2p.label_list = enc['token2int'], enc['label2int'], enc['label_list']
    g2p.initialize_network()
    shapes = [(k, tuple(s)) for k, s in json.loads(str(z['shapes']))]
    assert M.named_shapes(g2p.seq2seq) == shapes
    g2p.seq2seq.load_state_dict(M.fill_state_dict(shapes, int(z['seed'])), strict=True)
    g2p.to('cuda')
    g2p.train()
    return z, g2p


def _fp_bad(z, prefix, tensors):
    bad = {}
    for k in json.loads(str(z['grad_names'])):
        fp = {f: z['%s/%s/%s' % (prefix, k, f)] for f in ('norm', 'sum', 'probe', 'idx', 'samples', 'size')}
        dev = compare(tensors[k].detach().cpu().numpy(), k, fp)
        if max(dev.values()) > 1e-4:
            bad[k] = dev
    return bad


def test_training_without_dropout_matches_the_reference():
    from ttscube_amd.networks import g2p_train as GT
    z, g2p = _golden('g2p_train_a')
    net = g2p.seq2seq
    net.encoder.dropout = net.decoder.dropout = 0.0
    net.attention.dropout_prob = 0.0
    batches = json.loads(str(z['batches']))
    x, y = GT.make_batch(g2p, [(w, t) for w, t in batches[0]])
    assert np.array_equal(x, z['x']) and np.array_equal(y, z['y'])            # the reference's own construction
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    logits = GT.seq2seq_forward_train(net, xd, yd)
    assert logits.requires_grad and tuple(logits.shape) == z['logits'].shape
    assert float((logits.detach().cpu() - torch.from_numpy(z['logits'])).abs().max()) <= 1e-4
    opt = GT.g2p_configure_optimizer(g2p, lr=float(z['lr']))
    out = GT.g2p_training_step(g2p, [(w, t) for w, t in batches[0]], opt)
    assert abs(out['loss'] - float(z['loss'])) <= 1e-4
    params = dict(net.named_parameters())
    assert not _fp_bad(z, 'grad', {k: p.grad for k, p in params.items()})
    GT.g2p_training_step(g2p, [(w, t) for w, t in batches[1]], opt)['loss']
    assert not _fp_bad(z, 'param2', params)


def _masks_b(z):
    B, N = z['x'].shape
    T = z['y'].shape[1]
    un = lambda k, n: torch.from_numpy(np.unpackbits(z[k], axis=-1)[..., :n].astype(np.float32))
    m = {'att': list(un('mask_att', 200))}
    if int(z['lstm_dropout']):
        m.update(enc=un('mask_enc', 400), init=un('mask_init', 200), dec=list(un('mask_dec', 200)))
    return m


def test_training_with_replayed_dropout_masks_matches_the_reference():
    from ttscube_amd.networks import g2p_train as GT
    z, g2p = _golden('g2p_train_b')
    net = g2p.seq2seq
    if not int(z['lstm_dropout']):
        net.encoder.dropout = net.decoder.dropout = 0.0
    xd, yd = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['y']).cuda()
    logits = GT.seq2seq_forward_train(net, xd, yd, _masks_b(z))
    assert float((logits.detach().cpu() - torch.from_numpy(z['logits'])).abs().max()) <= 1e-4
    loss = GT.g2p_loss(logits, yd)
    loss.backward()
    assert abs(float(loss) - float(z['loss'])) <= 1e-4
    assert not _fp_bad(z, 'grad', {k: p.grad for k, p in net.named_parameters()})


def test_learn_batch_surface_and_both_optimizers_agree():
    from ttscube_amd.networks import g2p_train as GT
    z, g2p = _golden('g2p_train_a')
    batch = [(w, t) for w, t in json.loads(str(z['batches']))[0]]
    masks = None
    torch.manual_seed(3)
    loss = GT.learn_batch(g2p, batch, masks)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in g2p.seq2seq.parameters())
    # the reference's loop with torch.optim.Adam, and FlatAdamW from the same state and the same gradients
    sd0 = {k: v.detach().clone() for k, v in g2p.seq2seq.state_dict().items()}
    grads = {k: p.grad.detach().clone() for k, p in g2p.seq2seq.named_parameters()}
    adam = torch.optim.Adam(g2p.seq2seq.parameters(), lr=1e-3)
    adam.step()
    after_adam = {k: v.detach().clone() for k, v in g2p.seq2seq.state_dict().items()}
    g2p.seq2seq.load_state_dict(sd0)
    for k, p in g2p.seq2seq.named_parameters():
        p.grad = grads[k].clone()
    opt = GT.g2p_configure_optimizer(g2p, lr=1e-3)
    opt.step()
    for k, v in g2p.seq2seq.state_dict().items():
        assert _rel(v.cpu(), after_adam[k].cpu()) <= 1e-6, k


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _lexicon_subset(path, n):
    with open(os.path.join(GOLD, 'g2p.lexicon')) as f:
        lines = [l for l in f if len(l.strip().split('\t')) == 2]
    step = len(lines) // n
    with open(path, 'w') as f:
        f.writelines(lines[::step][:n])


def _train(args, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'train_g2p.py')] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_trainer_script_trains_saves_resumes_and_repeats(tmp_path):
    import re
    from ttscube_amd.networks.g2p import G2P
    train, base = str(tmp_path / 'train.lex'), str(tmp_path / 'g2p')
    _lexicon_subset(train, 150)
    common = ['--train-file', train, '--dev-file', train, '--batch-size', '32', '--patience', '1', '--seed', '5']
    r = _train(common + ['--store', base, '--max-epochs', '4'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for ext in ('.encodings', '.last', '.best'):
        assert os.path.exists(base + ext), ext
    avg = [float(v) for v in re.findall(r'Avg loss: ([0-9.eE+-]+)', r.stdout)]
    assert len(avg) >= 2 and avg[-1] < avg[0], avg
    g2p = G2P()
    g2p.load(base)
    g2p.to('cuda')
    g2p.eval()
    out = g2p.transcribe(['hello', 'world'])
    assert len(out) == 2 and all(isinstance(t, list) for t in out)
    # --load starts from BASE.last (not .best, not a fresh model): with no epoch to run, the .last the resumed run writes IS the loaded state
    last, best = torch.load(base + '.last', map_location='cpu'), torch.load(base + '.best', map_location='cpu')
    assert any(not torch.equal(last[k], best[k]) for k in last)          # (the two files differ, so the check below can tell them apart)
    base2 = str(tmp_path / 'resumed')
    r2 = _train(common + ['--store', base2, '--load', base, '--max-epochs', '0'])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    assert 'Setting baseline accuracy' in r2.stdout and os.path.exists(base2 + '.encodings')
    resumed = torch.load(base2 + '.last', map_location='cpu')
    assert sorted(resumed) == sorted(last) and all(torch.equal(resumed[k], last[k]) for k in last)
    # a 3-step run repeated with the same seed: bit-identical parameters
    sds = []
    for name in ('r1', 'r2'):
        b = str(tmp_path / name)
        r3 = _train(common + ['--store', b, '--max-steps', '3'])
        assert r3.returncode == 0, r3.stdout[-2000:] + r3.stderr[-4000:]
        sds.append(torch.load(b + '.last', map_location='cpu'))
    assert sorted(sds[0]) == sorted(sds[1])
    for k in sds[0]:
        assert torch.equal(sds[0][k], sds[1][k]), k
