"""Golden vectors for G2P TRAINING, produced by the REFERENCE ITSELF (build container only; the reference never travels).

    python tools/gen_golden_g2p_train.py   ->  tests/golden/g2p_train_a.npz, g2p_train_b.npz

Weights: the reference's Seq2Seq filled by oracle.meldecoder_ref.fill_state_dict (the fixtures store seed + shapes); encodings:
tests/golden/g2p.encodings; batches: words of tests/golden/g2p.lexicon.  Large tensors are stored as oracle/fingerprint.py fingerprints.

  g2p_train_a   dropout OFF (train() mode, encoder.dropout = decoder.dropout = attention.dropout_prob = 0: plain attributes read at call time).
                Two batches of 5 ragged words: x, y, logits and loss of the first, a fingerprint of every parameter's gradient, and a fingerprint
                of every parameter after two Adam(lr=1e-3) steps (batch 0, then batch 1).
  g2p_train_b   dropout ON, masks replayed.  After torch.manual_seed(s) the reference draws its masks on the CPU in a fixed order with
                empty_like(input).bernoulli_(1 - p): encoder layer-0 output (time-major inside torch.nn.LSTM: drawn as [N, B, 400]; the batch-major
                draw is tried too), start step [B, 1, 200], then per step the attention energy (a permuted
                view: shape [B, N, A], strides (N A, 1, N)) and the decoder [B, 1, 200].  The attention masks are also RECORDED through a wrapper
                around torch.dropout.  The fixture is refused unless every replayed attention mask equals the recorded one AND the float64
                formulation of tests/g2p_train_reference.py, fed the replayed masks, reproduces the reference's loss and every gradient
                fingerprint; the measured deviation is stored as `replay_check`.  If no replay of the LSTM masks validates, the fixture is made
                with LSTM dropout 0 and the recorded attention masks only, and says so in `note`."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

ref_import.setup()
from cube.networks.g2p import G2P, G2PDataset  # noqa: E402
from oracle import meldecoder_ref as M  # noqa: E402
from oracle.fingerprint import compare, fingerprint  # noqa: E402
from tests import g2p_train_reference as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED = 41
MASK_SEED = 97
GATE = 1e-4


def new_g2p():
    g2p = G2P()
    with open(os.path.join(OUT, 'g2p.encodings')) as f:
        enc = json.load(f)
    g2p.token2int, g2p.label2int, g2p.label_list = enc['token2int'], enc['label2int'], enc['label_list']
    torch.manual_seed(0)
    g2p.initialize_network()
    shapes = M.named_shapes(g2p.seq2seq)
    g2p.seq2seq.load_state_dict(M.fill_state_dict(shapes, SEED), strict=True)
    g2p.seq2seq.train()
    return g2p, shapes


def run(g2p, batch):
    """the reference's learn_batch with its Seq2Seq call watched -> (x, y, logits, loss tensor)"""
    seen = {}
    net = g2p.seq2seq
    orig = net.forward

    def spy(x, gs_output=None):
        out = orig(x, gs_output=gs_output)
        seen.update(x=x.clone(), y=gs_output.clone(), logits=out.detach().clone())
        return out
    net.forward = spy
    try:
        loss = g2p.learn_batch(batch)
    finally:
        del net.forward
    return seen['x'].numpy(), seen['y'].numpy(), seen['logits'].numpy(), loss


def put_fp(out, prefix, named):
    for k, t in named.items():
        for f, v in fingerprint(t.detach().numpy(), k).items():
            out['%s/%s/%s' % (prefix, k, f)] = v


def pick(ds, start, n):
    step = len(ds.examples) // (n + 1)
    return [ds.examples[start + i * step] for i in range(n)]


def gen_a(ds):
    g2p, shapes = new_g2p()
    net = g2p.seq2seq
    net.encoder.dropout = net.decoder.dropout = 0.0
    net.attention.dropout_prob = 0.0
    batches = [pick(ds, 11, 5), pick(ds, 23, 5)]
    optim = torch.optim.Adam(net.parameters(), lr=1e-3)
    out = dict(seed=SEED, shapes=json.dumps(shapes), batches=json.dumps(batches), lr=1e-3)
    for i, batch in enumerate(batches):
        x, y, logits, loss = run(g2p, batch)
        optim.zero_grad()
        loss.backward()
        if i == 0:
            out.update(x=x, y=y, logits=logits, loss=np.float64(loss.item()), grad_names=json.dumps([k for k, _ in net.named_parameters()]))
            put_fp(out, 'grad', {k: p.grad for k, p in net.named_parameters()})
        optim.step()
    put_fp(out, 'param2', dict(net.named_parameters()))
    print('g2p_train_a: x %s y %s loss %.6f' % (x.shape, y.shape, float(out['loss'])))
    np.savez_compressed(os.path.join(OUT, 'g2p_train_a.npz'), **out)


def replay(B, N, T, A, D, E, enc_layout, lstm_on):
    """the mask stream after torch.manual_seed(MASK_SEED), in the reference's order"""
    torch.manual_seed(MASK_SEED)
    m = {}
    if lstm_on:
        if enc_layout == 'bnc':
            m['enc'] = torch.empty(B, N, E).bernoulli_(1 - 0.33)
        else:                                                  # time-major inside torch.nn.LSTM
            m['enc'] = torch.empty(N, B, E).bernoulli_(1 - 0.33).permute(1, 0, 2).contiguous()
        m['init'] = torch.empty(B, 1, D).bernoulli_(1 - 0.33)
    m['att'], m['dec'] = [], []
    for _ in range(T):
        m['att'].append(torch.empty_strided((B, N, A), (N * A, 1, N)).bernoulli_(1 - 0.1).contiguous())
        if lstm_on:
            m['dec'].append(torch.empty(B, 1, D).bernoulli_(1 - 0.33))
    if not lstm_on:
        m['dec'] = None
    return m


def reference_pass(g2p, batch, lstm_on):
    net = g2p.seq2seq
    if not lstm_on:
        net.encoder.dropout = net.decoder.dropout = 0.0
    recorded = []
    orig = torch.dropout

    def spy(inp, p, train):
        out = orig(inp, p, train)
        recorded.append((out != 0).float().contiguous())
        return out
    torch.dropout = spy
    try:
        torch.manual_seed(MASK_SEED)
        x, y, logits, loss = run(g2p, batch)
    finally:
        torch.dropout = orig
    net.zero_grad()
    loss.backward()
    return x, y, logits, loss, recorded


def check64(g2p, x, y, masks, loss, lstm_on):
    """the float64 formulation with these masks against the reference's loss and gradients -> largest deviation"""
    net = g2p.seq2seq
    P = R.leaves(net.state_dict())
    lg = R.seq2seq_reference(P, torch.from_numpy(x), torch.from_numpy(y), masks)
    l64 = R.loss_reference(lg, torch.from_numpy(y))
    l64.backward()
    dev = abs(float(l64.detach()) - float(loss.detach()))
    for k, p in net.named_parameters():
        g = P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])
        dev = max(dev, max(compare(g.numpy(), k, fingerprint(p.grad.numpy(), k)).values()))
    return dev


def gen_b(ds):
    batch = pick(ds, 37, 4)
    note, chosen = '', None
    for lstm_on, layout in ((True, 'nbc'), (True, 'bnc'), (False, 'bnc')):
        g2p, shapes = new_g2p()
        x, y, logits, loss, recorded = reference_pass(g2p, batch, lstm_on)
        B, N = x.shape
        T = y.shape[1]
        masks = replay(B, N, T, 200, 200, 400, layout, lstm_on)
        if len(recorded) != T or any(not torch.equal(a, b) for a, b in zip(recorded, masks['att'])):
            print('g2p_train_b: lstm dropout %s, encoder layout %s: the replayed attention masks differ from the recorded ones' % (lstm_on, layout))
            if not lstm_on:
                masks['att'] = recorded
            else:
                continue
        dev = check64(g2p, x, y, masks, loss, lstm_on)
        print('g2p_train_b: lstm dropout %s, encoder layout %s: float64 replay deviates by %.3e' % (lstm_on, layout, dev))
        if dev <= GATE:
            chosen = (g2p, shapes, x, y, logits, loss, masks, dev, lstm_on)
            if not lstm_on:
                note = 'LSTM dropout 0: no replay of the LSTM masks reproduced the reference; attention masks only'
            break
    if chosen is None:
        raise SystemExit('g2p_train_b: no mask replay reproduces the reference; fixture not written')
    g2p, shapes, x, y, logits, loss, masks, dev, lstm_on = chosen
    B, N = x.shape
    T = y.shape[1]
    bits = lambda t: np.packbits(t.numpy().astype(np.uint8), axis=-1)
    out = dict(seed=SEED, mask_seed=MASK_SEED, shapes=json.dumps(shapes), batch=json.dumps(batch), x=x, y=y, logits=logits, loss=np.float64(loss.item()),
               replay_check=np.float64(dev), note=note, lstm_dropout=np.int64(lstm_on),
               grad_names=json.dumps([k for k, _ in g2p.seq2seq.named_parameters()]), mask_att=bits(torch.stack(masks['att'])))
    if lstm_on:
        out.update(mask_enc=bits(masks['enc']), mask_init=bits(masks['init']), mask_dec=bits(torch.stack(masks['dec'])))
    put_fp(out, 'grad', {k: p.grad for k, p in g2p.seq2seq.named_parameters()})
    print('g2p_train_b: x %s y %s loss %.6f replay_check %.3e %s' % (x.shape, y.shape, float(out['loss']), dev, note))
    np.savez_compressed(os.path.join(OUT, 'g2p_train_b.npz'), **out)


if __name__ == '__main__':
    ds = G2PDataset(os.path.join(OUT, 'g2p.lexicon'))
    gen_a(ds)
    gen_b(ds)
    for fn in ('g2p_train_a.npz', 'g2p_train_b.npz'):
        print('%-18s %7d bytes' % (fn, os.path.getsize(os.path.join(OUT, fn))))
