"""Golden vectors for CubenetTextcoder TRAINING, produced by the REFERENCE ITSELF (build container only; the reference never travels).

    python tools/gen_golden_textcoder_train.py   ->  tests/golden/textcoder_train_{a,b,pf1}.npz, textcoder_collate.npz

Each train fixture: a batch made by the reference's TextcoderCollate, the seeded weights (oracle.meldecoder_ref.fill_state_dict: seed + shapes),
the PreNet / PostNet dropout masks of two steps (torch.dropout / F.dropout are patched to replay them), the four outputs and the four losses of
step 1 (textcoder.py:191-226, restated call for call on the reference module's outputs — `self.optimizers()` is Lightning's), the gradient of EVERY
parameter and the BatchNorm running statistics after step 1, and every parameter after step 2 of torch.optim.Adam(lr) (configure_optimizers,
textcoder.py:269-270).  Large tensors are stored as fingerprints (oracle/fingerprint.py)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

ref_import.setup()
from cube.io_utils.io_textcoder import TextcoderCollate  # noqa: E402
from cube.networks.textcoder import CubenetTextcoder  # noqa: E402
from oracle import meldecoder_ref as M  # noqa: E402
from oracle.fingerprint import fingerprint  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')


class Enc:
    """the fields the reference's model and collate read (its TextcoderEncodings.compute uses np.long, gone from numpy >= 1.24)"""

    def __init__(self, nph, nsp, max_pitch, max_duration):
        self.phon2int = {'p%d' % i: i for i in range(nph)}
        self.speaker2int = {'s%d' % i: i for i in range(nsp)}
        self.max_pitch = max_pitch
        self.max_duration = max_duration


def examples(rng, nphs, nph_vocab=40, max_pitch=200, dur_hi=6, unknown=False):
    out = []
    for k, n in enumerate(nphs):
        durs = rng.randint(1, dur_hi, size=n)
        f2p = [int(p) for p, d in enumerate(durs) for _ in range(d)]
        phones = ['p%d' % v for v in rng.randint(0, nph_vocab, size=n)]
        if unknown:
            phones[0] = 'zz'          # not in the encodings: x_char 0
        F_ = len(f2p)
        pitch = np.where(rng.uniform(size=F_) > 0.3, rng.randint(60, max_pitch, size=F_), 0).astype(np.float64)
        out.append({'meta': {'id': 'u%d' % k, 'phones': phones, 'speaker': 's%d' % rng.randint(0, 2), 'frame2phon': f2p},
                    'mgc': np.clip(rng.randn(F_, 80) - 2, -5, 1).astype(np.float32), 'pitch': pitch})
    return out


def pack_examples(exs):
    return dict(ex_meta=json.dumps([e['meta'] for e in exs]), ex_mgc=np.concatenate([e['mgc'] for e in exs]),
                ex_pitch=np.concatenate([e['pitch'] for e in exs]), ex_len=np.asarray([e['mgc'].shape[0] for e in exs]))


def gen_collate():
    rng = np.random.RandomState(5)
    enc = Enc(40, 2, 200, 9)
    exs = examples(rng, [4, 9, 6], unknown=True)
    b = TextcoderCollate(enc).collate_fn(exs)
    np.savez_compressed(os.path.join(OUT, 'textcoder_collate.npz'), enc=json.dumps(enc.__dict__), **pack_examples(exs),
                        **{'out_' + k: v.numpy() for k, v in b.items() if torch.is_tensor(v)},
                        out_f2p=json.dumps(b['y_frame2phone']))
    print('textcoder_collate', {k: tuple(v.shape) for k, v in b.items() if torch.is_tensor(v)})


def gen_train(name, seed, nphs, pframes=3, max_pitch=200, max_duration=9):
    torch.manual_seed(0)
    enc = Enc(40, 2, max_pitch, max_duration)
    net = CubenetTextcoder(enc, pframes=pframes)
    shapes = M.named_shapes(net)
    net.load_state_dict(M.fill_state_dict(shapes, seed), strict=True)
    net.train()
    rng = np.random.RandomState(seed)
    exs = examples(rng, nphs, max_pitch=max_pitch)
    batch = TextcoderCollate(enc).collate_fn(exs)
    B, T = batch['y_mgc'].shape[:2]
    n_pre = T // pframes + 1
    m_ov = max(len(a) // pframes for a in batch['y_frame2phone'])
    Fm = min(m_ov, n_pre) * pframes
    masks = []
    for _ in range(2):
        masks.append({'pre': (rng.uniform(size=(2, B, n_pre, 256)) > 0.5).astype(np.float32),
                      'post': (rng.uniform(size=(4, B, 512, Fm)) > 0.1).astype(np.float32)})
    state = {}
    orig_td, orig_fd = torch.dropout, F.dropout

    def td(x, p, train):
        assert p == 0.5 and train
        m = torch.from_numpy(state['m']['pre'][state['pre']])
        state['pre'] += 1
        return x * m * 2.0

    def fd(x, p=0.5, training=True, inplace=False):
        assert p == 0.1 and training and tuple(x.shape) == (B, 512, Fm), (p, training, x.shape)
        m = torch.from_numpy(state['m']['post'][state['post']])
        state['post'] += 1
        return x * m * (1.0 / 0.9)

    opt = torch.optim.Adam(net.parameters(), lr=net._lr)     # configure_optimizers (textcoder.py:269-270)
    rec = {}
    torch.dropout, F.dropout = td, fd
    try:
        for step in range(2):
            state.update(m=masks[step], pre=0, post=0)
            # ---- textcoder.py:191-226, call for call
            opt.zero_grad()
            p_dur, p_pitch, pre_mel, post_mel = net.forward(batch)
            assert state['pre'] == 2 and state['post'] == 4
            t_dur = batch['y_dur']
            t_pitch = net._prepare_pitch(batch['y_pitch'])
            t_mel = batch['y_mgc']
            outs = (p_dur.detach().clone(), p_pitch.detach().clone(), pre_mel.detach().clone(), post_mel.detach().clone())
            m_size = min(t_dur.shape[1], p_dur.shape[1])
            t_dur = t_dur[:, :m_size]
            p_dur = p_dur[:, :m_size, :]
            m_size = min(t_pitch.shape[1], p_pitch.shape[1])
            t_pitch = t_pitch[:, :m_size]
            p_pitch = p_pitch[:, :m_size, :]
            m_size = min(pre_mel.shape[1], t_mel.shape[1])
            pre_mel = pre_mel[:, :m_size, :]
            post_mel = post_mel[:, :m_size, :]
            t_mel = t_mel[:, :m_size, :]
            loss_duration = net._loss_cross(p_dur.reshape(-1, p_dur.shape[2]), t_dur.reshape(-1))
            loss_pitch = net._loss_cross(p_pitch.reshape(-1, p_pitch.shape[2]), t_pitch.reshape(-1))
            loss_mel = net._loss_l1(pre_mel, t_mel) + net._loss_l1(post_mel, t_mel)
            loss = loss_duration + loss_pitch + loss_mel
            loss.backward()
            if step == 0:
                rec.update(p_dur=outs[0].numpy(), p_pitch=outs[1].numpy(), pre_mel=outs[2].numpy(), post_mel=outs[3].numpy(),
                           losses=np.asarray([float(loss), float(loss_mel), float(loss_pitch), float(loss_duration)]))
                grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
            opt.step()
            if step == 0:
                rec['bn'] = {k: v.detach().clone() for k, v in net.state_dict().items() if 'running' in k}
    finally:
        torch.dropout, F.dropout = orig_td, orig_fd
    out = dict(seed=seed, shapes=json.dumps(shapes), pframes=pframes, cfg=json.dumps(dict(max_pitch=max_pitch, max_duration=max_duration)),
               grad_names=json.dumps(list(grads)), **pack_examples(exs))
    for k in ('p_dur', 'p_pitch', 'pre_mel', 'post_mel', 'losses'):
        out[k] = rec[k]
    for s, mk in enumerate(masks):
        out['mask%d_pre' % s] = np.packbits(mk['pre'].astype(bool), axis=-1)
        out['mask%d_post' % s] = np.packbits(mk['post'].astype(bool), axis=-1)
        out['mask%d_post_shape' % s] = np.asarray(mk['post'].shape)
    for k, v in rec['bn'].items():
        out['bn/' + k] = v.numpy()
    for k, g in grads.items():
        for f, v in fingerprint(g.numpy(), k).items():
            out['grad/%s/%s' % (k, f)] = v
    for k, p in net.named_parameters():
        for f, v in fingerprint(p.detach().numpy(), k).items():
            out['param2/%s/%s' % (k, f)] = v
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(name, 'B', B, 'T', T, 'mel', rec['pre_mel'].shape, 'losses', rec['losses'])


CASES = {
    'textcoder_train_a': lambda: gen_train('textcoder_train_a', 61, [9]),
    'textcoder_train_b': lambda: gen_train('textcoder_train_b', 62, [7, 11, 5]),
    'textcoder_train_pf1': lambda: gen_train('textcoder_train_pf1', 63, [6, 9, 4], pframes=1),
    'textcoder_collate': gen_collate,
}

if __name__ == '__main__':
    for c in (sys.argv[1:] or list(CASES)):
        CASES[c]()
