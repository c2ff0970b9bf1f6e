"""Golden vector for TRAINING the word-conditioned mel decoder, produced by the REFERENCE ITSELF (imported through tools/ref_import.py; build
container only — the reference never travels).

    python tools/gen_golden_cond_training.py   ->  tests/golden/languasito2_ft_train_a.npz

`Languasito2(cond_type='fasttext').forward` in training mode (cube/networks/modules.py:916-999 with the `_use_cond` branches :932-940, :979-988 and
`_get_cond_selection` :1079-1082) on B = 3 ragged sentences of 9 / 6 / 4 phonemes (padding rows exist and carry x_phon2word = 0), Nw = 5 words per
utterance of which the first two are left context (the collate's offset, cube/io_utils/io_cubegan.py:198-199), words no phoneme points at and words
shared by several phonemes.  Probes and fingerprints are those of `languasito2_train_a` (tools/gen_golden_training.py::gen_languasito_train): p_dur,
p_pitch, p_vuv, conditioning, both text losses, a fixed linear functional of the conditioning, and the gradient of their sum with respect to every
parameter as a fingerprint (oracle/fingerprint.py) — this time including `_lm_t.*` / `_lm_g.*`.

`replay_check`: the same comparison the GPU test makes, made here against THIS project's formulation of the step (the composition
networks/training.py::_languasito_branches launches, written with torch ops in float64 on the CPU).  It is the distance between the reference's fp32
autograd and exact arithmetic — the part of the test's margin that no kernel can win back — recorded per `_lm_*` tensor maximum (`replay_check`), over
all tensors (`replay_check_all`) and for the outputs (`replay_outputs`)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.gen_golden_training import OUT, _batch, _lang  # noqa: E402  (registers the reference's import path)
from oracle.fingerprint import compare, fingerprint  # noqa: E402

WORDS_LEFT = 2
# sentence-internal word of every phoneme (the collate adds WORDS_LEFT): utterance 0 shares words between phonemes, utterance 1 skips its middle word
PHON2WORD = [[0, 0, 0, 1, 1, 2, 2, 2, 2], [0, 0, 0, 2, 2, 2], [0, 1, 1, 2]]
NW = 5


def _losses(net, X, p_dur, p_pitch, p_vuv, conditioning, R):
    """cubegan.py:94-112 on the module's outputs + the linear functional of the conditioning"""
    t_dur = X['y_dur']
    t_pitch = X['y_pitch'].to(p_pitch.dtype)
    t_vuv = (t_pitch > 1).to(p_pitch.dtype)
    m_size = min(t_dur.shape[1], p_dur.shape[1])
    t_dur = t_dur[:, :m_size]
    p_dur_ = p_dur[:, :m_size, :]
    m_size = min(t_pitch.shape[1], p_pitch.shape[1])
    t_pitch = t_pitch[:, :m_size]
    p_pitch_ = p_pitch[:, :m_size]
    t_vuv = t_vuv[:, :m_size]
    p_vuv_ = p_vuv[:, :m_size]
    ignore = int(max(net._max_pitch, net._max_dur) + 1)
    loss_duration = F.cross_entropy(p_dur_.reshape(-1, p_dur_.shape[2]), t_dur.reshape(-1), ignore_index=ignore)
    loss_pitch = (torch.abs(t_pitch / net._max_pitch - p_pitch_) * t_vuv).mean() + torch.abs(t_vuv - p_vuv_).mean()
    loss_cond = (conditioning * R.to(conditioning.dtype)).sum() / conditioning.numel()
    return loss_duration, loss_pitch, loss_cond


def _ours_f64(net, X):
    """networks/training.py::_languasito_branches with torch ops: `net` = this project's Languasito2 in float64 on the CPU"""
    x_char, x_speaker = X['x_char'], X['x_speaker']
    x_words, p2w = X['x_words'].double(), X['x_phon2word']

    def stack(which):
        h = getattr(net, '_phon_emb_' + which)(x_char).permute(0, 2, 1)
        for layer in getattr(net, '_char_cnn_' + which):
            if hasattr(layer, 'conv'):
                h = torch.tanh(F.conv1d(h, layer.conv.weight, layer.conv.bias, padding=1))
        h, _ = getattr(net, '_char_rnn_' + which)(h.permute(0, 2, 1))
        spk = getattr(net, '_speaker_emb_' + which)(x_speaker)
        cond, _ = getattr(net, '_lm_' + which)(x_words)
        sel = torch.gather(cond, 1, p2w[:, :, None].expand(-1, -1, cond.shape[2]))
        return torch.cat([h, spk.repeat(1, h.shape[1], 1), sel], dim=-1)

    al = X['y_frame2phone']
    idx = torch.zeros((len(al), max(len(a) for a in al)), dtype=torch.long)
    for b, a in enumerate(al):
        idx[b, :len(a)] = torch.as_tensor(a)
        idx[b, len(a):] = a[-1]
    expand = lambda x: torch.gather(x, 1, idx[:, :, None].expand(-1, -1, x.shape[2]))
    lin = lambda m, x: F.linear(x, m.linear_layer.weight, m.linear_layer.bias)
    hcs = stack('t')
    out_dur = lin(net._dur_output, net._dur_rnn(hcs)[0])
    op = lin(net._pitch_output, net._pitch_rnn(expand(hcs))[0])
    g = expand(stack('g'))
    pitch = X['y_pitch'].double().unsqueeze(2) / net._max_pitch
    m = min(g.shape[1], pitch.shape[1])
    cond = lin(net._cond_output, net._cond_rnn(torch.cat([g[:, :m], pitch[:, :m]], dim=-1))[0])
    return out_dur, torch.sigmoid(op[:, :, 0]), torch.sigmoid(op[:, :, 1]), cond


def gen_languasito_ft_train(name, seed, nphs, num_phones=50, num_speakers=3, max_pitch=300, max_duration=12):
    net, shapes = _lang(seed, num_phones, num_speakers, max_pitch, max_duration, cond_type='fasttext')
    net.train()
    rng = np.random.RandomState(seed)
    B = len(nphs)
    x_char, x_speaker, y_dur, f2ps, y_pitch = _batch(rng, B, nphs, num_phones, num_speakers, max_pitch, max_duration, 7)
    x_words = (rng.randn(B, NW, 300) * 0.3).astype(np.float32)
    p2w = np.zeros((B, max(nphs)), dtype=np.int64)                     # padding rows: word 0, as the collate leaves them
    for b, row in enumerate(PHON2WORD):
        assert len(row) == nphs[b] and max(row) + WORDS_LEFT < NW
        p2w[b, :len(row)] = np.asarray(row) + WORDS_LEFT
    X = {'x_char': torch.from_numpy(x_char), 'x_speaker': torch.from_numpy(x_speaker), 'y_frame2phone': [list(f) for f in f2ps],
         'y_pitch': torch.from_numpy(y_pitch), 'y_dur': torch.from_numpy(y_dur), 'x_words': torch.from_numpy(x_words),
         'x_phon2word': torch.from_numpy(p2w), 'x_tok_ids': None}
    p_dur, p_pitch, p_vuv, conditioning = net(X)
    R = torch.from_numpy(rng.randn(*conditioning.shape).astype(np.float32))
    loss_duration, loss_pitch, loss_cond = _losses(net, X, p_dur, p_pitch, p_vuv, conditioning, R)
    (loss_duration + loss_pitch + loss_cond).backward()
    out = dict(seed=seed, shapes=json.dumps(shapes), x_char=x_char, x_speaker=x_speaker, y_dur=y_dur, y_pitch=y_pitch, x_words=x_words, x_phon2word=p2w,
               words_left=WORDS_LEFT, f2p_flat=np.concatenate([np.asarray(f) for f in f2ps]), f2p_len=np.asarray([len(f) for f in f2ps]),
               p_dur=p_dur.detach().numpy(), p_pitch=p_pitch.detach().numpy(), p_vuv=p_vuv.detach().numpy(),
               conditioning=conditioning.detach().numpy(), cond_probe=R.numpy(),
               loss_duration=float(loss_duration), loss_pitch=float(loss_pitch), loss_cond=float(loss_cond),
               cfg=json.dumps(dict(num_phones=num_phones, num_speakers=num_speakers, max_pitch=max_pitch, max_duration=max_duration)))
    names = []
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        names.append(k)
        for fk, fv in fingerprint(p.grad.numpy(), k).items():
            out['grad/%s/%s' % (k, fk)] = fv
    out['grad_names'] = json.dumps(names)
    assert any(k.startswith('_lm_t.') for k in names) and any(k.startswith('_lm_g.') for k in names)

    # ---- replay: this project's formulation in float64 against the fingerprints just made
    from ttscube_amd.networks.modules import Languasito2 as Ours
    ours = Ours(num_phones, num_speakers, max_pitch, max_duration, cond_type='fasttext')
    ours.load_state_dict(net.state_dict(), strict=True)
    ours = ours.double().train()
    o_dur, o_pitch, o_vuv, o_cond = _ours_f64(ours, X)
    outs = {}
    for got, key in ((o_dur, 'p_dur'), (o_pitch, 'p_pitch'), (o_vuv, 'p_vuv'), (o_cond, 'conditioning')):
        outs[key] = float((got.detach() - torch.from_numpy(out[key]).double()).abs().max())
    l_dur, l_pitch, l_cond = _losses(ours, X, o_dur, o_pitch, o_vuv, o_cond, R)
    outs['loss_duration'], outs['loss_pitch'] = abs(float(l_dur) - float(loss_duration)), abs(float(l_pitch) - float(loss_pitch))
    (l_dur + l_pitch + l_cond).backward()
    devs = {}
    for k, p in ours.named_parameters():
        fp = {f: out['grad/%s/%s' % (k, f)] for f in ('norm', 'sum', 'probe', 'idx', 'samples', 'size')}
        devs[k] = max(compare(p.grad.numpy(), k, fp).values())
    out['replay_check'] = np.float64(max(v for k, v in devs.items() if k.startswith('_lm_')))
    out['replay_check_all'] = np.float64(max(devs.values()))
    out['replay_outputs'] = json.dumps(outs)
    out['replay_per_tensor'] = json.dumps(devs)
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(name, 'B', B, 'frames', conditioning.shape[1], 'loss_dur %.5f loss_pitch %.5f loss_cond %.3e' %
          (float(loss_duration), float(loss_pitch), float(loss_cond)), len(names), 'gradient tensors')
    print('  replay (float64 formulation vs the fixture): _lm_* %.3e, all tensors %.3e (worst %s), outputs %s' %
          (float(out['replay_check']), float(out['replay_check_all']), max(devs, key=devs.get), {k: '%.2e' % v for k, v in outs.items()}))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    gen_languasito_ft_train('languasito2_ft_train_a', 63, [9, 6, 4])
