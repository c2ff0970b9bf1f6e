"""Steady-state ms per `CubenetTextcoder.training_step` (textcoder.py:191-226) at B = 16 on synthetic utterances of reference-like length
(io_utils.synthetic: 20-60 phonemes, 2-11 frames each), HIP step against a torch-op formulation of the same step on the same weights in the same
process (torch.nn.LSTM / F.conv1d / nn.BatchNorm1d / F.cross_entropy / torch.optim.Adam), timed alternately with device events after a warm-up.
    python tools/bench_textcoder_step.py [--batch 16] [--steps 5] [--rounds 3] [--hip-only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def torch_forward(net, X):
    """the teacher-forced forward written with torch ops (the formulation the HIP step is measured against)"""
    dev = net._mel_output.linear_layer.weight.device
    pf = net._pframes
    x_char, x_speaker = X['x_char'].to(dev), X['x_speaker'].to(dev)
    B, N = x_char.shape
    h = net._phon_emb(x_char).permute(0, 2, 1)
    for layer in net._char_cnn:
        h = layer(h) if not hasattr(layer, 'conv') else layer.conv(h)
    h, _ = net._rnn_char(h.permute(0, 2, 1))
    h = torch.cat([h, net._speaker_emb(x_speaker).repeat(1, h.shape[1], 1)], dim=-1)
    out_dur = net._dur_output.linear_layer(net._dur_rnn(h)[0])
    al = X['y_frame2phone']
    m = max(len(a) // pf for a in al)
    idx = torch.full((B, m), N - 1, dtype=torch.long)
    for b, a in enumerate(al):
        k = len(a) // pf
        idx[b, :k] = torch.as_tensor(a[0:k * pf:pf])
    h = torch.gather(h, 1, idx.to(dev)[:, :, None].expand(-1, -1, h.shape[2]))
    h, _ = net._rnn_overlay(h)
    out_pitch = net._pitch_output.linear_layer(net._pitch_rnn(h)[0])
    y = X['y_mgc'].to(dev)
    cond = torch.cat([torch.full((B, 1, 80), -5.0, device=dev), y[:, pf - 1::pf][:, :y.shape[1] // pf]], dim=1)
    for layer in net._prenet.layers_h:
        cond = F.dropout(torch.relu(layer.linear_layer(cond)), 0.5, True)
    k = min(h.shape[1], cond.shape[1])
    hm, _ = net._mel_rnn(torch.cat([h[:, :k], cond[:, :k]], dim=-1))
    mel = net._mel_output.linear_layer(hm).reshape(B, -1, 80)
    p = mel.permute(0, 2, 1)
    for layer in net._postnet.network:
        p = layer.conv(p) if hasattr(layer, 'conv') else layer(p)
    return out_dur, out_pitch, mel, mel + p.permute(0, 2, 1)


def torch_step(net, batch, opt, ignore):
    dev = net._mel_output.linear_layer.weight.device
    pf = net._pframes
    opt.zero_grad()
    p_dur, p_pitch, pre, post = torch_forward(net, batch)
    t_dur, t_mel = batch['y_dur'].to(dev), batch['y_mgc'].to(dev)
    t_pitch = batch['y_pitch'].to(dev)[:, pf - 1::pf][:, :batch['y_pitch'].shape[1] // pf]
    m = min(t_dur.shape[1], p_dur.shape[1])
    l_dur = F.cross_entropy(p_dur[:, :m].reshape(-1, p_dur.shape[2]), t_dur[:, :m].reshape(-1), ignore_index=ignore)
    m = min(t_pitch.shape[1], p_pitch.shape[1])
    l_pitch = F.cross_entropy(p_pitch[:, :m].reshape(-1, p_pitch.shape[2]), t_pitch[:, :m].reshape(-1), ignore_index=ignore)
    m = min(pre.shape[1], t_mel.shape[1])
    loss = l_dur + l_pitch + (F.l1_loss(pre[:, :m], t_mel[:, :m]) + F.l1_loss(post[:, :m], t_mel[:, :m]))
    loss.backward()
    opt.step()
    return loss


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--hip-only', action='store_true')
    a = ap.parse_args()
    from ttscube_amd.io_utils.io_textcoder import TextcoderCollate
    from ttscube_amd.io_utils.synthetic import synthetic_encodings, synthetic_examples
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    enc = synthetic_encodings()
    torch.manual_seed(0)
    hip = CubenetTextcoder(enc).cuda().train()
    ref = CubenetTextcoder(enc)
    ref.load_state_dict(hip.state_dict())
    ref = ref.cuda().train()
    exs = list(synthetic_examples(a.batch, 2024))
    batch = TextcoderCollate(enc).collate_fn(exs)
    frames = [len(e['meta']['frame2phon']) for e in exs]
    ignore = int(max(enc.max_pitch, enc.max_duration) + 1)
    opt_t = torch.optim.Adam(ref.parameters(), lr=ref._lr)
    last = {}

    def run_hip():
        last['hip'] = hip.training_step(batch)

    def run_torch():
        last['torch'] = torch_step(ref, batch, opt_t, ignore)
    for _ in range(a.warmup):
        run_hip()
        if not a.hip_only:
            run_torch()
    torch.cuda.synchronize()
    res = {'hip': [], 'torch': []}
    for _ in range(a.rounds):
        res['hip'].append(timed(run_hip, a.steps))
        if not a.hip_only:
            res['torch'].append(timed(run_torch, a.steps))
    out = {'batch': a.batch, 'frames_min': min(frames), 'frames_max': max(frames), 'phonemes_max': int(batch['x_char'].shape[1]),
           'steps_per_round': a.steps, 'rounds': a.rounds, 'hip_ms_per_step': res['hip'], 'hip_ms_median': float(np.median(res['hip'])),
           'hip_last_loss': float(last['hip']['loss'])}
    if not a.hip_only:
        out.update(torch_ms_per_step=res['torch'], torch_ms_median=float(np.median(res['torch'])), torch_last_loss=float(last['torch'].detach()),
                   speedup=float(np.median(res['torch']) / np.median(res['hip'])))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
