"""One G2P training step (forward, loss, backward, Adam) at the reference's batch: B = 32 words, N = 12, T = 10, 45 labels, seeded weights — two
formulations of the same step on the same weights in the same process:
  hip     networks.g2p_train: HipEmbeddingFn -> lstm_forward_train (+ ttsc_dropout_scale) -> ttsc_g2p_train_forward / _backward (one launch each
          for the whole decoder loop) -> hip_linear -> ttsc_masked_ce -> optim.FlatAdamW
  torch   the same step in torch ops on the GPU (tests/g2p_train_reference.py in float32: the reference's per-step loop — matmul / tanh / softmax /
          sum per attention, two LSTM cells per step — with the encoder's input projections hoisted, autograd backward, torch.optim.Adam)
A second pair of legs times the DECODER ALONE (forward and backward from fixed encoder states; no encoder, loss or update): the part the two new
kernels replace — the whole-step figure also contains the encoder, which the torch side runs as hand-written LSTM cells (N steps x 2 directions x 2
layers), not MIOpen's fused nn.LSTM.
Both draw fresh dropout masks every step (hip: Philox in the kernels; torch: torch.rand on the device).  Wall-clock medians after a warm-up, the two
timed alternately in rounds; kernel launches per step are counted with torch.profiler on one extra step of each.  No gate: the numbers are recorded.
    python tools/bench_g2p_step.py [--reps 100] [--rounds 7]      (the JSON line is also written to profiles/g2p_train_bench.log)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return int(sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                   and 'memset' not in e.name.lower()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    from oracle import meldecoder_ref as M
    from tests import g2p_train_reference as R
    from ttscube_amd.networks import g2p_train as GT
    from ttscube_amd.networks.seq2seq import Seq2Seq, check_status
    from ttscube_amd.optim import FlatAdamW
    B, N, T, G, L = a.batch, 12, 10, 30, 45
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(3, G, (B, N), generator=gen)
    y = torch.randint(3, L, (B, T), generator=gen)
    for b in range(B):                                   # ragged words: <EOS> then <PAD>
        nx, ny = int(torch.randint(3, N, (1,), generator=gen)), int(torch.randint(2, T, (1,), generator=gen))
        x[b, nx], y[b, ny] = 2, 2
        x[b, nx + 1:], y[b, ny + 1:] = 0, 0
    x, y = x.to(dev), y.to(dev)
    net = Seq2Seq(G, L)
    sd = M.fill_state_dict(M.named_shapes(net), 33)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    opt = FlatAdamW(list(net.parameters()), 1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)

    def hip_step():
        opt.zero_grad()
        loss = GT.g2p_loss(GT.seq2seq_forward_train(net, x, y), y)
        loss.backward()
        opt.step()
        return loss

    P = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in sd.items()}
    adam = torch.optim.Adam(list(P.values()), lr=1e-3)

    def torch_step():
        keep = lambda shape, p: (torch.rand(shape, device=dev) >= p).float()
        masks = {'enc': keep((B, N, 400), 0.33), 'init': keep((B, 1, 200), 0.33), 'att': [keep((B, N, 200), 0.1) for _ in range(T)],
                 'dec': [keep((B, 1, 200), 0.33) for _ in range(T)]}
        adam.zero_grad()
        loss = R.loss_reference(R.seq2seq_reference(P, x, y, masks), y)
        loss.backward()
        adam.step()
        return loss

    # the decoder alone (what the two new kernels replace): forward and backward from fixed encoder states, no encoder, loss or update
    enc0 = (torch.randn(B, N, 400, generator=gen) * 0.5).to(dev)
    dlg = torch.randn(B, T, L, generator=gen).to(dev)

    def hip_decoder():
        net.zero_grad()
        e = enc0.clone().requires_grad_(True)
        (GT.decoder_forward_train(net, e, y) * dlg).sum().backward()

    def torch_decoder():
        keep = lambda shape, p: (torch.rand(shape, device=dev) >= p).float()
        masks = {'init': keep((B, 1, 200), 0.33), 'att': [keep((B, N, 200), 0.1) for _ in range(T)], 'dec': [keep((B, 1, 200), 0.33) for _ in range(T)]}
        adam.zero_grad()
        e = enc0.clone().requires_grad_(True)
        (R.decoder_reference(P, e, y, masks) * dlg).sum().backward()

    forms = {'hip': hip_step, 'torch': torch_step}
    dec_forms = {'hip_decoder': hip_decoder, 'torch_decoder': torch_decoder}
    first = {k: float(f().detach()) for k, f in forms.items()}    # the same weights, other masks: the first losses are close, not equal
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    check_status('bench_g2p_step')
    res = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, f in forms.items():
            res[k].append(wall_ms(f, a.reps))
    out = {'B': B, 'N': N, 'T': T, 'labels': L, 'reps': a.reps, 'rounds': a.rounds, 'first_step_loss': first}
    for k, v in res.items():
        out[k + '_ms_median'] = float(np.median(v))
        out[k + '_ms_min_max'] = [float(min(v)), float(max(v))]
    out['torch_over_hip'] = out['torch_ms_median'] / out['hip_ms_median']
    out['kernel_launches_per_step'] = {k: launches(f) for k, f in forms.items()}
    for f in dec_forms.values():
        for _ in range(a.warmup):
            f()
    dres = {k: [] for k in dec_forms}
    for _ in range(a.rounds):
        for k, f in dec_forms.items():
            dres[k].append(wall_ms(f, a.reps))
    for k, v in dres.items():
        out[k + '_ms_median'] = float(np.median(v))
    out['torch_decoder_over_hip_decoder'] = out['torch_decoder_ms_median'] / out['hip_decoder_ms_median']
    out['kernel_launches_decoder_only'] = {k: launches(f) for k, f in dec_forms.items()}
    out['hip_is_faster'] = out['hip_ms_median'] < out['torch_ms_median']
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'g2p_train_bench.log'), 'w') as f:
        f.write('python tools/bench_g2p_step.py --reps %d --rounds %d --batch %d\n%s\n' % (a.reps, a.rounds, B, line))
    return 0


if __name__ == '__main__':
    sys.exit(main())
