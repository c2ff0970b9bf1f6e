"""Latency of the sentence phonemizer (io_utils.io_text.Text2FeatBlizzard: text in, phones out, host work and the read-back of the tags included)
for one 120-character sentence and for 64 ragged sentences, three formulations of the same model on the same weights in the same process:
  built      ttsc_char_features -> Conv1dHip x 3 -> LSTMHip -> ttsc_tag_argmax                       (CubenetPhonemizer.tag)
  existing   the same middle composed from the ops the package had before: two weight[idx] gathers, torch.cat, _cnn_forward, LSTMHip,
             linear_hip, torch.argmax
  torch      the torch-op formulation on the GPU (nn.Embedding / nn.Conv1d / nn.LSTM / nn.Linear / argmax, no masking)
plus one B = 16 training step against its torch-op formulation (F.cross_entropy(ignore_index=0), torch.optim.AdamW).  Wall-clock medians after a
warm-up, the formulations timed alternately; kernel launches per call counted with torch.profiler where it is available.
    python tools/bench_phonemizer.py [--reps 20] [--rounds 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SENTENCE = ("Good morning, and welcome to the world of speech synthesis! Don't feel bad about us; we're only here to help, aren't we?")
WORDS = "the quick brown fox jumps over a lazy dog while it's raining cats and dogs in Spain, doesn't it? Yes! No; maybe: never".split()


def ragged_texts(n, seed=7):
    rng = np.random.RandomState(seed)
    return [' '.join(rng.choice(WORDS, size=rng.randint(3, 30))).capitalize() for _ in range(n)]


def tag_existing_ops(net, X, lengths=None, return_logits=False):
    from ttscube_amd import _lib
    from ttscube_amd.hip_layers import linear_hip
    from ttscube_amd.networks.modules import _cnn_forward
    dev = net._get_device()
    with torch.no_grad():
        x_char, x_case = X['x_char'].to(dev).long(), X['x_case'].to(dev).long()
        emb = torch.cat([net._char_emb.weight[x_char], net._case_emb.weight[x_case]], dim=-1)
        net._cnn()
        use = lengths if x_char.shape[0] > 1 else None
        h = _cnn_forward(net._hip['cnn'], emb, use)
        h = net._lstm()(h, lengths=use)
        logits = linear_hip(h, net._output_softmax.weight, net._output_softmax.bias)
        tags = torch.argmax(logits, dim=-1).to(torch.int32)
        if use is not None:
            tags = tags * (torch.arange(tags.shape[1], device=dev)[None, :] < _lib.lengths_dev(use, dev)[:, None])
    return tags


def torch_logits(net, X):
    dev = net._output_softmax.weight.device
    h = torch.cat([net._char_emb(X['x_char'].to(dev).long()), net._case_emb(X['x_case'].to(dev).long())], dim=-1).permute(0, 2, 1)
    for layer in net._convs:
        h = layer(h)
    h, _ = net._rnn(h.permute(0, 2, 1))
    return net._output_softmax(h)


def tag_torch_ops(net, X, lengths=None, return_logits=False):
    with torch.no_grad():
        return torch.argmax(torch_logits(net, X), dim=-1).to(torch.int32)


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
    except Exception as e:      # (a profiler that cannot attach is no reason to lose the timings)
        return 'n/a (%s)' % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    from ttscube_amd.io_utils.io_phonemizer import PhonemizerCollate, PhonemizerDataset, PhonemizerEncodings
    from ttscube_amd.io_utils.io_text import Text2FeatBlizzard
    from ttscube_amd.networks.phonemizer import CubenetPhonemizer
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    enc = PhonemizerEncodings(os.path.join(root, 'tests', 'golden', 'phonemizer.encodings'))
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, 'phonemizer')
        enc.save(base + '.encodings')
        CubenetPhonemizer(enc).save(base + '.model')
        t2f = Text2FeatBlizzard(base)
    net = t2f._phonemizer
    forms = {'built': type(net).tag.__get__(net), 'existing': lambda *x, **k: tag_existing_ops(net, *x, **k),
             'torch': lambda *x, **k: tag_torch_ops(net, *x, **k)}
    texts = ragged_texts(64)
    cases = {'one_sentence_%d_chars' % (len(SENTENCE) + 2): lambda: t2f(SENTENCE), 'batch_64_ragged': lambda: t2f.batch(texts)}
    out = {'reps': a.reps, 'rounds': a.rounds, 'batch_chars_min': min(len(t) for t in texts) + 2, 'batch_chars_max': max(len(t) for t in texts) + 2}
    for cname, call in cases.items():
        res = {k: [] for k in forms}
        for k, f in forms.items():
            net.tag = f
            for _ in range(a.warmup):
                call()
        for _ in range(a.rounds):
            for k, f in forms.items():
                net.tag = f
                res[k].append(wall_ms(call, a.reps))
        out[cname] = {k + '_ms_median': float(np.median(v)) for k, v in res.items()}
        for k, f in forms.items():
            net.tag = f
            out[cname][k + '_kernel_launches'] = launches(call)
    del net.tag
    # ---- one B = 16 training step
    ds = PhonemizerDataset(os.path.join(root, 'tests', 'golden', 'phonemizer_dev.json'))
    batch = PhonemizerCollate(enc, targets='aligned').collate_fn([ds[i] for i in range(16)])
    hip = CubenetPhonemizer(enc).cuda().train()
    ref = CubenetPhonemizer(enc)
    ref.load_state_dict(hip.state_dict())
    ref = ref.cuda().train()
    opt = torch.optim.AdamW(ref.parameters(), lr=ref._lr)

    def torch_step():
        opt.zero_grad()
        lg = torch_logits(ref, batch)
        loss = F.cross_entropy(lg.reshape(-1, lg.shape[-1]), batch['y_phon'].cuda().reshape(-1), ignore_index=0)
        loss.backward()
        opt.step()
        return loss
    steps = {'hip': lambda: hip.training_step(batch, 0), 'torch': torch_step}
    res = {k: [] for k in steps}
    for f in steps.values():
        for _ in range(a.warmup):
            f()
    for _ in range(a.rounds):
        for k, f in steps.items():
            res[k].append(wall_ms(f, max(a.reps // 4, 3)))
    out['train_step_b16_%d_chars' % batch['x_char'].shape[1]] = {k + '_ms_median': float(np.median(v)) for k, v in res.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
