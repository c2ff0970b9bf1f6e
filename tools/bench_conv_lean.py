"""Per-layer A/B of the lean wide / tall convolution kernels at the headline workload's shapes (B = 64 x 8 s), through the C ABI.

    python tools/bench_conv_lean.py [--B 64] [--iters 10] [--rounds 5]

TTSC_CONV_LEAN is read at every launch, so ONE process alternates the two variants: `rounds` times (lean, plain), `iters` launches each, device
events around them.  Prints, per layer, the minimum and the median over the rounds of both variants and their ratio.  Layers: every wide (C, K, D) of
the generator's first two stages (the dilated convolution with its residual-free epilogue and, at D = 1, the second convolution of a pair with its
residual) and the two tall upsamplers."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttscube_amd.hip_layers import Conv1dHip


def timed(fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(name, fn, iters, rounds):
    res = {'1': [], '0': []}
    for v in ('1', '0'):   # warm both variants (code objects, LDS attribute)
        os.environ['TTSC_CONV_LEAN'] = v
        fn()
    for _ in range(rounds):
        for v in ('1', '0'):
            os.environ['TTSC_CONV_LEAN'] = v
            res[v].append(timed(fn, iters))
    os.environ.pop('TTSC_CONV_LEAN')
    l, p = res['1'], res['0']
    print('%-28s lean min %.4f med %.4f ms | plain min %.4f med %.4f ms | lean/plain (medians) %.4f  %s' % (
        name, min(l), statistics.median(l), min(p), statistics.median(p), statistics.median(l) / statistics.median(p),
        'ranges apart' if max(l) < min(p) or max(p) < min(l) else 'ranges overlap'), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    torch.manual_seed(0)
    for cin, cout, s, pad, L in ((512, 256, 5, 5, 800), (256, 128, 3, 6, 4001)):
        conv = Conv1dHip(cin, cout, 16, stride=s, padding=pad, transposed=True).set_precision('f16x3')
        conv.set_weight(torch.randn(cin, cout, 16) / (cin * 16 / s) ** 0.5, torch.randn(cout) * 0.1)
        x = torch.randn(a.B, cin, L, device='cuda')
        y = torch.empty(a.B, cout, conv.out_len(L), device='cuda')
        ab('tall %d->%d k16 s%d L=%d' % (cin, cout, s, L), lambda: conv(x, out=y, in_slope=0.1), a.iters, a.rounds)
    for Cc, L in ((256, 4001), (128, 12004)):
        x = torch.randn(a.B, Cc, L, device='cuda')
        r = torch.randn_like(x)
        y = torch.empty_like(x)
        for k in (3, 7, 11):
            for d in (1, 3, 5):
                conv = Conv1dHip(Cc, Cc, k, padding=d * (k - 1) // 2, dilation=d).set_precision('f16x3')
                conv.set_weight(torch.randn(Cc, Cc, k) / (Cc * k) ** 0.5, torch.randn(Cc) * 0.1)
                ab('wide C=%d k=%d d=%d' % (Cc, k, d), lambda: conv(x, out=y, in_slope=0.1), a.iters, a.rounds)
                if d == 1:
                    ab('wide C=%d k=%d d=1 +resid' % (Cc, k), lambda: conv(x, out=y, resid=r, in_slope=0.1), a.iters, a.rounds)


if __name__ == '__main__':
    main()
