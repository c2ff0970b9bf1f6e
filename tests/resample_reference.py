"""float64 statement of the polyphase resampler (csrc/resample.hip, io_utils/resample.py): the definition, one direct sum per output sample.

    half = 10 max(up, down),   out_len = ceil(L up / down)
    y[n] = sum_i x[i] h[n down - i up + half]   over all i in [0, L) with |n down - i up| <= half

With h = design_filter(up, down) this is what scipy.signal.resample_poly(x, up, down) returns with its defaults (tests/test_resample_cpu.py holds
the two together).  A[n] = sum |x[i]| |h[...]| over the same terms is the scale of the rounding-error bound of a float32 evaluation."""
import numpy as np


def design_filter(up, down):
    """scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up in numpy"""
    half = 10 * max(up, down)
    fc = 1.0 / max(up, down)
    h = fc * np.sinc(fc * np.arange(-half, half + 1, dtype=np.float64)) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def out_len(L, up, down):
    return -(-L * up // down)


def resample(x, up, down, h=None, outputs=None):
    """x: 1-D -> (y, A) float64 for the output samples `outputs` (default: all out_len(len(x)) of them).  Python integers throughout: n down
    passes 2^31 for a long row."""
    x = np.asarray(x, dtype=np.float64)
    h = design_filter(up, down) if h is None else np.asarray(h, dtype=np.float64)
    L, half = x.shape[0], 10 * max(up, down)
    assert h.shape[0] == 2 * half + 1
    outputs = range(out_len(L, up, down)) if outputs is None else [int(n) for n in outputs]
    ax, ah = np.abs(x), np.abs(h)
    y, A = np.zeros(len(outputs)), np.zeros(len(outputs))
    for k, n in enumerate(outputs):
        c = n * down
        lo, hi = max(0, -(-(c - half) // up)), min(L - 1, (c + half) // up)       # ceil((c - half) / up) .. floor((c + half) / up)
        if hi < lo:
            continue
        taps = c - np.arange(lo, hi + 1) * up + half
        y[k] = np.dot(x[lo:hi + 1], h[taps])
        A[k] = np.dot(ax[lo:hi + 1], ah[taps])
    return y, A


def bound(A, up, down):
    """|float32 evaluation - y| <= (K + 2) 2^-24 A[n], K = ceil((2 half + 1) / up) terms per output: one rounding of every coefficient to float32,
    one of every product, K - 1 of the sum; to first order, for any order of summation, with or without FMA"""
    K = -(-(20 * max(up, down) + 1) // up)
    return (K + 2) * 2.0 ** -24 * A
