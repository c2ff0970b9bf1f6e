"""Plain references for the GEMM family of csrc/gemm.hip and the two mat-vecs (no GPU): float64 statements of every contract, their
abs-value companions S for the per-element bound, and host models of what the kernels do differently from a plain matmul — the fp16 hi / lo
split of ttsc_linear_forward_split (bit-faithful fp16 rounding), the row-shifted B operand of ttsc_gemm (h_prev without materialising it)
and the fixed-order split-K reduction.

The bound, per element:      |got - ref64| <= tau * S + TINY,      S = |A| . |B| (+ |bias| + |acc0|)
with tau = TAU = 2^-20 for every kernel here: 4 x the worst err / S of a serial, unfused float32 evaluation (f32_serial below: 2^-22.3 ..
2^-21.9 for K = 17 .. 2100; test_gemm_reference_cpu.py re-measures it at the GPU cases' shapes).  TINY only absorbs float64 rounding of the
comparison itself: there is no absolute floor, so operands of any scale are held to the same relative bound.

Contracts (numpy float64 in, float64 out):
    linear   y = act(x . w^T + bias [+ y0 when accumulate])                         ttsc_linear_forward / ttsc_linear_forward_split
    gemm     C = opA(A) . opB(shift(B)) [+ C0]                                       ttsc_gemm
    colsum   out[c] = sum_r x[r, c] [+ out0]                                         ttsc_colsum
    matvec   out = W x  or  W^T u                                                    ttsc_matvec
"""
import numpy as np

TAU = 2.0 ** -20
TINY = 1e-30
LO_SHIFT = 11                      # the split GEMM stores lo' = rn16((v - hi) * 2^LO_SHIFT)
ACT_LIPSCHITZ = {None: 1.0, 'relu': 1.0, 'tanh': 1.0, 'sigmoid': 0.25}
# evaluating tanhf / 1 / (1 + expf(-v)) in float32 and rounding the result: a few ulp of the result (expf and tanhf are 1-2 ulp functions,
# sigmoid adds one addition and one division) — 4 ulp = 2^-21 relative, none for the exact relu / identity
ACT_EVAL = {None: 0.0, 'relu': 0.0, 'tanh': 2.0 ** -21, 'sigmoid': 2.0 ** -21}


def f64(t):
    """torch tensor or array -> numpy float64 (a copy on the host)"""
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def act_f64(p, act):
    if act is None:
        return p
    if act == 'relu':
        return np.maximum(p, 0.0)
    if act == 'tanh':
        return np.tanh(p)
    if act == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-p))
    raise ValueError(act)


# ---- float64 contracts and their abs-value companions -------------------------------------------------------------------------------------

def linear_f64(x, w, bias=None, act=None, acc0=None):
    """(ref, S, pre): ref = act(pre), pre = x . w^T + bias + acc0, S = |x| . |w|^T + |bias| + |acc0|"""
    x, w = f64(x), f64(w)
    pre = x @ w.T
    S = np.abs(x) @ np.abs(w).T
    for extra in (bias, acc0):
        if extra is not None:
            pre = pre + f64(extra)
            S = S + np.abs(f64(extra))
    return act_f64(pre, act), S, pre


def overlapping_rows(flat, M, K, ldx):
    """row m = flat[m * ldx : m * ldx + K] (ldx < K: overlapping rows, the STFT framing mode)"""
    flat = np.asarray(flat)
    return np.stack([flat[m * ldx:m * ldx + K] for m in range(M)])


def shift_rows(b, shift, period):
    """the materialised row-shifted operand: row r holds b[r + shift] when 0 <= r % period + shift < period, zeros otherwise"""
    b = np.asarray(b)
    if shift == 0:
        return b.copy()
    out = np.zeros_like(b)
    r = np.arange(b.shape[0])
    t = r % period + shift
    ok = (t >= 0) & (t < period)
    out[r[ok]] = b[r[ok] + shift]
    return out


def gemm_f64(a, b, trans_a=False, trans_b=False, shift=0, period=0, acc0=None):
    """(ref, S) of C = opA(a) . opB(shift(b)) + acc0; a is [M, K] ([K, M] when trans_a), b is [K, N] ([N, K] when trans_b)"""
    a, b = f64(a), f64(b)
    if shift:
        assert not trans_b
        b = shift_rows(b, shift, period)
    A = a.T if trans_a else a
    B = b.T if trans_b else b
    ref = A @ B
    S = np.abs(A) @ np.abs(B)
    if acc0 is not None:
        ref = ref + f64(acc0)
        S = S + np.abs(f64(acc0))
    return ref, S


def colsum_f64(x, acc0=None):
    x = f64(x)
    ref, S = x.sum(axis=0), np.abs(x).sum(axis=0)
    if acc0 is not None:
        ref, S = ref + f64(acc0), S + np.abs(f64(acc0))
    return ref, S


def matvec_f64(W, v, transpose=False):
    W, v = f64(W), f64(v)
    if transpose:
        return W.T @ v, np.abs(W).T @ np.abs(v)
    return W @ v, np.abs(W) @ np.abs(v)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------

def worst_ratio(got, ref, S):
    """max err / S over the elements (0 where both vanish, inf where err > 0 on S == 0)"""
    err = np.abs(f64(got) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / S)
    return float(r.max())


def within(got, ref, S, tau=TAU, act=None):
    """the per-element bound, pushed through the activation: lip * tau * S + (evaluating the activation in float32) + TINY"""
    got = f64(got)
    if not np.isfinite(got).all():
        return False
    bound = ACT_LIPSCHITZ[act] * tau * S + ACT_EVAL[act] * np.abs(ref) + TINY
    return bool((np.abs(got - ref) <= bound).all())


def log2_ratio(r):
    return float(np.log2(r)) if r > 0 else float('-inf')


# ---- host models --------------------------------------------------------------------------------------------------------------------------------

def rn16(v):
    """round-to-nearest-even to fp16 (overflow to inf, gradual underflow), returned as float32 — exactly what v_cvt_f16_f32 gives"""
    with np.errstate(over='ignore'):
        return np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)


def split_f16(v, lo_shift=LO_SHIFT):
    """(hi, lo') as the split GEMM stages them: hi = rn16(v), lo' = rn16((v - hi) * 2^lo_shift); v - hi is one float32 operation (exact
    inside the fp16 range).  lo_shift = 0 is the plain split of the convolutions (and of this kernel before it scaled its low half)."""
    v = np.asarray(v, dtype=np.float32)
    hi = rn16(v)
    with np.errstate(invalid='ignore'):
        d = (v - hi).astype(np.float32)
        lo = rn16(d * np.float32(2.0 ** lo_shift))
    return hi, lo


def split_linear_model(x, w, bias=None, acc0=None, lo_shift=LO_SHIFT, slice_k=16, drop_slices=()):
    """ttsc_linear_forward_split's arithmetic on the host, float32 out: per 16-wide k-slice (one MFMA) the three products of fp16 halves —
    exact in float32 — are added into float32 accumulators, lo'_x.hi_w and hi_x.lo'_w into one, hi_x.hi_w into the other; the epilogue is
    acc_hi + 2^-lo_shift * acc_lo, + bias, + y0.  (Inside one MFMA the 16 products are summed here in float64: the hardware's own order is
    not modelled.)  drop_slices: k-slices left out (defect injection)."""
    xh, xl = split_f16(x, lo_shift)
    wh, wl = split_f16(w, lo_shift)
    M, K = xh.shape
    N = wh.shape[0]
    acc_hi = np.zeros((M, N), np.float32)
    acc_lo = np.zeros((M, N), np.float32)
    d = np.float64
    for s, k0 in enumerate(range(0, K, slice_k)):
        if s in drop_slices:
            continue
        k = slice(k0, min(k0 + slice_k, K))
        acc_lo = (acc_lo + xl[:, k].astype(d) @ wh[:, k].astype(d).T).astype(np.float32)
        acc_lo = (acc_lo + xh[:, k].astype(d) @ wl[:, k].astype(d).T).astype(np.float32)
        acc_hi = (acc_hi + xh[:, k].astype(d) @ wh[:, k].astype(d).T).astype(np.float32)
    y = (acc_hi + acc_lo * np.float32(2.0 ** -lo_shift)).astype(np.float32)
    if bias is not None:
        y = (y + np.asarray(bias, np.float32)).astype(np.float32)
    if acc0 is not None:
        y = (y + np.asarray(acc0, np.float32)).astype(np.float32)
    return y


def f32_serial(A, B, acc0=None):
    """the yardstick: C = A [M, K] . B [K, N] in float32, one k at a time, product and sum rounded separately (no fma)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32) if acc0 is None else np.asarray(acc0, np.float32).copy()
    for k in range(A.shape[1]):
        acc = (acc + (A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    return acc


GM, GN, GK = 128, 128, 16


def gemm_splits(M, N, K):
    """the split-K plan of ttsc_gemm: (splits, kchunk) — splits is what the kernel launches (ceil(K / kchunk))"""
    tiles = -(-M // GM) * -(-N // GN)
    if tiles >= 256 or K < 1024:
        s = 1
    else:
        s = max(1, min(-(-768 // tiles), -(-K // 256), 512))
    kchunk = -(-(-(-K // s)) // GK) * GK
    return -(-K // kchunk), kchunk


def splitk_model(A, B, splits, kchunk, acc0=None, drop=()):
    """fixed-order split-K on the host, float32: every split's partial tile over its own k range (f32_serial), then
    C = ((acc0 + p_0) + p_1) + ... in ascending split order (gemm_splitk_reduce_kernel).  drop: splits left out (defect injection)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    K = A.shape[1]
    parts = [f32_serial(A[:, z * kchunk:min((z + 1) * kchunk, K)], B[z * kchunk:min((z + 1) * kchunk, K)]) for z in range(splits)]
    s = np.zeros_like(parts[0]) if acc0 is None else np.asarray(acc0, np.float32).copy()
    for z, p in enumerate(parts):
        if z not in drop:
            s = (s + p).astype(np.float32)
    return s


# ---- operands of the split-linear scale sweep (shared by the GPU test and the CPU test of the yardstick) ---------------------------------------

SPLIT_M, SPLIT_N, SPLIT_KS = 130, 129, (36, 256)
SPLIT_SX = (10, 0, -4, -8, -12)
SPLIT_SW = (0, -3, -7, -11, -14)
F16_MAX = 65504.0


def sweep_operands(K, sx, sw, M=SPLIT_M, N=SPLIT_N):
    """x ~ randn * 2^sx [M, K], w ~ randn * 2^sw [N, K], bias at the scale of the products' sum; float32"""
    rng = np.random.RandomState(1000 + 37 * K + 5 * (sx + 20) + (sw + 20))
    x = (rng.randn(M, K) * 2.0 ** sx).astype(np.float32)
    w = (rng.randn(N, K) * 2.0 ** sw).astype(np.float32)
    b = (rng.randn(N) * 2.0 ** (sx + sw) * K ** 0.5).astype(np.float32)
    return x, w, b


def mixed_operands(K, M=SPLIT_M, N=SPLIT_N):
    """embedding-like: every row of x and every column of K carries its own scale, spread over 2^-12 .. 2^0"""
    rng = np.random.RandomState(77 + K)
    x = (rng.randn(M, K) * 2.0 ** rng.uniform(-12, 0, (M, 1)) * 2.0 ** rng.uniform(-12, 0, (1, K))).astype(np.float32)
    w = (rng.randn(N, K) * 2.0 ** rng.uniform(-12, 0, (1, K))).astype(np.float32)
    b = (rng.randn(N) * 2.0 ** -12).astype(np.float32)
    return x, w, b


def edge_operands(K, M=SPLIT_M, N=SPLIT_N):
    """|v| just below the fp16 maximum, both signs, with float32 low bits: hi = 65504 or the binade below and the largest low halves there
    are — a scaled low half must stay finite (|v - hi| <= 16 -> |lo'| <= 2^15)"""
    rng = np.random.RandomState(99 + K)
    x = (rng.choice([-1.0, 1.0], (M, K)) * rng.uniform(F16_MAX - 48.0, F16_MAX + 15.0, (M, K))).astype(np.float32)
    x[0, :4] = [65519.99, -65519.99, 65504.0, 65488.01]          # the last float32 values that still round to 65504, and its neighbours
    w = (rng.choice([-1.0, 1.0], (N, K)) * rng.uniform(F16_MAX - 48.0, F16_MAX + 15.0, (N, K))).astype(np.float32)
    return x, w, None


def colsum_parts(R):
    return min(-(-R // 256), 256) if R >= 1024 else 1


def matvec_parts(R):
    return min(R // 32, 32) if R >= 64 else 1
