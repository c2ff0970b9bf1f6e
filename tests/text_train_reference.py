"""Plain references for the small kernels text-side training runs on (no GPU): csrc/textcoder_train.hip (the BatchNorm -> tanh -> dropout
block and the four-term loss), csrc/ce_loss.hpp (the shared cross-entropy rows), csrc/phonemizer.hip (ttsc_masked_ce, ttsc_tag_argmax) and
csrc/g2p_train.hip (ttsc_dropout_scale).  For every operation: a float64 statement, its abs-value companion S (the first-order error scale
of evaluating the expression in floating point — each term by its magnitude, each intermediate's error carried into what reads it) and a
float32 host model that evaluates the same formula in float32, sums one term at a time.

The bound, per element:      |got - ref64| <= tau * S + FLT_MIN
No tolerance floor: FLT_MIN = 2^-126 is the smallest normal float32 — a float32 result cannot say less about a value below it, and only such
values meet it here (exp(-160) in the +-80 rows, whose float64 gradients go down to 1e-270; the squares of the 1e-20 channel).

tau per operation = 4 x the worst err / S of the float32 host model over all cases below (the *_case builders and their shape lists), rounded up to a power of two
(test_text_train_reference_cpu.py re-measures each and asserts worst <= tau / 4).  The 4 covers another (fixed) summation order and device
expf / logf / tanhf, which are not correctly rounded.  Measured on the host model, log2 of the worst err / S:

    operation      worst     tau      what carries it
    bn_y           -22.8     2^-20    the mean 1e3 / std 1e-2 channel at n = 2056
    bn_stats       -21.5     2^-19    mean / invstd / running statistics: the one-at-a-time float32 sum of 2056 values (gamma 0 channel, then
                                      the 1e3 one at -21.8).  The constant channel is 0.75 so that its float32 running sum is exact: a constant
                                      like 0.7 drifts the one-at-a-time mean by 2^-16.4 at n = 2056 — summation-order drift of the yardstick,
                                      which would only loosen tau for everything that reads the mean
    bn_dx          -23.4     2^-21
    bn_dparam      -23.5     2^-21    dgamma / dbeta
    ce_value       -21.8     2^-19
    ce_grad        -23.3     2^-21
    l1_value       -11.7     2^-9     the one-at-a-time float32 sum of 2^21 absolute differences
    l1_grad        -38.0     2^-24    +-1 / n is one rounding: tau is the unit roundoff itself, not 4 x a ratio that n near 2^21 makes tiny
    tag_logits     -22.0     2^-19    (mixed scales)
    dropout        -23.5     2^-21

(the kernels reduce in double, so l1_value — and to a lesser degree bn_stats — is slack for THEM by construction of the yardstick; their
measured ratios are in tests/test_text_train_f64_gpu.py)
"""
import numpy as np

from tests.gemm_reference import f32_serial, f64, log2_ratio  # noqa: F401  (re-exported)

FLT_MIN = 2.0 ** -126
TAU = {'bn_y': 2.0 ** -20, 'bn_stats': 2.0 ** -19, 'bn_dx': 2.0 ** -21, 'bn_dparam': 2.0 ** -21, 'ce_value': 2.0 ** -19, 'ce_grad': 2.0 ** -21,
       'l1_value': 2.0 ** -9, 'l1_grad': 2.0 ** -24, 'tag_logits': 2.0 ** -19, 'dropout': 2.0 ** -21}

TC_THREADS = 256
TC_BN_TAG = 0x424E3131
GT_TAG_DROP = 0x47324500
TAG_MAX_FLOATS = 4096              # K + P of ttsc_tag_argmax (64 KiB of LDS / 4 rows / 4 bytes)
F32 = np.float32


def within(got, ref, S, tau):
    """the per-element bound; a non-finite value never passes"""
    got = f64(got)
    if got.shape != np.shape(ref) or not np.isfinite(got).all():
        return False
    return bool((np.abs(got - ref) <= tau * S + FLT_MIN).all())


def worst_ratio(got, ref, S):
    """max over the elements of (err - FLT_MIN) / S: the tau this result would need (0 where the error is at most FLT_MIN, inf where a
    larger one meets S == 0)"""
    err = np.maximum(np.abs(f64(got) - ref) - FLT_MIN, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / S)
    return float(np.max(r))


def _ssum(a, axis=-1):
    """float32 sum, one term at a time in index order"""
    return np.cumsum(np.asarray(a, F32), axis=axis, dtype=F32).take(-1, axis=axis)


# ---- dropout masks from the documented counters -----------------------------------------------------------------------------------------------

def philox_keep(n, p, seed, word2, tag, first=0):
    """{0,1} float32 [n]: element i = first .. first + n - 1 draws Philox-4x32-10 at counter (i >> 2, i >> 34, word2, tag), key = seed (low,
    high word), takes word i & 3 and is kept when ttsc_u01(word) >= p (float32) — host Philox / u01 of oracle/wavernn_ref.py"""
    from oracle import wavernn_ref as W
    i = np.arange(first, first + n, dtype=np.uint64)
    ctr = np.stack([(i >> np.uint64(2)) & np.uint64(0xffffffff), i >> np.uint64(34), np.full(n, word2, np.uint64), np.full(n, tag, np.uint64)],
                   axis=1).astype(np.uint32)
    key = np.tile(np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], np.uint32), (n, 1))
    words = W.philox_array(ctr, key)[np.arange(n), (i & np.uint64(3)).astype(np.int64)]
    return (W.math_array(W.FN_U01, words) >= F32(p)).astype(F32)


def bn_philox_mask(B, C, F, p, seed, layer):
    """the PostNet dropout mask of ttsc_bn_tanh_dropout_train_*: element index i = (b * C + c) * F + f"""
    return philox_keep(B * C * F, p, seed, layer, TC_BN_TAG).reshape(B, C, F)


def dropout_philox_mask(n, p, seed, stream_id):
    return philox_keep(n, p, seed, stream_id, GT_TAG_DROP)


# ---- BatchNorm -> tanh -> dropout ----------------------------------------------------------------------------------------------------------------

def _cn(a):
    """[B, C, F] -> [C, B * F]: a channel's values in (b, f) order"""
    return np.ascontiguousarray(np.transpose(a, (1, 0, 2))).reshape(a.shape[1], -1)


def _bcf(a, B, F):
    return np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], B, F), (1, 0, 2)))


def bn_f64(x, gamma, beta, rm0, rv0, mask, p, momentum=0.1, eps=1e-5, dy=None):
    """float64 statement of the block and the abs-value companion of every output -> {name: (ref, S)}.  p, momentum and eps enter as the
    float32 values the C ABI takes.  With dy: dx, dgamma, dbeta as well.

    Forward, per channel over its n = B * F values (u = the unit roundoff that tau stands for):
      mean = sum x / n                      S_mean = A = sum |x| / n
      d = x - mean                          E_d = |x| + A                      (rounding of the difference <= u (|x| + |mean|), error of mean)
      var = sum d^2 / n                     S_var = 2 sum |d| E_d / n + var     (d^2 moves by 2 |d| E_d; squares, sum and division: var)
      invstd = (var + eps)^-1/2             S_inv = invstd + invstd^3 S_var / 2 (own roundings + the derivative times S_var)
      xh = d * invstd                       S_xh = E_d invstd + |d| S_inv
      a = gamma xh + beta                   S_a = |gamma| S_xh + |beta|         (S_xh >= |xh| covers the product's rounding)
      y = k tanh(a), k = keep / (1 - p)     S_y = k (S_a + |t|)                 (tanh is 1-Lipschitz; evaluating it: |t|)
      rmean = m mean + (1 - m) rm0          S = m S_mean + (1 - m) |rm0|
      rvar = m sum d^2 / (n - 1) + ..       S = m S_var n / (n - 1) + (1 - m) |rv0|
    Backward:
      dz = dy k (1 - t^2)                   E_t = S_a + |t|,  S_dz = |dy| k (2 |t| E_t + (1 - t^2))
      dbeta = sum dz, c1 = dbeta / n        S_dbeta = sum S_dz
      dgamma = sum dz xh, c2 = dgamma / n   S_dgamma = sum (S_dz |xh| + |dz| S_xh)
      dx = gamma invstd (dz - c1 - xh c2)   S_dx = |gamma| (S_inv |dz - c1 - xh c2| + invstd (S_dz + S_c1 + S_xh |c2| + |xh| S_c2))
    A channel with gamma = 0 (and beta = 0) has S = 0 where the value is an exact zero: the bound then asks for the exact zero."""
    x = f64(x)
    B, C, F = x.shape
    n = float(B * F)
    p, m, eps = float(F32(p)), float(F32(momentum)), float(F32(eps))
    g, be = f64(gamma)[:, None], f64(beta)[:, None]
    xc = _cn(x)
    k = _cn(f64(mask)) / (1.0 - p)
    mean = xc.sum(1, keepdims=True) / n
    A = np.abs(xc).sum(1, keepdims=True) / n
    d = xc - mean
    E_d = np.abs(xc) + A
    m2 = (d * d).sum(1, keepdims=True)
    var = m2 / n
    S_var = 2.0 * (np.abs(d) * E_d).sum(1, keepdims=True) / n + var
    inv = 1.0 / np.sqrt(var + eps)
    S_inv = inv + 0.5 * inv ** 3 * S_var
    xh = d * inv
    S_xh = E_d * inv + np.abs(d) * S_inv
    a = g * xh + be
    S_a = np.abs(g) * S_xh + np.abs(be)
    t = np.tanh(a)
    out = {'y': (_bcf(k * t, B, F), _bcf(k * (S_a + np.abs(t)), B, F)),
           'mean': (mean[:, 0], A[:, 0]), 'invstd': (inv[:, 0], S_inv[:, 0]),
           'rmean': (m * mean[:, 0] + (1 - m) * f64(rm0), m * A[:, 0] + (1 - m) * np.abs(f64(rm0))),
           'rvar': (m * m2[:, 0] / (n - 1.0) + (1 - m) * f64(rv0), m * S_var[:, 0] * n / (n - 1.0) + (1 - m) * np.abs(f64(rv0)))}
    if dy is None:
        return out
    dyc = _cn(f64(dy))
    E_t = S_a + np.abs(t)
    dz = dyc * k * (1.0 - t * t)
    S_dz = np.abs(dyc) * k * (2.0 * np.abs(t) * E_t + (1.0 - t * t))
    sum_dz = dz.sum(1, keepdims=True)
    S_sum_dz = S_dz.sum(1, keepdims=True)
    sum_dzx = (dz * xh).sum(1, keepdims=True)
    S_sum_dzx = (S_dz * np.abs(xh) + np.abs(dz) * S_xh).sum(1, keepdims=True)
    c1, c2 = sum_dz / n, sum_dzx / n
    inner = dz - c1 - xh * c2
    S_inner = S_dz + S_sum_dz / n + S_xh * np.abs(c2) + np.abs(xh) * S_sum_dzx / n
    out['dx'] = (_bcf(g * inv * inner, B, F), _bcf(np.abs(g) * (S_inv * np.abs(inner) + inv * S_inner), B, F))
    out['dgamma'] = (sum_dzx[:, 0], S_sum_dzx[:, 0])
    out['dbeta'] = (sum_dz[:, 0], S_sum_dz[:, 0])
    return out


BN_GROUP = {'y': 'bn_y', 'mean': 'bn_stats', 'invstd': 'bn_stats', 'rmean': 'bn_stats', 'rvar': 'bn_stats', 'dx': 'bn_dx', 'dgamma': 'bn_dparam',
            'dbeta': 'bn_dparam'}
BN_DEFECTS = ('var_e2', 'biased_rvar', 'eps_outside', 'no_scale', 'mask_scalar_index', 'no_c2', 'dgamma_from_x', 'stats_rows_only')


def bn_f32(x, gamma, beta, rm0, rv0, mask, p, momentum=0.1, eps=1e-5, dy=None, defect=None):
    """the block in float32 -> {name: float32 array}: two-pass statistics, every sum one term at a time in (b, f) order, the backward from
    the saved float32 mean / invstd as the kernels do.  defect: one of BN_DEFECTS (what a wrong kernel would compute):
      var_e2             var = E[x^2] - E[x]^2 in float32          biased_rvar        sum d^2 / n into running_var
      eps_outside        invstd = 1 / (sqrt(var) + eps)            no_scale           1 / (1 - p) missing
      mask_scalar_index  the float4 walk (F % 4 == 0) reads the mask of vector j at row offset j, not 4 j
      no_c2              dx without the xh c2 term                 dgamma_from_x      dgamma = sum dz x
      stats_rows_only    the statistics divide by B, the row count, not by B * F"""
    assert defect is None or defect in BN_DEFECTS
    x = np.asarray(x, F32)
    B, C, F = x.shape
    n = F32(B if defect == 'stats_rows_only' else B * F)
    p, m, eps = F32(p), F32(momentum), F32(eps)
    g, be = np.asarray(gamma, F32)[:, None], np.asarray(beta, F32)[:, None]
    mk = np.asarray(mask, F32)
    if defect == 'mask_scalar_index' and F % 4 == 0:
        j = np.arange(F) // 4
        mk = np.ascontiguousarray(mk[:, :, j + np.arange(F) % 4])
    scale = F32(1.0) if defect == 'no_scale' else F32(1.0) / (F32(1.0) - p)
    k = _cn(mk) * scale
    xc = _cn(x)
    mean = (_ssum(xc) / n)[:, None]
    d = xc - mean
    if defect == 'var_e2':
        m2 = ((_ssum(xc * xc) / n)[:, None] - mean * mean) * n
    else:
        m2 = _ssum(d * d)[:, None]
    var = m2 / n
    with np.errstate(invalid='ignore', divide='ignore'):
        inv = F32(1.0) / (np.sqrt(var) + eps) if defect == 'eps_outside' else F32(1.0) / np.sqrt(var + eps)
    xh = d * inv
    t = np.tanh(g * xh + be)
    nm1 = n if defect == 'biased_rvar' else n - F32(1.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = {'y': _bcf(t * k, B, F), 'mean': mean[:, 0], 'invstd': inv[:, 0],
               'rmean': m * mean[:, 0] + (F32(1.0) - m) * np.asarray(rm0, F32),
               'rvar': m * (m2[:, 0] / nm1) + (F32(1.0) - m) * np.asarray(rv0, F32)}
    if dy is None:
        return out
    dz = _cn(np.asarray(dy, F32)) * k * (F32(1.0) - t * t)
    sum_dz = _ssum(dz)[:, None]
    sum_dzx = _ssum(dz * (xc if defect == 'dgamma_from_x' else xh))[:, None]
    c1, c2 = sum_dz / n, sum_dzx / n
    inner = dz - c1 if defect == 'no_c2' else dz - c1 - xh * c2
    out.update(dx=_bcf((g * inv) * inner, B, F), dgamma=sum_dzx[:, 0], dbeta=sum_dz[:, 0])
    return {k_: np.asarray(v, F32) for k_, v in out.items()}


BN_C = 6
BN_CHANNELS = ('benign', 'mean 1e3 std 1e-2', 'constant', 'gamma 50', 'gamma 0', 'scale 1e-20')
BN_SHAPES = ((1, 2), (2, 1), (1, 4), (3, 8), (2, 1028), (5, 7), (1, 1025), (2, 8))       # (B, F); F % 4 == 0: the float4 kernels
BN_P = 0.1


def bn_case(B, F, mask=None):
    """x [B, 6, F] with one regime per channel (BN_CHANNELS), gamma / beta, non-trivial running statistics, a {0,1} mask (p = 0.1; or the
    one handed in) and dy; float32"""
    rng = np.random.RandomState(100 * B + F)
    x = np.empty((B, BN_C, F), F32)
    x[:, 0] = 1.5 * rng.randn(B, F) + 0.3
    x[:, 1] = 1e3 + 1e-2 * rng.randn(B, F)
    x[:, 2] = 0.75                 # (two mantissa bits: its float32 running sum stays exact, so the yardstick measures rounding, not drift)
    x[:, 3] = rng.randn(B, F)
    x[:, 4] = rng.randn(B, F) - 0.5
    x[:, 5] = 1e-20 * rng.randn(B, F)
    gamma = np.array([1.2, 0.8, 1.1, 50.0, 0.0, 1.3], F32)
    beta = np.array([0.1, -0.2, 0.3, 0.5, 0.25, -0.1], F32)
    rm0 = np.array([0.2, 900.0, -0.4, 0.1, -0.3, 0.05], F32)
    rv0 = np.array([1.5, 0.5, 0.8, 1.2, 0.9, 0.7], F32)
    if mask is None:
        mask = (rng.rand(B, BN_C, F) >= BN_P).astype(F32)
        mask.reshape(-1)[rng.randint(B * BN_C * F)] = 0.0                  # at least one dropped value whatever the size
    dy = rng.randn(B, BN_C, F).astype(F32)
    return dict(x=x, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, mask=np.asarray(mask, F32), p=BN_P, dy=dy)


# ---- cross-entropy with ignore_index ---------------------------------------------------------------------------------------------------------

def ce_blocks(R, cap=512):
    """workgroups of the cross-entropy stage: 4 rows (waves) each, capped — 512 for ttsc_masked_ce and the pitch head, 256 for the duration
    head; beyond the cap a workgroup walks r += 4 * blocks"""
    return max(min(-(-R // 4), cap), 1)


def tc_loss_grid(Rd, Rp, n):
    return min(-(-Rd // 4), 256), min(-(-Rp // 4), 512), max(min(-(-(n // 4) // (4 * TC_THREADS)), 512), 1)


def tc_loss_workspace_bytes(Rd, Rp, n):
    return 64 + 2 * 8 * sum(tc_loss_grid(Rd, Rp, n))


def masked_ce_workspace_bytes(R):
    return 64 + 8 * ce_blocks(R)


def ce_valid(target, K, ignore):
    t = np.asarray(target, np.int64)
    return (t != ignore) & (t >= 0) & (t < K)


def ce_f64(logits, target, ignore, empty='nan'):
    """-> (value, S_value, grad [R, K], S_grad): the mean over the rows whose target is in [0, K) and is not `ignore` of lse - x_t, and
    d value / d logits = (softmax - onehot) / count; rows left out have a zero gradient row.  No valid row: NaN (ttsc_textcoder_loss, torch's
    mean) or 0 (ttsc_masked_ce), and a zero gradient either way.  Per row, m = max x, s = sum exp(x - m), lse = m + log s, p = exp(x - lse):
      S_lse = sum_k p_k (1 + |x_k| + |m|) + |log s| + |lse|     each exp's argument moves by u (|x_k| + |m|) and its value by u, so s moves by
                                                               the p-weighted mean relative to s; then the log's and the sum's own rounding
      S_row = S_lse + |x_t|                                     (lse - x_t)
      S_p   = p_k (1 + |x_k| + |lse| + S_lse)                   the argument x_k - lse moves by u (|x_k| + |lse|) + the error of lse
      S_g   = (S_p + onehot) / count                            (p - 1) rounds relative to p + 1; 1 / count relative to the result
      S_value = sum S_row / count"""
    x = f64(logits)
    R, K = x.shape
    t = np.asarray(target, np.int64)
    valid = ce_valid(t, K, ignore)
    cnt = int(valid.sum())
    grad, S_g = np.zeros((R, K)), np.zeros((R, K))
    if cnt == 0:
        return (float('nan') if empty == 'nan' else 0.0), 0.0, grad, S_g
    xv, tv = x[valid], t[valid]
    m = xv.max(1, keepdims=True)
    s = np.exp(xv - m).sum(1, keepdims=True)
    lse = m + np.log(s)
    pk = np.exp(xv - lse)
    S_lse = (pk * (1.0 + np.abs(xv) + np.abs(m))).sum(1, keepdims=True) + np.abs(np.log(s)) + np.abs(lse)
    rows = np.arange(len(tv))
    x_t = xv[rows, tv][:, None]
    onehot = np.zeros_like(xv)
    onehot[rows, tv] = 1.0
    grad[valid] = (pk - onehot) / cnt
    S_g[valid] = (pk * (1.0 + np.abs(xv) + np.abs(lse) + S_lse) + onehot) / cnt
    return float((lse - x_t).sum() / cnt), float((S_lse + np.abs(x_t)).sum() / cnt), grad, S_g


CE_DEFECTS = ('mean_all_rows', 'no_max', 'onehot_tm1', 'skip_rows', 'ignored_unwritten')


def ce_f32(logits, target, ignore, empty='nan', defect=None, cap=512):
    """the same in float32, sums one term at a time -> (value float32, grad float32 [R, K] — started from NaN, as the tests pre-fill it).
    defect: mean_all_rows (divides by R), no_max (exp(x) without the max), onehot_tm1 (the one-hot at t - 1), skip_rows (rows >= 4 *
    ce_blocks(R, cap) never visited), ignored_unwritten (gradient rows of left-out targets not written)"""
    assert defect is None or defect in CE_DEFECTS
    x = np.asarray(logits, F32)
    R, K = x.shape
    t = np.asarray(target, np.int64)
    valid = ce_valid(t, K, ignore)
    cnt = R if defect == 'mean_all_rows' else int(valid.sum())
    grad = np.full((R, K), np.nan, F32)
    seen = np.ones(R, bool)
    if defect == 'skip_rows':
        seen = np.arange(R) < 4 * ce_blocks(R, cap)
    if defect != 'ignored_unwritten':
        grad[~valid & seen] = 0.0
    use = valid & seen
    if int(valid.sum()) == 0:
        return F32('nan') if empty == 'nan' else F32(0.0), grad
    inv = F32(1.0 / cnt)
    xv, tv = x[use], t[use]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        m = np.zeros((len(tv), 1), F32) if defect == 'no_max' else xv.max(1, keepdims=True)
        s = _ssum(np.exp(xv - m))[:, None]
        lse = m + np.log(s)
        rows = np.arange(len(tv))
        onehot = np.zeros_like(xv)
        onehot[rows, (tv - 1) % K if defect == 'onehot_tm1' else tv] = 1.0
        grad[use] = (np.exp(xv - lse) - onehot) * inv
        value = F32(np.float64(_ssum(lse[:, 0] - xv[rows, tv])) / cnt) if len(tv) else F32(0.0)
    return value, grad


CE_KS = (1, 7, 63, 64, 65, 201)
CE_ROWS = {'dur': (1, 1023, 1024, 1025), 'pitch': (1, 2047, 2048, 2049), 'masked': (1, 2047, 2048, 2049)}
CE_CAP = {'dur': 256, 'pitch': 512, 'masked': 512}


def ce_case(R, K, ignore_inside, seed=0, bad_row=None):
    """logits [R, K] float32 whose rows cycle randn / 80 randn / one +80 among -80s (the +80 at the target, one class off it, or anywhere),
    targets with about a third ignored and the last class in every sixth row; ignore_index = 0 (inside [0, K)) or K + 5 (beyond).
    bad_row: that row's target is out of range (K + 2, not ignore_index)"""
    rng = np.random.RandomState(7919 * K + 31 * R + 2 * seed + int(ignore_inside))
    ignore = 0 if ignore_inside else K + 5
    x = rng.randn(R, K)
    kind = np.arange(R) % 3
    x[kind == 1] *= 80.0
    t = rng.randint(0, K, R).astype(np.int64)
    t[np.arange(R) % 6 == 4] = K - 1
    for r in np.nonzero(kind == 2)[0]:
        x[r] = -80.0
        x[r, (t[r] + (r // 3) % 3 * (1 + rng.randint(K))) % K] = 80.0
    t[rng.rand(R) < 1.0 / 3.0] = ignore
    if R == 1:
        t[0] = K - 1                                                    # the single row is a valid one, in the last class
    if bad_row is not None:
        t[bad_row] = K + 2
    return x.astype(F32), t, ignore


# ---- the two mel L1 terms ------------------------------------------------------------------------------------------------------------------------

def l1_f64(pre, target):
    """-> (value, S_value, grad, S_grad): mean |pre - t| and sign(pre - t) / n (0 at an exact tie).  The difference of two float32 is one
    rounding, u |pre - t|, and so is every further step: S_value = the value itself; S_grad = |grad| (1 / n rounded once; an exact 0 stays)"""
    d = f64(pre) - f64(target)
    n = d.size
    g = np.sign(d) / n
    v = float(np.abs(d).sum() / n)
    return v, v, g, np.abs(g)


L1_DEFECTS = ('n_float4', 'skip_tail')


def l1_f32(pre, target, defect=None):
    """float32, one term at a time.  defect: n_float4 (the gradient divides by n / 4, the float4 count), skip_tail (the float4s a thread
    reaches only on a trip beyond the 4 the uncapped grid is sized for: j >= 4 * nbm * TC_THREADS)"""
    assert defect is None or defect in L1_DEFECTS
    d = np.asarray(pre, F32) - np.asarray(target, F32)
    n = d.size
    g = np.sign(d) * F32(1.0 / (n // 4 if defect == 'n_float4' else n))
    a = np.abs(d)
    if defect == 'skip_tail':
        a = a[:4 * 4 * tc_loss_grid(0, 0, n)[2] * TC_THREADS]
    return F32(np.float64(_ssum(a)) / n), g.astype(F32)


L1_CAP_N = 4 * 512 * 4 * TC_THREADS                  # 512 workgroups x 256 threads x 4 trips x float4
L1_NS = (4, L1_CAP_N - 4, L1_CAP_N, L1_CAP_N + 4)
L1_TIES = (0, 3, 1025)                               # exact ties pre == target (post ties one further on), where n allows
L1_TAIL = 32768.0                                    # |pre - t| of the last four values: 4 * 2^15 / n = 2^-4 at n = 2^21, against a bound
#                                                      tau * S = 2^-9 * (mean |d| ~ 0.8 + 2^-4): over 30 x the bound


def l1_case(n):
    rng = np.random.RandomState(n % 1000 + 5)
    t = rng.randn(n).astype(F32)
    pre = (t + rng.randn(n)).astype(F32)
    post = (t + 0.5 * rng.randn(n)).astype(F32)
    for i in L1_TIES:
        if i + 1 < n:
            pre[i] = t[i]
            post[i + 1] = t[i + 1]
    if n > 8:
        pre[-4:] = t[-4:] + F32(L1_TAIL) * np.array([1, -1, 1, 1], F32)
        post[-4:] = t[-4:] - F32(L1_TAIL) * np.array([1, 1, -1, 1], F32)
    return pre, post, t


# ---- tag head -------------------------------------------------------------------------------------------------------------------------------------

def tag_valid(M, lens, period):
    if lens is None:
        return np.ones(M, bool)
    r = np.arange(M)
    return (r % period) < np.asarray(lens)[r // period]


def tag_f64(x, W, b, lens=None, period=0):
    """-> (logits [M, P], S, tags int [M], ambiguous bool [M]): logits = x . W^T + b, S = |x| . |W|^T + |b| (the GEMM family's companion);
    tag = the first maximum; padding rows (r % period >= len) have zero logits and tag 0, and so has a row whose logits are all NaN.  A row is
    ambiguous when its float64 top two differ (by more than nothing) by no more than the bound on the two: either may win in float32.  Every
    dot product is summed in the same order, so identical rows of W give identical float64 logits: an exact tie, which is NOT ambiguous."""
    x, W = f64(x), f64(W)
    M, P = x.shape[0], W.shape[0]
    with np.errstate(invalid='ignore'):
        lg = np.stack([(x[r][None, :] * W).sum(-1) for r in range(M)])
        S = np.stack([(np.abs(x[r])[None, :] * np.abs(W)).sum(-1) for r in range(M)])
    if b is not None:
        lg, S = lg + f64(b), S + np.abs(f64(b))
    ok = tag_valid(M, lens, period)
    lg[~ok], S[~ok] = 0.0, 0.0
    tags, amb = tag_argmax(lg, ok, S)
    return lg, S, tags, amb


def tag_argmax(lg, ok, S=None, last=False, pad_tag=False):
    """first (last: defect) maximum of every row, NaN never wins; 0 for padding rows (pad_tag: defect — the arg-max of what the tile held)"""
    M, P = lg.shape
    tags, amb = np.zeros(M, np.int64), np.zeros(M, bool)
    for r in range(M):
        if not (ok[r] or pad_tag):
            continue
        v = np.where(np.isnan(lg[r]), -np.inf, lg[r])
        if not np.isfinite(v).any():
            continue
        i = int(np.argmax(v)) if not last else P - 1 - int(np.argmax(v[::-1]))
        tags[r] = i
        if S is not None and P > 1:
            rest = np.delete(v, i)
            j = int(np.argmax(rest))
            gap = v[i] - rest[j]
            j += j >= i
            amb[r] = 0.0 < gap <= TAU['tag_logits'] * (S[r, i] + S[r, j]) + 2 * FLT_MIN
    return tags, amb


TAG_DEFECTS = ('bias_pass0', 'last_max', 'pad_tag')


def tag_f32(x, W, b, lens=None, period=0, defect=None):
    """float32: every dot product one k at a time, product and sum rounded separately, bias last -> (logits float32, tags).  defect:
    bias_pass0 (the bias reaches the first 128 classes only), last_max (the last maximum wins a tie), pad_tag (a padding row — zeros in the
    tile — gets the arg-max of the bias)"""
    assert defect is None or defect in TAG_DEFECTS
    x, W = np.asarray(x, F32), np.asarray(W, F32)
    M, P = x.shape[0], W.shape[0]
    ok = tag_valid(M, lens, period)
    with np.errstate(invalid='ignore', over='ignore'):
        lg = f32_serial(np.where(ok[:, None], x, F32(0.0)), W.T)
        if b is not None:
            bb = np.asarray(b, F32).copy()
            if defect == 'bias_pass0':
                bb[128:] = 0.0
            lg = lg + bb
    tags, _ = tag_argmax(lg.astype(np.float64), ok, last=defect == 'last_max', pad_tag=defect == 'pad_tag')
    lg[~ok] = 0.0
    return lg, tags


TAG_SHAPES = ((1, 1, 4), (5, 7, 8), (4, 129, 12), (9, 300, 400), (3, 512, 3584))         # (M, P, K)
TAG_TIE_CLASSES = (7, 70, 135, 263)        # identical rows of W and bias: lanes 7 and 6 of one pass, and the second and third 128-class pass
TAG_CASES = tuple('%dx%dx%d' % s for s in TAG_SHAPES) + ('ldx', 'ragged', 'mixed', 'ties', 'nan')
TAG_AMBIGUOUS_CAP = 0.02


def tag_case(name):
    """-> dict(x [M, K], W [P, K], b [P], lens, period, ldx) float32.  'ldx': rows at a stride of K + 8; 'ragged': 3 utterances of period 8
    with lengths 5, 0, 8 — rows 8 .. 15 are two tiles of padding only, tile 1 is half padding; 'mixed': W ~ 2^-12, x ~ 2^12 with a scale per
    column; 'ties': TAG_TIE_CLASSES share one row of W and one bias, raised above every other class, so every row's maximum is a four-way
    exact tie across lanes and passes; 'nan': row 2 of x is NaN"""
    shapes = {'ldx': (6, 40, 16), 'ragged': (24, 33, 16), 'mixed': (40, 130, 64), 'ties': (8, 300, 16), 'nan': (5, 9, 8)}
    M, P, K = shapes[name] if name in shapes else tuple(int(v) for v in name.split('x'))
    rng = np.random.RandomState(M + 3 * P + 5 * K)
    x = rng.randn(M, K).astype(F32)
    W = (rng.randn(P, K) / np.sqrt(K)).astype(F32)
    b = (0.5 * rng.randn(P)).astype(F32)
    c = dict(lens=None, period=0, ldx=K)
    if name == 'ldx':
        c['ldx'] = K + 8
    elif name == 'ragged':
        c.update(lens=np.array([5, 0, 8], np.int32), period=8)
    elif name == 'mixed':
        col = 2.0 ** rng.uniform(-3, 3, (1, K))
        x = (rng.randn(M, K) * 2.0 ** 12 * col).astype(F32)
        W = (rng.randn(P, K) * 2.0 ** -12 / col).astype(F32)
        b = (rng.randn(P) * np.sqrt(K)).astype(F32)
    elif name == 'ties':
        W = (0.1 * W).astype(F32)
        w = rng.randn(K).astype(F32)
        x = (x * np.sign(x.astype(np.float64) @ w.astype(np.float64))[:, None]).astype(F32)
        for p_ in TAG_TIE_CLASSES:
            W[p_], b[p_] = w, 8.0
    elif name == 'nan':
        x[2] = np.nan
    c.update(x=x, W=W, b=b)
    return c


# ---- dropout_scale ----------------------------------------------------------------------------------------------------------------------------------

def dropout_f64(x, keep, p):
    """y = x keep / (1 - p), p as the float32 the C ABI takes; S = |y|: 1 - p, the division and the two products round once each"""
    y = f64(x) * f64(keep) / (1.0 - float(F32(p)))
    return y, np.abs(y)


def dropout_f32(x, keep, p):
    scale = F32(1.0) / (F32(1.0) - F32(p))
    return (np.asarray(x, F32) * (np.asarray(keep, F32) * scale)).astype(F32)


DROPOUT_NS = (1, 3, 4, 1025)
DROPOUT_P = 0.33


def dropout_case(n):
    rng = np.random.RandomState(n)
    keep = (rng.rand(n) >= DROPOUT_P).astype(F32)
    if n >= 3:
        keep[0], keep[-1] = 0.0, 1.0
    return (rng.randn(n) * 2.0 ** rng.randint(-20, 20, n)).astype(F32), keep, rng.randn(n).astype(F32)
