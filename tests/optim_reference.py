"""Plain-numpy float64 statements of the AdamW step (csrc/train_ops.hip: adamw_flat_kernel behind ttsc_adamw_step, ttscube_amd/optim.py) and of the
training-side sums (bias_grad_kernel, rows_gather_kernel, rows_scatter_add_kernel, rows_segment_sum_kernel), the per-element bound a float32
evaluation of one AdamW step has to meet, a float32 restatement of the step as the yardstick, and generators of data on which a float32 sum cannot
round.  No import from ttscube_amd; checked without a GPU in tests/test_optim_reference_cpu.py, used by tests/test_adamw_f64_gpu.py and
tests/test_train_sums_f64_gpu.py.

The hyperparameters of a step.  The C ABI carries lr, beta1, beta2, eps and weight_decay as float32, so the step the kernel is asked for is the one
with THOSE values: `f32_hyper` rounds a Python setting to what the call carries, and the float64 statement is evaluated there.  (With beta2 = 0.99
the float32 value is 0.99 + 9.5e-9, and 1 - beta2 follows it: 16 u of 0.01.  That is a property of the interface, equal for every element and
every step, and no rounding of the kernel; torch's own float32 AdamW rounds 1 - beta2 instead of beta2.  The existing comparison with torch's
float32 optimizer in tests/test_training_gpu.py covers the difference between the two.)"""
import numpy as np

U = 2.0 ** -24                       # unit roundoff of float32
TINY = 2.0 ** -149                   # smallest subnormal
_UG = U / (1 - 16 * U)               # u with the second-order terms of up to 16 stacked roundings folded in (gamma_k = k u / (1 - k u))

PRODUCT = (2e-4, (0.8, 0.99), 1e-8, 1e-2)      # Cubegan.configure_optimizers: lr, betas, eps, weight_decay


# ---- AdamW: float64 statement ------------------------------------------------------------------------------------------------------------------

def f32_hyper(lr, betas, eps, weight_decay):
    """the setting as the C ABI carries it: every value rounded to float32, returned as Python floats"""
    r = lambda x: float(np.float32(x))
    return r(lr), (r(betas[0]), r(betas[1])), r(eps), r(weight_decay)


def true_scalars(step, lr, betas, eps, weight_decay):
    """the seven scalars of one step in float64"""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(decay=1.0 - lr * weight_decay, om_b1=1.0 - b1, b2=b2, om_b2=1.0 - b2, inv_bc2s=1.0 / np.sqrt(bc2), eps=eps, step_size=lr / bc1)


def adamw_step(p, g, m, v, step, lr, betas, eps, weight_decay):
    """torch's single-tensor AdamW (torch/optim/adamw.py::_single_tensor_adamw, the order ttscube_amd/optim.py cites) in float64:
    param.mul_(1 - lr wd); exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2);
    denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps; param.addcdiv_(exp_avg, denom, value=-lr / bc1).  Arrays in, (p, m, v) out."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    with np.errstate(over='ignore', invalid='ignore'):
        p = p * (1.0 - lr * weight_decay)
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + g * g * (1.0 - b2)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v


# ---- AdamW: the bound ----------------------------------------------------------------------------------------------------------------------------
# adamw_elem, operation by operation; fl() = one rounding of relative size <= u, scalars with a hat = the float32 word the host hands over.
#
#   m' = fl(m + fl(fl(g - m) * om_b1^))
C_M = 4    # difference 1 + scalar 1 + product 1, all on a term of size <= om_b1 (|g| + |m|) <= |g| + |m|; the sum 1 on |m'| <= |m| + |g|
#   v' = fl(fl(v * b2^) + fl(fl(om_b2^ * g) * g))        (torch's addcmul order: value * t1 * t2)
C_V = 4    # v b2: scalar 1 + product 1; g^2 om_b2: scalar 1 + two products 2; both terms are non-negative and add up to v', so the worse
#            of the two (3) holds for their sum; the sum itself 1.  Underflow: om_b2 * g, its product with g and v * b2 can each lose half a
#            subnormal spacing (2^-150) instead of a relative u, and a sum of subnormals is exact: 1.5 spacings in all — the issue's "plus the
#            smallest subnormal" with the three operations counted
C_V_TINY = 1.5
#   denom = fl(fl(sqrtf(v') * inv_bc2s^) + eps^)
C_D = 6    # sqrt halves v's 4 -> 2; the correctly rounded root 1 + scalar 1 + product 1 = 5 on sqrt(v') inv_bc2s <= denom; eps^ is carried
#            exactly; the sum 1 on denom.  (1.5 TINY in v' moves the root by at most 2^-74.2 = 4.5e-23 inv_bc2s: 4e-14 of an eps of 1e-8, where u is
#            6e-8 — inside the unit counted for b2^ in C_V, which the interface in fact carries exactly.)
#   p' = fl(fl(p * decay^) - fl(step_size^ * fl(m' / denom)))
C_P = 4    # decay^ = fl(1 - fl(lr wd)): 1 + lr wd / decay <= 2; product 1; the final difference 1 on its |p decay| share
C_Q = 10   # on step_size |m'| / denom: denom 6 + the correctly rounded quotient 1 + scalar 1 + product 1 + the final difference 1 on its share;
#            what m' itself carries comes in through |dm| / denom
# (-ffp-contract=off in csrc/Makefile keeps the kernel unfused; a contraction only removes roundings from this count.)


def adamw_step_bound(p, g, m, v, p1, m1, v1, scalars):
    """(bp, bm, bv): per element, how far a float32 evaluation of one step from the float32 state (p, g, m, v) may be from its float64 result
    (p1, m1, v1).  scalars = true_scalars(...) of that step."""
    p, g, m, v, p1, m1, v1 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v, p1, m1, v1))
    bm = C_M * _UG * (np.abs(m) + np.abs(g))
    bv = C_V * _UG * v1 + C_V_TINY * TINY
    denom = np.sqrt(v1) * scalars['inv_bc2s'] + scalars['eps']
    bp = C_P * _UG * np.abs(p) + scalars['step_size'] * (bm / denom + C_Q * _UG * np.abs(m1) / denom)
    return bp, bm, bv


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 counts as 0, a non-zero error against a zero bound as inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- AdamW: float32 restatement ------------------------------------------------------------------------------------------------------------------

def host_scalars(step, lr, betas, eps, weight_decay):
    """the seven float32 words ttsc_adamw_step_guarded computes on the host (float arithmetic on the float arguments; the two bias corrections in
    double, rounded once)"""
    f = np.float32
    lr_, b1, b2, eps_, wd = f(lr), f(betas[0]), f(betas[1]), f(eps), f(weight_decay)
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    return dict(decay=f(1) - lr_ * wd, om_b1=f(1) - b1, b2=b2, om_b2=f(1) - b2, inv_bc2s=f(1.0 / np.sqrt(bc2)), eps=eps_, step_size=f(float(lr_) / bc1))


def _fma(a, b, c):
    # float32 a * b is exact in float64; the sum rounds to double, then to float32 (the second rounding moves a float32 fma by at most a
    # double's ulp: immaterial for a restatement whose own error is what is measured)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adamw_step_f32(p, g, m, v, s, fused=False):
    """adamw_elem in numpy float32, every operation rounded; fused=True contracts the three multiply-adds a compiler may contract.
    s = host_scalars(...).  Returns float32 (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    one = lambda k: np.full(p.shape, s[k], dtype=f)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        p = p * s['decay']
        if fused:
            m = _fma(g - m, one('om_b1'), m)
            v = _fma(s['om_b2'] * g, g, v * s['b2'])
        else:
            m = m + (g - m) * s['om_b1']
            v = v * s['b2'] + (s['om_b2'] * g) * g
        denom = np.sqrt(v) * s['inv_bc2s'] + s['eps']
        q = m / denom
        p = _fma(-one('step_size'), q, p) if fused else p - s['step_size'] * q
    return p.astype(f), m.astype(f), v.astype(f)


# ---- AdamW: input families (shared by the CPU check of the bound and the GPU test) ---------------------------------------------------------------

def adamw_families(n, seed=0):
    """name -> dict(p, g, m, v float32 arrays of n elements, step, hyper = (lr, betas, eps, weight_decay) as set in Python)"""
    r = np.random.RandomState(seed)
    f = np.float32
    sign = lambda: r.choice([-1.0, 1.0], size=n)
    logu = lambda lo, hi: 10.0 ** r.uniform(lo, hi, size=n)
    lr, betas, eps, wd = PRODUCT
    fam = {}
    fam['zero_grad'] = dict(p=r.randn(n), g=np.zeros(n), m=np.zeros(n), v=np.zeros(n), step=3, hyper=PRODUCT)
    g = sign() * logu(-30, -20)
    fam['tiny_grad'] = dict(p=r.randn(n), g=g, m=sign() * logu(-30, -20), v=np.zeros(n), step=1, hyper=PRODUCT)
    g = sign() * logu(-12, 12)
    fam['wide_grad'] = dict(p=r.randn(n), g=g, m=g * r.uniform(-1, 1, size=n), v=(g * r.uniform(0.5, 2.0, size=n)) ** 2, step=1000, hyper=PRODUCT)
    fam['v_dominates'] = dict(p=r.randn(n), g=1e-3 * r.randn(n), m=1e-3 * r.randn(n), v=r.uniform(1e1, 1e2, size=n), step=7, hyper=PRODUCT)
    fam['g_dominates'] = dict(p=r.randn(n), g=sign() * r.uniform(0.5, 2.0, size=n), m=1e-3 * r.randn(n), v=r.uniform(1e-13, 1e-12, size=n), step=7,
                              hyper=PRODUCT)
    g, m = r.randn(n), 0.1 * r.randn(n)
    g[::5] = 0.0
    m[::5] = 0.0                                             # update exactly 0 there: p must stay as it is
    fam['no_decay'] = dict(p=r.randn(n), g=g, m=m, v=r.uniform(1e-3, 1.0, size=n), step=2, hyper=(lr, betas, eps, 0.0))
    fam['eps_dominates'] = dict(p=r.randn(n), g=1e-6 * r.randn(n), m=1e-6 * r.randn(n), v=r.uniform(1e-13, 1e-12, size=n), step=1000,
                                hyper=(lr, betas, 1e-3, wd))
    for c in fam.values():
        for k in 'pgmv':
            c[k] = c[k].astype(f)
    return fam


def random_state(n, seed):
    """generic float32 state of n elements: p, g ~ N(0, 1), m ~ 0.1 N(0, 1), v >= 0 of the size of g^2"""
    r = np.random.RandomState(seed)
    f = np.float32
    return (r.standard_normal(n).astype(f), r.standard_normal(n).astype(f), (0.1 * r.standard_normal(n)).astype(f),
            (r.standard_normal(n).astype(f) ** 2).astype(f))


def lr_at(lr0, t):
    """the learning rate after t completed steps, as networks/training.py sets it (Cubegan._compute_lr with delta = 1e-5)"""
    return lr0 / (1 + 1e-5 * t)


def trajectory(p0, grads, lr0, betas, eps, weight_decay, kind, first_step=1, m0=None, v0=None, every=None):
    """T steps from p0 (float32) with grads [T, n] (float32) and the decayed learning rate; kind 'f64' (the statement, at the float32 hyperparameters
    of every step), 'f32' or 'f32-fused' (the restatement).  Returns p after the last step (and the list of p at every `every`-th step)."""
    T = grads.shape[0]
    wide = kind == 'f64'
    dt = np.float64 if wide else np.float32
    p = np.asarray(p0, dtype=dt)
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, dtype=dt)
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, dtype=dt)
    snaps = []
    for t in range(T):
        step = first_step + t
        hyper = (lr_at(lr0, step - 1), betas, eps, weight_decay)
        if wide:
            p, m, v = adamw_step(p, grads[t], m, v, step, *f32_hyper(*hyper))
        else:
            p, m, v = adamw_step_f32(p, grads[t], m, v, host_scalars(step, *hyper), fused=kind == 'f32-fused')
        if every and step % every == 0:
            snaps.append(p.copy())
    return (p, snaps) if every else p


# ---- data on which a float32 sum does not round --------------------------------------------------------------------------------------------------

def exact_values(shape, terms, seed=0):
    """float32 values k / 64 with integer |k| <= K, K the largest with terms * K < 2^24: a sum of up to `terms` of them, in any order and with any
    grouping, is an integer multiple of 1/64 below 2^24 / 64 at every partial sum, hence exact in float32 — the float64 sum is the only right
    answer, bit for bit"""
    K = (2 ** 24 - 1) // int(terms)
    assert K >= 1 and int(terms) * K < 2 ** 24, (terms, K)
    k = np.random.RandomState(seed).randint(-K, K + 1, size=shape)
    return (k / 64.0).astype(np.float32)


# ---- the sums ----------------------------------------------------------------------------------------------------------------------------------

def bias_grad(dy):
    """db[c] = sum_{b, t} dy[b, c, t]"""
    return np.asarray(dy, dtype=np.float64).sum(axis=(0, 2))


def rows_gather(table, idx):
    """out[i, :] = table[idx[i], :]; an index outside [0, V) reads as a zero row"""
    table, idx = np.asarray(table, dtype=np.float64), np.asarray(idx)
    V = table.shape[0]
    ok = (idx >= 0) & (idx < V)
    out = np.zeros((idx.shape[0], table.shape[1]))
    out[ok] = table[idx[ok]]
    return out


def rows_scatter_add(gout, idx, V, skip_row=-1):
    """gtable[v, :] = sum_{i: idx[i] == v} gout[i, :]; row skip_row stays zero; rows no index names are zero"""
    gout, idx = np.asarray(gout, dtype=np.float64), np.asarray(idx)
    out = np.zeros((V, gout.shape[1]))
    for v in range(V):
        if v != skip_row:
            out[v] = gout[idx == v].sum(axis=0)
    return out


def rows_segment_sum(gout, idx_sorted, V):
    """the same sums for a non-decreasing index list (no skipped row)"""
    idx_sorted = np.asarray(idx_sorted)
    assert np.all(np.diff(idx_sorted) >= 0)
    return rows_scatter_add(gout, idx_sorted, V, -1)


def rows_abs_sum(gout, idx, V, skip_row=-1):
    return rows_scatter_add(np.abs(np.asarray(gout, dtype=np.float64)), idx, V, skip_row)


def rows_depth(idx, V):
    """per table row: the number of list entries that name it = the length of its one chain of additions"""
    idx = np.asarray(idx)
    return np.array([int((idx == v).sum()) for v in range(V)])


# ---- the summation order of bias_grad_kernel (restated from csrc/train_ops.hip, not imported) ------------------------------------------------------

def bias_grad_splits(B, C, L):
    s = (L + 1023) // 1024                 # >= 1024 positions of every batch item per block
    cap = (1024 + C - 1) // C              # ~1024 blocks in all
    return max(1, min(s, cap))


def bias_grad_depth(B, C, L):
    """(d, S): the longest chain of additions behind one output.  A block sums n = B * w values (w = its slice of L, at most per = ceil(L / S)):
    thread t adds a0 once per trip of the four-way loop (i + 768 < n, i += 1024) and once per trip of the remainder loop (i < n, i += 256); then the
    2 joins (a0 + a1) + (a2 + a3), 6 shuffle levels, the 4 waves, and the S partials in index order."""
    S = bias_grad_splits(B, C, L)
    per = (L + S - 1) // S
    n = B * per
    trips = 0
    for t in range(256):
        i, k = t, 0
        while i + 768 < n:
            i += 1024
            k += 1
        while i < n:
            i += 256
            k += 1
        trips = max(trips, k)
    return trips + 2 + 6 + 4 + S, S
