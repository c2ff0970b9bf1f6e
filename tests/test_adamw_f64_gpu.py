"""GPU: the AdamW step (csrc/train_ops.hip: adamw_flat_kernel behind ttsc_adamw_step / ttsc_adamw_step_guarded) and ttscube_amd/optim.py::FlatAdamW
against the float64 statement of tests/optim_reference.py (checked without a GPU in tests/test_optim_reference_cpu.py).

One step, straight through the C ABI: per element |got - ref64| <= adamw_step_bound — the operations of adamw_elem counted, one unit roundoff each —
at every n the index arithmetic distinguishes (the scalar tail n & 3, the second trip of the grid-stride loop above 2048 * 256 * 4 elements), at
resumed step counts, and on the input families where float32 is at its edges.  Long runs through FlatAdamW: against the float64 trajectory, at most
4 x the deviation of the float32 restatement on the same gradients plus 1e-7 * lr * steps (the yardstick rule of tests/test_mel_loss_f64_gpu.py).

Measured on an MI355X, worst error / bound (p, m, v): the figures this file prints are recorded in DESIGN.md section 2d."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0                      # tests/test_mel_loss_f64_gpu.py
SENT = -777.25                    # sentinel around every arena
NS = (1, 2, 3, 4, 5, 7, 1021, 1024, 1027, 2097152, 2097156, 2097159, 5000003)
STEPS = (1, 2, 1000, 1000000)
_STATE = {}


def _state(n):
    if n not in _STATE:
        if n > 4099:                      # (two large states at a time are enough: the cases come n by n)
            for k in [k for k in _STATE if k > 4099]:
                del _STATE[k]
        _STATE[n] = R.random_state(n, seed=n % 1009)
    return _STATE[n]


def _arena(x, lead=4):
    """a device view that starts `lead` elements into a sentinel-filled tensor and ends 4 before its end"""
    n = x.shape[0]
    big = torch.full((n + lead + 4,), SENT, dtype=torch.float32, device='cuda')
    big[lead:lead + n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return big, big[lead:lead + n]


def _sentinels_ok(big, n, lead=4):
    return bool((big[:lead] == SENT).all()) and bool((big[lead + n:] == SENT).all())


def _launch(views, n, hyper, step, guard=None, plain=True):
    from ttscube_amd import _lib
    L = _lib.lib()
    lr, (b1, b2), eps, wd = hyper
    ptr = lambda t: None if t is None else _lib.dev_ptr(t)
    args = [ptr(t) for t in views] + [n, lr, b1, b2, eps, wd, step]
    if guard is None and plain:
        return L.ttsc_adamw_step(*args, _lib.current_stream())
    return L.ttsc_adamw_step_guarded(*args, None if guard is None else guard.data_ptr(), _lib.current_stream())


def _one_step(p, g, m, v, hyper, step, guard=None, plain=True):
    """-> float32 numpy (p, m, v) after one launch over sentinel-wrapped arenas; asserts the sentinels and that g is left alone"""
    n = p.shape[0]
    bigs, views = zip(*[_arena(x) for x in (p, g, m, v)])
    rc = _launch(views, n, hyper, step, guard, plain)
    assert rc == 0
    torch.cuda.synchronize()
    for b in bigs:
        assert _sentinels_ok(b, n)
    assert torch.equal(views[1].cpu(), torch.from_numpy(g))
    return views[0].cpu().numpy(), views[2].cpu().numpy(), views[3].cpu().numpy()


def _check(label, p, g, m, v, hyper, step, got):
    h32 = R.f32_hyper(*hyper)
    ref = R.adamw_step(p, g, m, v, step, *h32)
    bound = R.adamw_step_bound(p, g, m, v, *ref, R.true_scalars(step, *h32))
    ratios = [R.worst_ratio(a, b, c) for a, b, c in zip(got, ref, bound)]
    print('ADAMW %s: worst error / bound  p %.3f  m %.3f  v %.3f' % (label, *ratios))
    for name, a, r in zip('pmv', got, ratios):
        assert np.all(np.isfinite(a)) and r <= 1.0, '%s %s: error / bound %.3f' % (label, name, r)
    return ref, bound


# ---- 1. every n the index arithmetic distinguishes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('step', STEPS)
@pytest.mark.parametrize('n', NS)
def test_one_step_at_every_length_and_step_count(n, step):
    p, g, m, v = _state(n)
    got = _one_step(p, g, m, v, R.PRODUCT, step)
    _check('n=%d step=%d' % (n, step), p, g, m, v, R.PRODUCT, step, got)


# ---- 2. input families ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', ['zero_grad', 'tiny_grad', 'wide_grad', 'v_dominates', 'g_dominates', 'no_decay', 'eps_dominates'])
def test_one_step_on_the_input_families(family):
    c = R.adamw_families(4099, seed=5)[family]
    p, g, m, v = c['p'], c['g'], c['m'], c['v']
    got = _one_step(p, g, m, v, c['hyper'], c['step'])
    ref, bound = _check(family, p, g, m, v, c['hyper'], c['step'], got)
    if family == 'zero_grad':            # the update is exactly 0: both moments stay 0, p = p * decay within c_p u |p|
        assert not got[1].any() and not got[2].any()
        decay = R.true_scalars(c['step'], *R.f32_hyper(*c['hyper']))['decay']
        assert np.all(np.abs(got[0] - p.astype(np.float64) * decay) <= R.C_P * R.U * np.abs(p))
    if family == 'no_decay':             # the decay factor is exactly 1: where the update is 0, p keeps its bits
        still = (g == 0) & (m == 0)
        assert still.sum() > 800 and np.array_equal(got[0][still], p[still])
        assert (got[0][~still] != p[~still]).mean() > 0.9
    if family == 'eps_dominates':
        s = R.true_scalars(c['step'], *R.f32_hyper(*c['hyper']))
        assert np.all(np.sqrt(ref[2]) * s['inv_bc2s'] < 1e-2 * s['eps'])


# ---- 3. outside float32's range: stated, not bounded ------------------------------------------------------------------------------------------------

def test_a_gradient_whose_square_overflows_behaves_as_torch_float32_adamw_on_the_cpu():
    """|g| = 1e20: g * g is infinite in float32, (1 - beta2) * g * g = 1e38 is not.  torch's single-tensor AdamW on the CPU evaluates addcmul as
    value * t1 * t2 and keeps v finite there; the kernel multiplied g * g first and returned v = inf and no update until this test (it now keeps
    torch's order).  At |g| = 3e20 the term itself is beyond float32: the CPU run gives v = inf, an update of 0 and p = p * decay, and so must the
    kernel.  Every expectation below is asserted of the CPU run first."""
    n, k, kk = 4099, 1002, 2051
    lr, betas, eps, wd = R.PRODUCT
    p, g, _, _ = R.random_state(n, seed=11)
    g = g.copy()
    g[k], g[kk] = 1e20, -3e20
    zero = np.zeros(n, dtype=np.float32)
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    q.grad = torch.from_numpy(g.copy())
    opt.step()
    tm, tv, tp = opt.state[q]['exp_avg'].numpy(), opt.state[q]['exp_avg_sq'].numpy(), q.detach().numpy()
    got = _one_step(p, g, zero, zero, R.PRODUCT, 1)
    # 3e20, what the CPU run gives: v = +inf, the update 0, p = p * decay (torch multiplies by the float32 rounding of 1 - lr wd), m finite
    assert np.isinf(tv[kk]) and tv[kk] > 0 and np.isfinite(tv).sum() == n - 1 and np.isfinite(tm[kk])
    assert tp[kk] == np.float32(p[kk]) * np.float32(1 - lr * wd)
    assert np.isinf(got[2][kk]) and got[2][kk] > 0
    decay = R.true_scalars(1, *R.f32_hyper(*R.PRODUCT))['decay']
    assert abs(float(got[0][kk]) - float(p[kk]) * decay) <= R.C_P * R.U * abs(float(p[kk]))
    assert abs(float(got[0][kk]) - float(tp[kk])) <= R.C_P * R.U * abs(float(p[kk]))
    assert abs(float(got[1][kk]) - float(tm[kk])) <= R.C_M * R.U * 3e20
    # 1e20, what the CPU run gives: v = 1e38, finite, and a full first-step update of lr against the sign of g
    assert np.isfinite(tv[k]) and abs(float(tv[k]) / 1e38 - 1) < 1e-6 and abs((float(tp[k]) - float(p[k]) * decay) / -lr - 1) < 1e-3
    # (the kernel's 1 - beta2 follows the float32 beta2 the interface carries, torch rounds 1 - beta2 itself: 16 u of 0.01 between the two v, see
    # tests/optim_reference.py; the bound below is against float64 at the interface's values)
    assert np.isfinite(got[2][k]) and abs(float(got[2][k]) - float(tv[k])) <= (16 + 2 * R.C_V) * R.U * 1e38
    # ... and every finite element, that one included, is inside the bound of the float64 step
    rest = np.arange(n) != kk
    _check('|g| = 1e20 and the other elements', p[rest], g[rest], zero[rest], zero[rest], R.PRODUCT, 1, [a[rest] for a in got])


def test_a_nan_gradient_reaches_its_own_element_and_no_other():
    n = 4099
    p, g, m, v = R.random_state(n, seed=12)
    clean = _one_step(p, g, m, v, R.PRODUCT, 5)
    bad = g.copy()
    hit = [1001, 4097]                   # the second word of a 16-byte group; the middle of the scalar tail
    bad[hit] = np.nan
    bigs, views = zip(*[_arena(x) for x in (p, bad, m, v)])
    assert _launch(views, n, R.PRODUCT, 5) == 0
    torch.cuda.synchronize()
    got = [views[i].cpu().numpy() for i in (0, 2, 3)]
    rest = np.ones(n, dtype=bool)
    rest[hit] = False
    for a, b in zip(got, clean):
        assert np.isnan(a[hit]).all()
        assert np.array_equal(a[rest], b[rest])       # the three neighbours in the group included
    assert all(_sentinels_ok(b, n) for b in bigs)


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch():
    n = 1027
    x = np.full(n, 3.5, dtype=np.float32)
    for what in ('n=0', 'step=0', 'null p', 'null g', 'null m', 'null v', 'offset p', 'offset g', 'offset m', 'offset v'):
        for plain in (True, False):
            lead = [4, 4, 4, 4]
            if what.startswith('offset'):
                lead['pgmv'.index(what[-1])] = 5             # one element off the 16-byte boundary
            bigs, views = zip(*[_arena(x, l) for l in lead])
            before = [b.clone() for b in bigs]
            args = list(views)
            if what.startswith('null'):
                args['pgmv'.index(what[-1])] = None
            rc = _launch(args, 0 if what == 'n=0' else n, R.PRODUCT, 0 if what == 'step=0' else 1, plain=plain)
            torch.cuda.synchronize()
            assert rc != 0, what
            for b, b0 in zip(bigs, before):
                assert torch.equal(b, b0), what


@pytest.mark.parametrize('n', [n for n in NS if n % 2])
def test_guarded_entry_has_the_plain_bits_on_a_zero_word_and_does_nothing_on_a_set_one(n):
    p, g, m, v = _state(n)
    plain = _one_step(p, g, m, v, R.PRODUCT, 3)
    word = torch.zeros(1, dtype=torch.int32, device='cuda')
    guarded = _one_step(p, g, m, v, R.PRODUCT, 3, guard=word)
    for a, b in zip(plain, guarded):
        assert np.array_equal(a, b)
    null_word = _one_step(p, g, m, v, R.PRODUCT, 3, plain=False)
    for a, b in zip(plain, null_word):
        assert np.array_equal(a, b)
    word.fill_(4)
    skipped = _one_step(p, g, m, v, R.PRODUCT, 3, guard=word)
    for a, b in zip(skipped, (p, m, v)):
        assert np.array_equal(a, b)


# ---- FlatAdamW with injected gradients ------------------------------------------------------------------------------------------------------------

SHAPES = [(1,), (3,), (63,), (64,), (65,), (129,), (4096,), (5000,), (37, 129), (5, 129), (16, 3, 7), (2, 3, 5)]
SCALES = [1.0, 1e-3, 30.0, 1e-2, 1.0, 1e-5, 0.1, 1.0, 1e-2, 3.0, 1e-4, 1.0]       # gradient scale per parameter


def _drawn(steps, seed):
    """initial parameters and `steps` gradients per parameter, drawn in advance (they do not depend on the parameters: the recurrence does not
    amplify rounding chaotically) -> p0 [total], grads [steps, total], slices"""
    r = np.random.RandomState(seed)
    sizes = [int(np.prod(s)) for s in SHAPES]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    p0 = r.standard_normal(offs[-1]).astype(np.float32)
    grads = r.standard_normal((steps, offs[-1])).astype(np.float32)
    for k, sc in enumerate(SCALES):
        grads[:, offs[k]:offs[k + 1]] *= np.float32(sc)
    return p0, grads, [slice(int(offs[k]), int(offs[k + 1])) for k in range(len(sizes))]


def _params(p0, sl):
    return [torch.nn.Parameter(torch.from_numpy(p0[s].reshape(shape).copy()).cuda()) for s, shape in zip(sl, SHAPES)]


def _set_grads(ps, G, t, sl):
    for p, s in zip(ps, sl):
        p.grad = G[t, s].view(p.shape)


def _flat(ps):
    return np.concatenate([p.detach().reshape(-1).cpu().numpy() for p in ps])


def _padding_mask(opt):
    pad = np.ones(opt.p.numel(), dtype=bool)
    for i, o in zip(opt.live, opt.offsets):
        pad[o:o + opt.params[i].numel()] = False
    return torch.from_numpy(pad).cuda()


def _check_trajectory(label, got, p0, grads, sl, lr0, steps):
    """per parameter: max |got - f64| <= 4 x max |f32 restatement - f64| + 1e-7 * lr * steps"""
    _, betas, eps, wd = R.PRODUCT
    ref = R.trajectory(p0, grads[:steps], lr0, betas, eps, wd, 'f64')
    yard = R.trajectory(p0, grads[:steps], lr0, betas, eps, wd, 'f32')
    floor = 1e-7 * lr0 * steps
    worst = 0.0
    for k, s in enumerate(sl):
        ek, ey = float(np.abs(got[s] - ref[s]).max()), float(np.abs(yard[s].astype(np.float64) - ref[s]).max())
        worst = max(worst, ek / max(ey, 1e-300))
        print('TRAJ %s %s: kernel %.3e  yardstick %.3e  floor %.1e' % (label, SHAPES[k], ek, ey, floor))
        assert np.all(np.isfinite(got[s])) and ek <= FACTOR * ey + floor, '%s %s: %.3e > 4 x %.3e + %.1e' % (label, SHAPES[k], ek, ey, floor)
    print('TRAJ %s: worst kernel / yardstick deviation %.3f over %d steps' % (label, worst, steps))


def test_three_hundred_steps_through_flat_adamw_stay_with_the_float64_trajectory():
    from ttscube_amd.optim import FlatAdamW
    steps = 300
    lr0, betas, eps, wd = R.PRODUCT
    p0, grads, sl = _drawn(steps, seed=21)
    ps = _params(p0, sl)
    G = torch.from_numpy(grads).cuda()
    opt = FlatAdamW(ps, lr=lr0, betas=betas, eps=eps, weight_decay=wd)
    pad = None
    for t in range(steps):
        opt.zero_grad()
        _set_grads(ps, G, t, sl)
        opt.step()
        opt.param_groups[0]['lr'] = R.lr_at(lr0, t + 1)
        if (t + 1) % 50 == 0:
            pad = _padding_mask(opt) if pad is None else pad
            assert int(pad.sum()) > 300
            for name in 'pgmv':
                assert not bool(getattr(opt, name)[pad].any()), (name, t + 1)
    assert opt.live == list(range(len(SHAPES)))
    _check_trajectory('FlatAdamW', _flat(ps), p0, grads, sl, lr0, steps)


# ---- 6. gather ------------------------------------------------------------------------------------------------------------------------------------

def test_gather_brings_every_kind_of_gradient_into_the_arena_whole_and_in_chunks():
    from ttscube_amd.optim import FlatAdamW
    p0, grads, sl = _drawn(3, seed=22)
    ps = _params(p0, sl)
    G = torch.from_numpy(grads).cuda()
    opt = FlatAdamW(ps, lr=1e-3)
    _set_grads(ps, G, 0, sl)
    opt.step()                                     # lays the arenas out
    offs, numel = opt.offsets, opt.numel
    g_ = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=g_).cuda()

    KINDS = ['fresh', 'transposed', 'expanded', 'none', 'arena', 'fresh', 'arena', 'expanded', 'transposed', 'none', 'expanded', 'transposed']

    def kinds(none_at):
        """a gradient of some kind per parameter -> the expected arena content"""
        want = torch.zeros(opt.g.numel())
        for k, p in enumerate(ps):
            kind = KINDS[k] if k not in none_at else 'none'
            if kind == 'fresh':
                p.grad = rnd(*p.shape)
            elif kind == 'transposed':
                p.grad = rnd(*reversed(p.shape)).permute(*reversed(range(p.dim())))
                assert p.dim() < 2 or not p.grad.is_contiguous()
            elif kind == 'expanded':
                p.grad = rnd(*([1] * p.dim())).expand(p.shape)
                assert p.numel() == 1 or p.grad.stride()[-1] == 0
            elif kind == 'arena':
                view = opt._gviews[k]
                view.copy_(rnd(*p.shape))
                p.grad = view
            else:
                p.grad = None
            if p.grad is not None:
                want[offs[k]:offs[k] + p.numel()] = p.grad.detach().reshape(-1).cpu()
        return want

    def scribble():
        """garbage wherever gather() has to write: every parameter's range but the one whose gradient already IS the arena view"""
        for k, p in enumerate(ps):
            if p.grad is not opt._gviews[k]:
                opt.g[offs[k]:offs[k] + p.numel()] = 7.0

    opt.zero_grad()
    want = kinds(none_at=())
    assert sum(p.grad is None for p in ps) >= 2 and sum(p.grad is opt._gviews[k] for k, p in enumerate(ps)) >= 2
    scribble()
    opt.gather()
    whole = opt.g.clone()
    assert torch.equal(whole.cpu(), want)            # the gradients' values, zeros for None, zeros in the padding
    k2 = SHAPES.index((37, 129))
    # at a parameter start (3, 7); inside a parameter: the arena view (6), the expanded (7), the transposed (8), the one without a gradient (9);
    # inside the padding behind 5 and behind 8
    cuts = sorted({0, offs[3], offs[7], offs[6] + 64 * 17 + 5, offs[7] + 2500, offs[k2] + 1000, offs[9] + 100, offs[5] + 129 + 3,
                   offs[k2] + 37 * 129 + 11, numel})
    for bounds in (cuts, list(range(0, numel, 64 * 29)) + [numel], list(range(0, numel, 64)) + [numel]):
        scribble()
        for s, e in zip(bounds[:-1], bounds[1:]):
            opt.gather(s, e)
        assert torch.equal(opt.g, whole), bounds[:4]
    # the next step: parameters that had a gradient have None now -> zeros, not the earlier gradient
    opt.grads_in_arena()
    opt.step()
    opt.zero_grad()
    want = kinds(none_at=(0, 6, k2))                 # a fresh one, an arena view and the transposed matrix of the step before
    opt.gather()
    assert torch.equal(opt.g.cpu(), want)
    for k in (0, 6, k2):
        assert not bool(opt.g[offs[k]:offs[k] + ps[k].numel()].any())


def _no_gather_child(out_path):
    """(child process, TTSC_GRAD_GATHER=0) 20 steps with autograd accumulating into the standing arena views; writes the parameters"""
    from ttscube_amd import optim
    assert not optim.GATHER_GRADS
    lr0, betas, eps, wd = R.PRODUCT
    p0, grads, sl = _drawn(20, seed=23)
    ps = _params(p0, sl)
    G = torch.from_numpy(grads).cuda()
    opt = optim.FlatAdamW(ps, lr=lr0, betas=betas, eps=eps, weight_decay=wd)
    for t in range(20):
        opt.zero_grad()
        sum((p * G[t, s].view(p.shape)).sum() for p, s in zip(ps, sl)).backward()        # d/dp = the drawn gradient
        if t > 0:
            assert all(p.grad is v for p, v in zip(ps, opt._gviews))                     # the standing views, accumulated into
        opt.step()
        opt.param_groups[0]['lr'] = R.lr_at(lr0, t + 1)
    np.save(out_path, _flat(ps))


def test_standing_arena_views_without_gather_stay_with_the_float64_trajectory(tmp_path):
    """TTSC_GRAD_GATHER=0 is read at import: the path runs in a process of its own"""
    out = str(tmp_path / 'p.npy')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'import sys; from tests.test_adamw_f64_gpu import _no_gather_child; _no_gather_child(sys.argv[1])'
    run = subprocess.run([sys.executable, '-c', code, out], env=dict(os.environ, TTSC_GRAD_GATHER='0'), cwd=root, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    p0, grads, sl = _drawn(20, seed=23)
    _check_trajectory('no-gather', np.load(out), p0, grads, sl, R.PRODUCT[0], 20)


# ---- 7. resuming ----------------------------------------------------------------------------------------------------------------------------------

def test_a_resumed_optimizer_carries_the_bits_of_the_uninterrupted_one():
    from ttscube_amd.optim import FlatAdamW
    lr0, betas, eps, wd = R.PRODUCT
    p0, grads, sl = _drawn(60, seed=24)
    G = torch.from_numpy(grads).cuda()
    ps = _params(p0, sl)
    opt = FlatAdamW(ps, lr=lr0, betas=betas, eps=eps, weight_decay=wd)

    def moments(state):
        return tuple(np.concatenate([state['state'][k][key].reshape(-1).cpu().numpy() for k in range(len(SHAPES))]) for key in ('exp_avg', 'exp_avg_sq'))

    def run(o, params, t0, t1):
        out = []
        for t in range(t0, t1):
            o.zero_grad()
            _set_grads(params, G, t, sl)
            o.step()
            out.append((_flat(params), ) + (moments(o.state_dict()) if t == t0 else ()))
        return out

    run(opt, ps, 0, 40)
    sd = opt.state_dict()
    assert all(float(e['step']) == 40.0 for e in sd['state'].values()) and len(sd['state']) == len(SHAPES)
    at40 = _flat(ps)
    m40, v40 = moments(sd)
    # through torch's optimizer and back
    qs = _params(at40, sl)
    to = torch.optim.AdamW(qs, lr=1.0)
    to.load_state_dict({'state': sd['state'], 'param_groups': [dict(sd['param_groups'][0], params=list(range(len(SHAPES))))]})
    sd_t = to.state_dict()
    resumed = []
    for state in (sd, sd_t):
        rs = _params(at40, sl)
        o = FlatAdamW(rs, lr=1.0)                       # every setting comes from the state
        o.load_state_dict(state)                        # before its arenas exist
        assert not o.built
        resumed.append(run(o, rs, 40, 60))
        assert o.step_count == 60 and o.param_groups[0]['lr'] == lr0 and tuple(o.param_groups[0]['betas']) == betas
    straight = run(opt, ps, 40, 60)
    for other in resumed:
        for t, (a, b) in enumerate(zip(straight, other)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b), 41 + t
    # step 41 is the float64 step with step = 41 from the float32 state at 40
    # (a resume that restarted the bias correction at 1 leaves this bound by three orders of magnitude: tests/test_optim_reference_cpu.py)
    _check('resumed, step 41', at40, grads[40], m40, v40, R.PRODUCT, 41, resumed[0][0])


# ---- 8. stragglers --------------------------------------------------------------------------------------------------------------------------------

def test_a_parameter_with_its_first_gradient_after_the_layout_raises():
    from ttscube_amd import _lib
    from ttscube_amd.optim import FlatAdamW
    a, b = (torch.nn.Parameter(torch.randn(n).cuda()) for n in (70, 5))
    opt = FlatAdamW([a, b], lr=1e-3)
    a.grad = torch.randn(70).cuda()
    opt.step()
    assert opt.live == [0]
    b0 = b.detach().clone()
    opt.zero_grad()
    a.grad = torch.randn(70).cuda()
    b.grad = torch.randn(5).cuda()
    assert opt.step_count < 4
    with pytest.raises(_lib.TTSCError, match='first gradient after'):
        opt.step()
    assert torch.equal(b.detach(), b0)

