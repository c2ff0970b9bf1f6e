"""The yardstick of tests/test_text_train_f64_gpu.py, checked without a GPU (tests/text_train_reference.py): on every case the GPU test runs,
the per-element bound |got - ref64| <= tau * S accepts the float32 host model of each operation with a factor 4 to spare (tau is 4 x its worst
err / S, rounded up to a power of two) — and rejects each defect a kernel of this family can plausibly have, on a named case.  The dispatch
arithmetic the cases are placed around (the grid caps of the loss kernels) is asserted against the C side, without a launch."""
import numpy as np
import pytest

from tests import text_train_reference as R

WORST = {}
NOTED = {}
# how many results of each operation the accepting tests of this file measure when all of them run
NOTED_WHEN_COMPLETE = {'bn_y': 10, 'bn_stats': 40, 'bn_dx': 10, 'bn_dparam': 20, 'ce_value': 136, 'ce_grad': 144, 'l1_value': 8, 'l1_grad': 8,
                       'tag_logits': 10, 'dropout': 16}


def _ratio(op, got, ref, S):
    r = R.worst_ratio(got, np.asarray(ref, np.float64), np.asarray(S, np.float64))
    WORST[op] = max(WORST.get(op, 0.0), r)
    NOTED[op] = NOTED.get(op, 0) + 1
    return r


def _ok(op, got, ref, S):
    _ratio(op, got, ref, S)
    return R.within(got, np.asarray(ref, np.float64), np.asarray(S, np.float64), R.TAU[op])


# ---- BatchNorm -> tanh -> dropout ----------------------------------------------------------------------------------------------------------------

def _bn(B, F, defect=None):
    c = R.bn_case(B, F)
    ref = R.bn_f64(**c)
    got = R.bn_f32(defect=defect, **c)
    return c, ref, got


def _bn_bad(ref, got):
    return [k for k in ref if not R.within(got[k], ref[k][0], ref[k][1], R.TAU[R.BN_GROUP[k]])]


@pytest.mark.parametrize('B,F', R.BN_SHAPES)
def test_bn_bound_accepts_float32_in_every_regime(B, F):
    c, ref, got = _bn(B, F)
    for k in ref:
        assert _ok(R.BN_GROUP[k], got[k], *ref[k]), (k, R.log2_ratio(R.worst_ratio(got[k], *ref[k])))
        assert R.worst_ratio(got[k], *ref[k]) <= R.TAU[R.BN_GROUP[k]] / 4, k
    # the exact zeros: dropped values, and everything gamma = 0 multiplies
    assert np.array_equal(got['y'] == 0, c['mask'] == 0)
    assert not got['dx'][:, 4].any() and not ref['dx'][1][:, 4].any()


@pytest.mark.parametrize('B,F', [(3, 8), (5, 7)])
def test_bn_bound_accepts_float32_under_the_philox_masks_of_the_gpu_cases(B, F):
    mask = R.bn_philox_mask(B, R.BN_C, F, R.BN_P, 0x1234567887654321, 2)
    assert 0 < (mask == 0).sum() < mask.size
    c = R.bn_case(B, F, mask=mask)
    ref, got = R.bn_f64(**c), R.bn_f32(**c)
    for k in ref:
        assert _ok(R.BN_GROUP[k], got[k], *ref[k]) and R.worst_ratio(got[k], *ref[k]) <= R.TAU[R.BN_GROUP[k]] / 4, k


def test_bn_companions_follow_the_condition_of_each_channel():
    """S / |ref| per channel: ~1 where the expression is well conditioned, large where float32 cannot do better (|mean| >> std)"""
    c, ref, _ = _bn(3, 8)
    inv, S_inv = ref['invstd']
    assert S_inv[0] / inv[0] < 16 and S_inv[2] / inv[2] < 4 and S_inv[5] / inv[5] < 4
    assert S_inv[1] / inv[1] > 1e4                                           # var = 1e-4 out of values near 1e3
    y, S_y = ref['y']
    kept = c['mask'] != 0
    assert (S_y[~kept] == 0).all() and (S_y[kept] > 0).all()
    assert np.allclose(S_y[:, 4][kept[:, 4]], (0.25 + np.tanh(0.25)) / 0.9, rtol=1e-6)      # gamma = 0: k (|beta| + |t|), whatever x is


@pytest.mark.parametrize('defect,B,F,seen_in', [
    ('var_e2', 2, 1028, 'invstd'), ('var_e2', 3, 8, 'invstd'), ('biased_rvar', 3, 8, 'rvar'), ('biased_rvar', 1, 2, 'rvar'),
    ('eps_outside', 3, 8, 'invstd'), ('no_scale', 5, 7, 'y'), ('no_scale', 1, 4, 'y'), ('mask_scalar_index', 3, 8, 'y'),
    ('mask_scalar_index', 2, 1028, 'y'), ('no_c2', 3, 8, 'dx'), ('no_c2', 5, 7, 'dx'), ('dgamma_from_x', 3, 8, 'dgamma'),
    ('dgamma_from_x', 2, 1, 'dgamma'), ('stats_rows_only', 3, 8, 'mean'), ('stats_rows_only', 1, 1025, 'rvar')])
def test_bn_bound_rejects(defect, B, F, seen_in):
    c, ref, got = _bn(B, F, defect)
    assert seen_in in _bn_bad(ref, got)


def test_bn_defects_only_some_cases_see():
    # the large-offset channel alone carries E[x^2] - E[x]^2: without it the defect passes at these sizes
    c = R.bn_case(3, 8)
    ref, got = R.bn_f64(**c), R.bn_f32(defect='var_e2', **c)
    err = ~(np.abs(got['invstd'].astype(np.float64) - ref['invstd'][0]) <= R.TAU['bn_stats'] * ref['invstd'][1])      # (NaN: a negative variance)
    assert err[1] and not err[[0, 3, 4]].any()
    # the mask index of the float4 walk: a scalar shape never takes it
    for B, F in ((5, 7), (1, 1025), (2, 1), (1, 2)):
        _, ref, got = _bn(B, F, 'mask_scalar_index')
        assert not _bn_bad(ref, got)


def test_bn_philox_mask_rebuild_has_the_documented_statistics():
    m = R.bn_philox_mask(3, R.BN_C, 8, 0.1, 1234, 2)
    assert m.shape == (3, R.BN_C, 8) and set(np.unique(m)) <= {0.0, 1.0}
    big = R.philox_keep(1 << 14, 0.1, 1234, 2, R.TC_BN_TAG)
    assert 0.88 < big.mean() < 0.92
    assert np.array_equal(big[:144], m.reshape(-1))                           # one stream over the flat element index
    assert np.array_equal(R.philox_keep(64, 0.1, 1234, 2, R.TC_BN_TAG, first=100), big[100:164])
    other = R.philox_keep(1 << 14, 0.1, 1234, 3, R.TC_BN_TAG)
    assert not np.array_equal(other, big) and not np.array_equal(R.dropout_philox_mask(1 << 14, 0.1, 1234, 2), big)
    assert R.philox_keep(256, 0.0, 5, 0, R.GT_TAG_DROP).all()


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------------------------------

def _ce_cases():
    for K in R.CE_KS:
        for head, rows in R.CE_ROWS.items():
            for Rn in rows:
                for inside in (False, True):
                    yield head, K, Rn, inside


@pytest.mark.parametrize('K', R.CE_KS)
def test_ce_bound_accepts_float32(K):
    for head, K_, Rn, inside in _ce_cases():
        if K_ != K:
            continue
        empty = 'zero' if head == 'masked' else 'nan'
        x, t, ignore = R.ce_case(Rn, K, inside)
        v, S_v, g, S_g = R.ce_f64(x, t, ignore, empty)
        gv, gg = R.ce_f32(x, t, ignore, empty)
        if np.isnan(v):
            assert np.isnan(gv) and K == 1 and inside
        else:
            assert _ok('ce_value', gv, v, S_v) and R.worst_ratio(gv, v, S_v) <= R.TAU['ce_value'] / 4, (head, Rn, inside)
        assert _ok('ce_grad', gg, g, S_g) and R.worst_ratio(gg, g, S_g) <= R.TAU['ce_grad'] / 4, (head, Rn, inside)
        assert not gg[~R.ce_valid(t, K, ignore)].any()


def test_ce_cases_hold_what_they_are_meant_to():
    x, t, ignore = R.ce_case(2049, 201, False)
    valid = R.ce_valid(t, 201, ignore)
    assert 0.25 < 1 - valid.mean() < 0.42 and (t[valid] == 200).sum() > 100
    assert np.abs(x[1::3]).max() > 250 and (np.sort(x[2::3], axis=1)[:, -2] == -80).all() and (x[2::3].max(1) == 80).all()
    _, _, g, _ = R.ce_f64(x, t, ignore)
    assert (np.abs(g[valid]) < 1e-60).mean() > 0.3                           # probabilities float32 cannot hold: most of two rows in three
    x, t, ignore = R.ce_case(7, 1, True)
    assert not R.ce_valid(t, 1, ignore).any()                                # K = 1 with ignore_index 0: no valid row, both conventions
    assert np.isnan(R.ce_f64(x, t, ignore, 'nan')[0]) and R.ce_f64(x, t, ignore, 'zero')[0] == 0.0
    assert R.ce_valid(R.ce_case(1, 65, True)[1], 65, 0).all()
    x, t, ignore = R.ce_case(1025, 7, False, bad_row=1024)
    assert t[1024] == 9 and not R.ce_valid(t, 7, ignore)[1024]


@pytest.mark.parametrize('defect,head,Rn,K,inside', [
    ('mean_all_rows', 'pitch', 2049, 65, False), ('mean_all_rows', 'dur', 1023, 7, True),
    ('no_max', 'masked', 2047, 201, False), ('no_max', 'dur', 1024, 63, True), ('onehot_tm1', 'masked', 1, 64, False),
    ('onehot_tm1', 'pitch', 2048, 7, True), ('skip_rows', 'dur', 1025, 7, False), ('skip_rows', 'pitch', 2049, 64, True),
    ('skip_rows', 'masked', 2049, 201, False), ('ignored_unwritten', 'masked', 2048, 63, True), ('ignored_unwritten', 'dur', 1023, 1, True)])
def test_ce_bound_rejects(defect, head, Rn, K, inside):
    x, t, ignore = R.ce_case(Rn, K, inside)
    v, S_v, g, S_g = R.ce_f64(x, t, ignore, 'zero')
    bv, bg = R.ce_f32(x, t, ignore, 'zero', defect=defect, cap=R.CE_CAP[head])
    assert not (R.within(bv, v, S_v, R.TAU['ce_value']) and R.within(bg, g, S_g, R.TAU['ce_grad']))
    gv, gg = R.ce_f32(x, t, ignore, 'zero', cap=R.CE_CAP[head])
    assert R.within(gv, v, S_v, R.TAU['ce_value']) and R.within(gg, g, S_g, R.TAU['ce_grad'])


def test_ce_defects_only_some_cases_see():
    # rows beyond 4 x the cap exist only beyond the cap; no max subtraction survives randn logits
    for head, Rn in (('dur', 1024), ('pitch', 2048), ('masked', 2048), ('masked', 2047)):
        x, t, ignore = R.ce_case(Rn, 7, False)
        v, S_v, g, S_g = R.ce_f64(x, t, ignore)
        bv, bg = R.ce_f32(x, t, ignore, defect='skip_rows', cap=R.CE_CAP[head])
        assert R.within(bv, v, S_v, R.TAU['ce_value']) and R.within(bg, g, S_g, R.TAU['ce_grad'])
    rng = np.random.RandomState(0)
    x, t = rng.randn(40, 65).astype(np.float32), rng.randint(0, 65, 40)
    v, S_v, g, S_g = R.ce_f64(x, t, -1)
    bv, bg = R.ce_f32(x, t, -1, defect='no_max')
    assert R.within(bv, v, S_v, R.TAU['ce_value']) and R.within(bg, g, S_g, R.TAU['ce_grad'])


def test_dispatch_arithmetic_matches_the_c_side():
    from ttscube_amd import _lib
    L = _lib.lib()
    for Rd in (0, 1, 4, 5, 1020, 1021, 1023, 1024, 1025, 1028, 1029, 5000):
        for Rp in (0, 1, 2044, 2045, 2047, 2048, 2049, 2052, 2053, 9000):
            for n in (4, 4096, 4100, R.L1_CAP_N - 4096, R.L1_CAP_N - 4, R.L1_CAP_N, R.L1_CAP_N + 4, 4 * R.L1_CAP_N):
                assert int(L.ttsc_textcoder_loss_workspace_bytes(Rd, Rp, n)) == R.tc_loss_workspace_bytes(Rd, Rp, n), (Rd, Rp, n)
    for Rn in (1, 4, 5, 2044, 2045, 2047, 2048, 2049, 2052, 2053, 100000):
        assert int(L.ttsc_masked_ce_workspace_bytes(Rn)) == R.masked_ce_workspace_bytes(Rn), Rn
    # the cases sit where they are meant to: the last uncapped grid, the cap reached, the cap crossed (a workgroup's second trip)
    assert [R.tc_loss_grid(r, 0, 4)[0] for r in R.CE_ROWS['dur']] == [1, 256, 256, 256]
    assert [4 * R.tc_loss_grid(r, 0, 4)[0] >= r for r in R.CE_ROWS['dur']] == [True, True, True, False]
    assert [R.tc_loss_grid(0, r, 4)[1] for r in R.CE_ROWS['pitch']] == [1, 512, 512, 512]
    assert [R.ce_blocks(r) for r in R.CE_ROWS['masked']] == [1, 512, 512, 512] and 4 * R.ce_blocks(2049) < 2049
    assert [R.tc_loss_grid(0, 0, n)[2] for n in R.L1_NS] == [1, 512, 512, 512]
    assert [n // 4 > 4 * 512 * R.TC_THREADS for n in R.L1_NS] == [False, False, False, True]


# ---- mel L1 ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', R.L1_NS)
def test_l1_bound_accepts_float32_and_rejects_its_defects(n):
    pre, post, t = R.l1_case(n)
    for a in (pre, post):
        v, S_v, g, S_g = R.l1_f64(a, t)
        gv, gg = R.l1_f32(a, t)
        assert _ok('l1_value', gv, v, S_v) and R.worst_ratio(gv, v, S_v) <= R.TAU['l1_value'] / 4
        assert _ok('l1_grad', gg, g, S_g)
        assert (g == 0).sum() == sum(1 for i in R.L1_TIES if i + 1 < n) and np.array_equal(gg == 0, g == 0)
        bv, bg = R.l1_f32(a, t, defect='n_float4')
        assert not R.within(bg, g, S_g, R.TAU['l1_grad'])
        bv, _ = R.l1_f32(a, t, defect='skip_tail')
        assert R.within(bv, v, S_v, R.TAU['l1_value']) == (n != R.L1_CAP_N + 4)      # only beyond the cap is there such a tail
        if n > 8:                                                                      # the tail moves the sum by far more than the bound
            assert 4 * R.L1_TAIL / n > 16 * R.TAU['l1_value'] * S_v


# ---- tag head --------------------------------------------------------------------------------------------------------------------------------------

def _tag(name, defect=None):
    c = R.tag_case(name)
    ref = R.tag_f64(c['x'], c['W'], c['b'], c['lens'], c['period'])
    got = R.tag_f32(c['x'], c['W'], c['b'], c['lens'], c['period'], defect=defect)
    return c, ref, got


def _tag_holds(ref, got):
    lg, S, tags, amb = ref
    fin = np.isfinite(lg)
    if not np.array_equal(np.isnan(got[0]), ~fin):
        return False
    if not R.within(np.where(fin, got[0], 0.0), np.where(fin, lg, 0.0), np.where(fin, S, 0.0), R.TAU['tag_logits']):
        return False
    return bool((got[1][~amb] == tags[~amb]).all())


@pytest.mark.parametrize('name', R.TAG_CASES)
def test_tag_bound_accepts_float32_and_few_rows_are_ambiguous(name):
    c, ref, got = _tag(name)
    lg, S, tags, amb = ref
    fin = np.isfinite(lg)
    r = _ratio('tag_logits', np.where(fin, got[0], 0.0), np.where(fin, lg, 0.0), np.where(fin, S, 0.0))
    assert _tag_holds(ref, got) and r <= R.TAU['tag_logits'] / 4, R.log2_ratio(r)
    assert amb.mean() <= R.TAG_AMBIGUOUS_CAP, amb.mean()                       # (these seeds: none at all but a 1-in-40 row at most)
    M, P, K = c['x'].shape[0], c['W'].shape[0], c['x'].shape[1]
    assert K % 4 == 0 and K + P <= R.TAG_MAX_FLOATS
    if name == 'ties':
        assert (tags == R.TAG_TIE_CLASSES[0]).all() and not amb.any()
        assert all((lg[:, p] == lg[:, R.TAG_TIE_CLASSES[0]]).all() for p in R.TAG_TIE_CLASSES)
    if name == 'nan':
        assert tags[2] == 0 and np.isnan(lg[2]).all() and fin[[0, 1, 3, 4]].all()
    if name == 'ragged':
        ok = R.tag_valid(M, c['lens'], c['period'])
        assert ok.sum() == 13 and not ok[8:16].any() and not tags[~ok].any() and not lg[~ok].any() and tags[ok].any()


def test_tag_limit_case_sits_on_the_lds_limit():
    M, P, K = R.TAG_SHAPES[-1]
    assert K + P == R.TAG_MAX_FLOATS


@pytest.mark.parametrize('defect,name', [('bias_pass0', '4x129x12'), ('bias_pass0', '9x300x400'), ('last_max', 'ties'), ('pad_tag', 'ragged')])
def test_tag_bound_rejects(defect, name):
    _, ref, got = _tag(name, defect)
    assert not _tag_holds(ref, got)
    assert _tag_holds(ref, _tag(name)[2])


def test_tag_bias_defect_needs_a_second_pass():
    _, ref, got = _tag('5x7x8', 'bias_pass0')
    assert _tag_holds(ref, got)


# ---- dropout_scale ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', R.DROPOUT_NS)
def test_dropout_bound_accepts_float32_and_rejects_a_missing_scale(n):
    x, keep, dy = R.dropout_case(n)
    for v in (x, dy):
        for p, k in ((R.DROPOUT_P, keep), (0.0, np.ones(n, np.float32))):
            ref, S = R.dropout_f64(v, k, p)
            got = R.dropout_f32(v, k, p)
            assert _ok('dropout', got, ref, S) and R.worst_ratio(got, ref, S) <= R.TAU['dropout'] / 4
            assert np.array_equal(got == 0, (k == 0) | (v == 0))
            if p and k.any():
                assert not R.within(v * k, ref, S, R.TAU['dropout'])
    ref, S = R.dropout_f64(x, keep, 0.0)
    assert np.array_equal(ref, x.astype(np.float64) * keep)                   # p = 0: the kept values themselves


def test_zz_tau_is_four_times_the_measured_yardstick():
    """runs last: every tau is the power of two at or above 4 x the worst err / S the float32 models reached above (and no more than 2 x
    that), so the table of tests/text_train_reference.py stays what the cases measure.  (An operation whose tests did not run in this
    session — a selection with -k — has nothing to compare.)"""
    for op in sorted(WORST):
        print('YARDSTICK %-12s worst 2^%.1f  tau 2^%d  (%d results)' % (op, R.log2_ratio(WORST[op]), int(np.log2(R.TAU[op])), NOTED[op]))
    assert set(NOTED_WHEN_COMPLETE) == set(R.TAU)
    for op, tau in R.TAU.items():
        if NOTED.get(op, 0) != NOTED_WHEN_COMPLETE[op]:
            continue
        if op == 'l1_grad':
            assert 4 * WORST[op] <= tau == 2.0 ** -24, op            # +-1 / n is one rounding: tau is the unit roundoff
            continue
        assert 4 * WORST[op] <= tau < 8 * WORST[op], (op, R.log2_ratio(WORST[op]))
