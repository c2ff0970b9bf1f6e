"""CPU: the convolution dispatch (csrc/conv_plan.hpp through the query ttsc_conv1d_plan — the function the launcher itself calls) against its
Python restatement in tests/conv_reference.py, over every layer shape of the project around every threshold of the fill rule, and pinned as
literals for the headline workload.  All tiles of a layer give the same bits, so nothing but this file notices a drifted threshold.
The once-per-process switches (TTSC_F16_TILE, TTSC_CONV_ACC_INIT, TTSC_CONV_TALL, TTSC_CONV_WANT, TTSC_CONV_NARROW, TTSC_CONV_EPI_PREFETCH,
TTSC_TALL_SWIZZLE) are covered unset only."""
import ctypes as C

import pytest

from tests import conv_reference as R

BATCHES = (1, 2, 3, 64)
FIELDS = ('rows', 'cols', 'tap_bucket', 'grid', 'lds', 'lean', 'acc_init', 'short_from')


def _conv(cin, cout, k, d=1):
    return dict(cin=cin, cout=cout, k=k, dilation=d, padding=d * (k - 1) // 2)


def _trans(cin, cout, k, s):
    return dict(cin=cin, cout=cout, k=k, stride=s, padding=(k - s) // 2, transposed=True)


CONV_PRE, CONV_POST = _conv(80, 512, 7), _conv(32, 1, 7)
UPS = [_trans(512, 256, 16, 5), _trans(256, 128, 16, 3), _trans(128, 64, 4, 4), _trans(64, 32, 4, 4)]
RESBLOCK = [_conv(c, c, k, d) for c in (256, 128, 64, 32) for k in (3, 7, 11) for d in (1, 3, 5)]
GROUPED = dict(_conv(256, 256, 41), groups=16)   # a discriminator layer: fp32 whatever is asked for
LAYERS = ([CONV_PRE] + UPS + RESBLOCK + [CONV_POST] + [_conv(*l) for l in R.GENERAL_CONV] + [_trans(*l) for l in R.GENERAL_TRANS] + [GROUPED])


class _Handles:
    """weightless handles (ttsc_conv1d_create + ttsc_conv1d_set_precision: no device is touched), one per (layer, precision)"""

    def __init__(self):
        from ttscube_amd import _lib
        self._lib, self.L, self.h = _lib, _lib.lib(), {}

    def get(self, layer, prec):
        key = (tuple(sorted(layer.items())), prec)
        if key not in self.h:
            cfg = self._lib.Conv1dCfg(layer['cin'], layer['cout'], layer['k'], layer.get('stride', 1), layer['padding'], layer.get('dilation', 1),
                                      int(layer.get('transposed', False)), layer.get('groups', 1))
            h = C.c_void_p()
            self._lib.check(self.L.ttsc_conv1d_create(C.byref(cfg), C.byref(h)), 'create')
            self._lib.check(self.L.ttsc_conv1d_set_precision(h, self._lib.PREC_F16X3 if prec == 'f16x3' else self._lib.PREC_FP32), 'set_precision')
            self.h[key] = h
        return self.h[key]

    def plan(self, layer, prec, B, Lin, phase=0, gate=False, act=None, out_scale=1.0, in_scale=1.0):
        """the query's answer as the restatement's dict, None where it refuses"""
        ep = self._lib.Conv1dEpilogue(in_scale, 1.0, out_scale, self._lib.ACT_TANH if act == 'tanh' else self._lib.ACT_NONE, 0, 16 if gate else None, 1.0)
        info = (C.c_int32 * 10)()
        fam = self.L.ttsc_conv1d_plan(self.get(layer, prec), B, Lin, C.byref(ep), phase, info)
        if fam < 0:
            return None
        v = list(info)
        return dict(family=fam, rows=v[0], cols=v[1], tap_bucket=v[2], grid=tuple(v[3:6]), lds=v[6], lean=v[7], acc_init=v[8], short_from=v[9])

    def close(self):
        for h in self.h.values():
            self.L.ttsc_conv1d_destroy(h)


@pytest.fixture(scope='module')
def handles():
    hs = _Handles()
    yield hs
    hs.close()


def _restated(layer, prec, B, Lin, **kw):
    try:
        return R.plan(B=B, Lin=Lin, prec=prec, **layer, **kw)
    except R.PlanError:
        return None


def _phases(layer):
    vfused = layer.get('transposed', False) and layer['cout'] % 32 == 0
    return range(layer['stride']) if layer.get('transposed', False) and not vfused else (0,)


def _agree(handles, layer, prec, B, Lin, env, **kw):
    if R.out_len(Lin, layer['k'], layer.get('stride', 1), layer['padding'], layer.get('dilation', 1), layer.get('transposed', False)) <= 0:
        return None
    got = [handles.plan(layer, prec, B, Lin, phase=ph, **kw) for ph in _phases(layer)]
    want = [_restated(layer, prec, B, Lin, phase=ph, **env, **kw) for ph in _phases(layer)]
    assert got == want, (layer, prec, B, Lin, env, kw, got, want)
    return want[0]


def _threshold_lengths(layer, B):
    """lengths at which a workgroup count the rule compares with 512 is just below it, the first at or above it, and the next one: for every
    tile the fill rule tests (the first two of the class), the tall tiles and the wide tile, whole tiles - 1, exact and + 1 column"""
    vfused = layer.get('transposed', False) and layer['cout'] % 32 == 0
    rows_v = layer['cout'] * (layer['stride'] if vfused else 1)
    out = set()
    for prec in ('f16x3', 'fp32'):
        mt = R.mt_class(layer['cout'], layer.get('stride', 1), layer.get('transposed', False))
        for rows, cols in R.tiles_of(prec, mt)[:2] + [(256, 128), (128, 256)]:
            m = max(1, -(-rows_v // rows)) * B
            n0 = -(-512 // m)
            for n in (n0 - 1, n0, n0 + 1):
                out.update(L for L in (n * cols - 1, n * cols, n * cols + 1) if L > 0)
    return sorted(out)


def _setenv(monkeypatch, wide=None, lean=None, tile=None):
    for name, v in (('TTSC_CONV_WIDE', wide), ('TTSC_CONV_LEAN', lean), ('TTSC_CONV_TILE', tile)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return dict(wide=1 if wide is None else wide, lean=lean is None, tile=tile)


def test_headline_workload_reaches_these_kernels(handles, monkeypatch):
    """bench.py's batch (B = 64, 800 frames, f16x3; every stage hands on (L - 1) * stride + k - 2 * padding positions: 4001, 12004, 48016):
    kernel, template arguments, grid (in workgroups) and dynamic LDS bytes as the kernel trace (rocprofv3 --kernel-trace over bench.py --steps 1
    --warmup 0) of the build BEFORE the planner existed lists them.  At this batch conv_post runs inside the last chain kernel; the trace holds
    it as a launch of its own for the generator's one-utterance calibration pass (96 frames -> 23104 samples), with conv_pre beside it."""
    env = _setenv(monkeypatch)
    want = [(CONV_PRE, 64, 800, R.PATH_F16X3, 64, 256, 7, (4, 8, 64), 45440),          # conv_f16x3_kernel<2, 2, 7, false>
            (UPS[0], 64, 800, R.PATH_TALL, 256, 128, 0, (2240, 1, 1), 49600),          # conv_f16x3_tall_kernel<512, 4, 4, 2, true>, XCD-aware 1-D grid
            (UPS[1], 64, 4001, R.PATH_TALL, 128, 256, 0, (3072, 1, 1), 49856),         # conv_f16x3_tall_kernel<256, 6, 2, 4, true>
            (UPS[2], 64, 12004, R.PATH_F16X3, 64, 256, 3, (47, 4, 64), 20480),         # conv_f16x3_kernel<2, 2, 3, false>
            (UPS[3], 64, 48016, R.PATH_F16X3, 64, 256, 3, (188, 2, 64), 20480),        # conv_f16x3_kernel<2, 2, 3, false>
            (_conv(256, 256, 3, 1), 64, 4001, R.PATH_WIDE, 128, 256, 0, (16, 2, 64), 49472),      # conv_f16x3_wide_kernel<256, 3, 1, true>
            (_conv(128, 128, 11, 5), 64, 12004, R.PATH_WIDE, 128, 256, 0, (47, 1, 64), 55616),    # conv_f16x3_wide_kernel<128, 11, 5, true>
            (CONV_POST, 1, 23104, R.PATH_COUT1, 1, 1024, 0, (23, 1, 1), 0),            # conv_cout1_kernel
            (CONV_PRE, 1, 96, R.PATH_F16X3, 32, 128, 7, (1, 16, 1), 22912)]            # conv_f16x3_kernel<1, 1, 7, false>
    for layer, B, Lin, fam, rows, cols, bucket, grid, lds in want:
        p = _agree(handles, layer, 'f16x3', B, Lin, env)
        assert (p['family'], p['rows'], p['cols'], p['tap_bucket'], p['grid'], p['lds']) == (fam, rows, cols, bucket, grid, lds), (layer, p)
        assert p['lean'] == (fam in (R.PATH_TALL, R.PATH_WIDE, R.PATH_F16X3))   # (the trace's wide and tall instantiations end in `true`)


@pytest.mark.parametrize('wide', [None, 0, 2])
@pytest.mark.parametrize('lean', [None, 0])
def test_plan_matches_the_restatement_around_every_threshold(handles, monkeypatch, wide, lean):
    env = _setenv(monkeypatch, wide, lean)
    seen = set()
    for layer in LAYERS:
        for B in BATCHES:
            for Lin in _threshold_lengths(layer, B) + [1, 7, 800]:
                for prec in ('f16x3', 'fp32'):
                    p = _agree(handles, layer, prec, B, Lin, env)
                    if p:
                        seen.add((p['family'], p['rows'], p['cols']))
    # every family and every tile of every class was planned by the default rule somewhere
    fams = {s[0] for s in seen}
    assert fams >= {R.PATH_COUT1, R.PATH_F16X3, R.PATH_FP32} and ((R.PATH_WIDE in fams and R.PATH_TALL in fams) or wide == 0)
    for prec, fam in (('f16x3', R.PATH_F16X3), ('fp32', R.PATH_FP32)):
        for mt in (32, 64, 128):
            for t in R.tiles_of(prec, mt):
                assert (fam,) + t in seen, (prec, mt, t)


def test_narrower_pays_flips(handles, monkeypatch):
    """fp32 fill rule: a tile that fills the machine is passed over when the next narrower column count cuts the padded columns by more than an
    eighth; every length up to a few tiles, at batch sizes at which every tile fills the machine"""
    env = _setenv(monkeypatch)
    for layer in (_conv(512, 512, 3), _conv(64, 64, 7, 3), _conv(32, 32, 11, 5), _conv(512, 100, 5), GROUPED):
        picked = set()
        for B in (64, 600):
            for Lin in range(1, 1100):
                p = _agree(handles, layer, 'fp32', B, Lin, env)
                picked.add((B, p['rows'], p['cols']))
        mt = 32 if layer is GROUPED else R.mt_class(layer['cout'])
        tiles = R.tiles_of('fp32', mt)
        assert {t[1:] for t in picked} == set(tiles), (layer, picked)
        # at B = 600 every tile fills the machine: only the padding test is left, and it sends lengths to the last tile
        assert (600,) + tiles[0] in picked and (600,) + tiles[2] in picked, (layer, picked)


def test_forced_tiles_and_refusals(handles, monkeypatch):
    for layer in [CONV_PRE, CONV_POST, UPS[0], UPS[2], _conv(256, 256, 7, 3), _conv(32, 32, 3)] + [_conv(*l) for l in R.GENERAL_CONV] + \
                 [_trans(*l) for l in R.GENERAL_TRANS] + [GROUPED]:
        for prec in ('f16x3', 'fp32'):
            mt = 32 if layer is GROUPED else R.mt_class(layer['cout'], layer.get('stride', 1), layer.get('transposed', False))
            legal = R.tiles_of('fp32' if layer is GROUPED else prec, mt)
            for tile in ['%dx%d' % t for t in legal] + ['16x128', '64x', '128X128']:
                for wide in (None, 2):
                    env = _setenv(monkeypatch, wide=wide, tile=tile)
                    for B, Lin in ((1, 300), (64, 800)):
                        p = _agree(handles, layer, prec, B, Lin, env)
                        general = R.plan(B=B, Lin=Lin, prec=prec, **layer, wide=env['wide'])['family'] in (R.PATH_F16X3, R.PATH_FP32)
                        if tile == '64x' or (general and tile == '16x128'):
                            assert p is None, (layer, prec, tile, p)
                        elif general and tile != '128X128':
                            assert (p['rows'], p['cols']) == tuple(map(int, tile.split('x'))), (layer, prec, tile, p)
    # the refusal says what is wrong, in the launcher's words
    _setenv(monkeypatch, tile='16x128')
    assert handles.plan(CONV_PRE, 'f16x3', 1, 300) is None
    assert b'TTSC_CONV_TILE=16x128 is not a split-kernel tile of this layer (MT 128: 64x256, 64x128, 32x128)' in handles.L.ttsc_last_error()
    assert handles.plan(CONV_PRE, 'fp32', 1, 300) is None
    assert b'is not an fp32 tile of this layer (MT 128: 128x128, 64x128, 64x64)' in handles.L.ttsc_last_error()
    _setenv(monkeypatch, tile='big')
    assert handles.plan(CONV_POST, 'f16x3', 1, 300) is None and b"TTSC_CONV_TILE must be <rows>x<cols>, e.g. 64x256 (got 'big')" in handles.L.ttsc_last_error()


def test_epilogue_fields_that_steer_the_dispatch(handles, monkeypatch):
    env = _setenv(monkeypatch)
    for layer in (_conv(256, 256, 7, 3), _conv(128, 128, 3), UPS[0], UPS[1], UPS[2], CONV_POST, CONV_PRE):
        for prec in ('f16x3', 'fp32'):
            for B, Lin in ((1, 300), (64, 4000)):
                for kw in (dict(gate=True), dict(act='tanh'), dict(out_scale=0.5), dict(in_scale=0.0), dict(in_scale=-1.0), dict(in_scale=float('inf')),
                           dict(in_scale=1.0 / 3.0)):
                    _agree(handles, layer, prec, B, Lin, env, **kw)
    # what the fields do, on the layer where each matters
    big = dict(B=64, Lin=4000)
    assert handles.plan(_conv(256, 256, 7, 3), 'f16x3', **big)['acc_init'] == 1 and handles.plan(_conv(256, 256, 7, 3), 'f16x3', act='tanh', **big)['acc_init'] == 0
    assert handles.plan(_conv(256, 256, 7, 3), 'f16x3', gate=True, **big)['family'] == R.PATH_F16X3
    assert handles.plan(UPS[0], 'f16x3', gate=True, **big)['family'] == R.PATH_F16X3
    assert handles.plan(CONV_POST, 'f16x3', gate=True, **big)['family'] == R.PATH_F16X3 and handles.plan(CONV_POST, 'fp32', **big)['family'] == R.PATH_COUT1
    assert handles.plan(UPS[0], 'f16x3', in_scale=0.0, **big)['lean'] == 0 and handles.plan(UPS[0], 'f16x3', **big)['lean'] == 1
    assert handles.plan(GROUPED, 'f16x3', **big)['family'] == R.PATH_FP32
