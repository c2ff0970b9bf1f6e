"""Input sets of the shared-math tests (tests/test_shared_math_cpu.py: host build against float64; tests/test_shared_math_gpu.py: device
against host, bit for bit).  Everything is a pure function of constants: both tests see the same values."""
import numpy as np

STRIDE = 1021                      # a prime: the stratified set visits every exponent with both signs, subnormals, infinities and NaNs
RADIUS = 64                        # bit patterns on either side of a boundary point

F32 = np.float32
FLT_MIN = F32(1.17549435e-38)
SQRT2_F = F32(1.41421356237)       # the fold constant of ttsc_logf, as the compiler reads it
PLOW_F = F32(0.02425)              # ttsc_normal_icdf's tail boundary
U01_MIN = F32(2.0 ** -24)          # ttsc_u01(0)
U01_MAX = F32(1.0 - 2.0 ** -24)    # ttsc_u01(0xffffffff)
CLIP_LO = F32(1e-5)
SIGMOID_SUBNORMAL_BELOW = F32(-87.34)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def floats(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint32)).view(np.float32)


def stratified_u32():
    """every STRIDE-th uint32: ceil(2^32 / 1021) = 4 206 629 values"""
    return np.arange(0, 1 << 32, STRIDE, dtype=np.uint64).astype(np.uint32)


def neighbours(x, radius=RADIUS):
    """the float32 bit patterns within `radius` steps of x on either side, in the order of the real line (both zeros count as one step)"""
    b = int(bits([x])[0])
    key = (b & 0x7fffffff) * (-1 if b >> 31 else 1)
    keys = np.arange(key - radius, key + radius + 1, dtype=np.int64)
    out = np.where(keys >= 0, keys, (-keys) | 0x80000000).astype(np.uint32)
    if (keys == 0).any():
        out = np.concatenate([out, np.array([0x80000000], dtype=np.uint32)])
    return out


def boundary_points():
    one = F32(1.0)
    pts = [F32(0.0), F32(-0.0), FLT_MIN, -FLT_MIN, floats([0x007fffff])[0], F32(-87.0), F32(88.0), SIGMOID_SUBNORMAL_BELOW,
           F32(0.0625), F32(-0.0625)]
    pts += [F32(np.ldexp(np.float64(SQRT2_F), e)) for e in (-126, -64, -1, 0, 1, 64, 127)]
    pts += [one, PLOW_F, F32(one - PLOW_F), U01_MIN, U01_MAX, CLIP_LO, F32(one - CLIP_LO)]
    pts += [F32(np.inf), F32(-np.inf)]   # the stride steps over both infinities: here with FLT_MAX's side and the first NaNs behind them
    return pts


def boundary_f32():
    return floats(np.unique(np.concatenate([neighbours(p) for p in boundary_points()])))


def float_inputs():
    """stratified set + boundary set, as float32"""
    return floats(np.unique(np.concatenate([stratified_u32(), bits(boundary_f32())])))


def u32_inputs():
    """stratified set, both ends, and the patterns around r >> 9 in {0, 1, 2^22, 2^23 - 1}"""
    extra = [np.array([0, 0xffffffff], dtype=np.int64)]
    for q in (0, 1, 1 << 22, (1 << 23) - 1):
        for edge in (q << 9, (q << 9) + 511):            # first and last r of the bucket
            extra.append(np.arange(edge - RADIUS, edge + RADIUS + 1, dtype=np.int64))
    e = np.concatenate(extra)
    e = e[(e >= 0) & (e <= 0xffffffff)]
    return np.unique(np.concatenate([stratified_u32(), e.astype(np.uint32)]))


def u01_exact(r):
    """ttsc_u01 in exact arithmetic (every value is a float32): float64 [n]"""
    return ((np.asarray(r, dtype=np.uint32) >> 9).astype(np.float64) + 0.5) / 8388608.0


def same_bits_or_nan(got, want):
    """mask of elements where got is NOT acceptable: bits differ, except that a NaN answers a NaN whatever the payload"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
