"""The numpy restatement of the two controlled kernels of csrc/prosody.hip: the integer duration rule as a plain loop and the
pitch transform in float32 with the kernel's documented float64 summation order.  Shared by tests/test_prosody_cpu.py (properties of the rule)
and tests/test_prosody_gpu.py (kernel == restatement, exactly)."""
import numpy as np


def q16(scale):
    """float duration multipliers -> int32 Q16, round to nearest"""
    return np.rint(np.asarray(scale, dtype=np.float64) * 65536.0).astype(np.int32)


def durations_row(d, scale_q16=None, dur_set=None, dcap=None):
    """d: the argmax durations of ONE row's valid phones -> (controlled durations int64 [n], emitted, number of times the floor at 1 engaged,
    number of times dcap engaged).  All in Python integers (no overflow, no rounding mode to think about)."""
    n = len(d)
    scale_q16 = [65536] * n if scale_q16 is None else [int(v) for v in scale_q16]
    dur_set = [-1] * n if dur_set is None else [int(v) for v in dur_set]
    dcap = (1 << 62) if dcap is None else int(dcap)
    acc = emitted = floors = caps = 0
    out = []
    for p in range(n):
        if dur_set[p] >= 0:
            nd = min(dur_set[p], dcap)
            emitted += nd
            acc = emitted << 16
        elif int(d[p]) == 0:
            nd = 0
        else:
            acc += int(d[p]) * scale_q16[p]
            nd = ((acc + 32768) >> 16) - emitted
            if nd < 1:
                nd, floors = 1, floors + 1
            if nd > dcap:
                nd, caps = dcap, caps + 1
            emitted += nd
        out.append(nd)
    return np.asarray(out, dtype=np.int64), emitted, floors, caps


def align_durations(logits, lengths=None, scale_q16=None, dur_set=None, dcap=None, fcap=None):
    """logits [B, N, D] -> (durs int32 [B, N], list of per-row frame->phone lists cut at fcap, flen int32 [B]) as ttsc_align_durations_ctl writes them"""
    B, N, D = logits.shape
    d_all = np.argmax(logits, axis=2)          # (first maximum, like the kernel's strict comparison)
    durs = np.zeros((B, N), np.int32)
    f2p, flen = [], np.zeros((B,), np.int32)
    for b in range(B):
        n = N if lengths is None else min(int(lengths[b]), N)
        nd, emitted, _, _ = durations_row(d_all[b, :n], None if scale_q16 is None else scale_q16[b, :n], None if dur_set is None else dur_set[b, :n], dcap)
        durs[b, :n] = nd
        row = np.repeat(np.arange(n), nd)
        if fcap is not None:
            row = row[:fcap]
        f2p.append(row.astype(np.int32))
        flen[b] = len(row)
    return durs, f2p, flen


def voiced_mean(p0, voiced):
    """the kernel's mean of the voiced p0 (float32 [n], the row's own frames): lane t of 64 adds frames t, t + 64, ... in float64 in that order, the 64
    partial sums are folded pairwise (part[t] += part[t + off], off = 32 .. 1); float32(sum / count).  None when no frame is voiced."""
    part = np.zeros(64, np.float64)
    cnt = int(np.count_nonzero(voiced))
    for f in range(len(p0)):
        if voiced[f]:
            part[f % 64] += np.float64(p0[f])
    off = 32
    while off > 0:
        part[:off] = part[:off] + part[off:2 * off]
        off >>= 1
    return np.float32(part[0] / np.float64(cnt)) if cnt else None


def pitch_from_p0(p0, voiced, flen, max_pitch, mul_per_frame, rng, mean=None):
    """the transform itself on the uncontrolled pitch p0 float32 [F] (0 on unvoiced frames) and the voiced flags [F]: steps 1 and 2 of
    ttsc_cond_input_ctl on the voiced frames, every operation rounded on its own in float32.  mean: override of the voiced mean."""
    f32 = np.float32
    p0 = np.asarray(p0, f32)
    p = p0.copy()
    rng = f32(rng)
    if rng != f32(1.0):
        m = voiced_mean(p0[:flen], voiced[:flen]) if mean is None else f32(mean)
        if m is not None:
            p = (m + (rng * (p0 - m).astype(f32)).astype(f32)).astype(f32)
    p = (p * np.asarray(mul_per_frame, f32)).astype(f32)
    p = np.minimum(np.maximum(p, f32(0.0)), f32(max_pitch)).astype(f32)
    return np.where(voiced, p, p0).astype(f32)


def pitch_row(op, flen, max_pitch, mul_per_frame, rng, mean=None):
    """op float32 [F, 2] (pitch head: value, voicing), flen = the row's own frame count, mul_per_frame float32 [F] (the multiplier of each frame's
    phone), rng = the row's range -> pitch float32 [F]"""
    f32 = np.float32
    op = np.asarray(op, f32)
    vuv = np.rint(op[:, 1]).astype(f32)                          # half to even, like rintf / torch.round
    p0 = (op[:, 0] * f32(max_pitch)).astype(f32) * vuv
    return pitch_from_p0(p0, vuv == f32(1.0), flen, max_pitch, mul_per_frame, rng, mean)


def frame_rows(f2p_row, flen, F):
    """the phone of each of F frames: the row's own map, then its last aligned phone (phone 0 for a row without frames): cond_input's padding rule"""
    rows = np.zeros(F, np.int64)
    n = min(int(flen), F)
    rows[:n] = f2p_row[:n]
    if flen > 0:
        rows[n:] = f2p_row[flen - 1]
    return rows


def cond_input(g, f2p, flen, op, max_pitch, pitch_mul, pitch_range, Cp):
    """g float32 [B, N, C], f2p: per-row frame->phone arrays, flen [B], op float32 [B, F, 2], pitch_mul float32 [B, N], pitch_range float32 [B]
    -> (pitch float32 [B, F], gin float32 [B, F, Cp]) as ttsc_cond_input_ctl writes them"""
    f32 = np.float32
    B, N, C = g.shape
    F = op.shape[1]
    pitch = np.zeros((B, F), f32)
    gin = np.zeros((B, F, Cp), f32)
    inv = f32(1.0) / f32(max_pitch)
    for b in range(B):
        rows = frame_rows(f2p[b], int(flen[b]), F)
        pitch[b] = pitch_row(op[b], int(flen[b]), max_pitch, pitch_mul[b][rows], pitch_range[b])
        gin[b, :, :C] = g[b][rows]
        gin[b, :, C] = (pitch[b] * inv).astype(f32)
    return pitch, gin
