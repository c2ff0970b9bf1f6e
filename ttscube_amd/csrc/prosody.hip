// Prosody control inside the two launches a sentence already pays for: the duration head -> frame map with a per-phone tempo
// and pinned frame counts (align.hip::align_durations_kernel's controlled form), and the input of Languasito2's conditioning recurrence with a
// per-phone pitch multiplier and a per-row pitch range (align.hip::cond_input_kernel's controlled form).  The uncontrolled kernels stay what
// they are: a call without controls never comes here.  Both controlled kernels reproduce their uncontrolled twin bit for bit under the
// identity controls (scale 65536, no pinned count; multiplier 1, range 1).
#include "common.hpp"

namespace ttsc {

// One workgroup per utterance, as align_durations_kernel.  Per pass of 256 phones: every thread takes the first-maximum argmax of its phone
// and stages it with the phone's controls in LDS; lane 0 then walks the pass in phone order with the row's carry in registers — the rule is
// a recurrence over (acc, emitted) whose clamps (floor at 1, dcap, a pinned count resynchronising the carry) do not compose into a scan, and
// a row has a few hundred phones at most: 256 steps of integer work out of LDS —; then every thread scatters its phone's indices.
//   acc = 0 (int64, Q16); emitted = 0
//   set[p] >= 0: nd = min(set[p], dcap); emitted += nd; acc = emitted << 16
//   d == 0:      nd = 0
//   else:        acc += d * scale[p]; nd = ((acc + 32768) >> 16) - emitted; nd = min(max(nd, 1), dcap); emitted += nd
// scale == NULL reads as 65536 everywhere, set == NULL as -1 everywhere.
__global__ __launch_bounds__(256) void align_durations_ctl_kernel(const float* __restrict__ logits, const int* __restrict__ len, int N, int D,
                                                                  const int* __restrict__ scale, const int* __restrict__ set, int dcap,
                                                                  int* __restrict__ durs, int* __restrict__ f2p, int* __restrict__ flen,
                                                                  int Fcap) {
    __shared__ int s_d[256], s_scale[256], s_set[256], s_nd[256], s_start[256];
    __shared__ long long s_acc, s_emitted;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = len ? (len[b] < N ? (len[b] > 0 ? len[b] : 0) : N) : N;
    if (tid == 0) {
        s_acc = 0;
        s_emitted = 0;
    }
    for (int p0 = 0; p0 < n; p0 += 256) {
        const int p = p0 + tid;
        int d = 0;
        if (p < n) {
            const float* row = logits + ((size_t)b * N + p) * D;
            float best = row[0];
            for (int k = 1; k < D; ++k) {
                const float v = row[k];
                if (v > best) {   // strict: the FIRST maximum, NaN never wins (as align_durations_kernel)
                    best = v;
                    d = k;
                }
            }
            s_scale[tid] = scale ? scale[(size_t)b * N + p] : 65536;
            s_set[tid] = set ? set[(size_t)b * N + p] : -1;
        }
        s_d[tid] = d;
        __syncthreads();
        if (tid == 0) {
            long long acc = s_acc, emitted = s_emitted;
            const int m = n - p0 < 256 ? n - p0 : 256;
            for (int i = 0; i < m; ++i) {
                long long nd;
                if (s_set[i] >= 0) {
                    nd = s_set[i] < dcap ? s_set[i] : dcap;
                    s_start[i] = (int)(emitted < Fcap ? emitted : Fcap);
                    emitted += nd;
                    acc = emitted << 16;
                } else if (s_d[i] == 0) {
                    nd = 0;
                    s_start[i] = 0;
                } else {
                    acc += (long long)s_d[i] * (long long)s_scale[i];
                    nd = ((acc + 32768) >> 16) - emitted;
                    nd = nd > 1 ? nd : 1;
                    nd = nd < dcap ? nd : dcap;
                    s_start[i] = (int)(emitted < Fcap ? emitted : Fcap);
                    emitted += nd;
                }
                s_nd[i] = (int)nd;
            }
            s_acc = acc;
            s_emitted = emitted;
        }
        __syncthreads();
        if (p < n) {
            const int nd = s_nd[tid], start = s_start[tid];
            durs[(size_t)b * N + p] = nd;
            for (int k = 0; k < nd && start + k < Fcap; ++k) f2p[(size_t)b * Fcap + start + k] = p;   // (start <= Fcap, k < Fcap: no overflow)
        }
        __syncthreads();   // (the staging arrays are rewritten by the next pass)
    }
    for (int p = n + tid; p < N; p += 256) durs[(size_t)b * N + p] = 0;
    __syncthreads();
    if (tid == 0) flen[b] = (int)(s_emitted < Fcap ? s_emitted : Fcap);
}

// cond_input_kernel with the pitch controls.  One workgroup per (frame, row), 64 or 256 threads.  With p0 = (o0 * max_pitch) * vuv as there, a
// voiced frame (vuv == 1) becomes
//   1. rng[b] != 1 and the row has a voiced frame f < flen[b]:  p = m + rng[b] * (p0 - m)
//   2. p = p * mul[b, row(f)];  p = min(max(p, 0), max_pitch)
// every operation rounded on its own in float32.  m = the mean of p0 over the row's voiced frames f < flen[b].  It is formed in THIS launch, by
// every workgroup that needs it, in one fixed order that depends on neither the block size nor the batch: thread t < 64 adds the voiced p0 of
// frames t, t + 64, t + 128, ... in float64 in that order; the 64 partial sums (and counts) are folded pairwise — part[t] += part[t + off] for
// off = 32, 16, 8, 4, 2, 1 —; m = float32(part[0] / count).  A row costs its workgroups flen[b] reads of 8 bytes each out of L2, which is
// cheaper than a launch of its own on the critical path of a sentence, and a row's result cannot depend on its neighbours.
__global__ __launch_bounds__(256) void cond_input_ctl_kernel(const float* __restrict__ x, const int* __restrict__ f2p, const int* __restrict__ flen,
                                                             const float* __restrict__ op, float max_pitch, const float* __restrict__ mul,
                                                             const float* __restrict__ rng, int N, int C, int Cp, int Fcap, int F,
                                                             float* __restrict__ pitch, float* __restrict__ out) {
    __shared__ double s_sum[64];
    __shared__ int s_cnt[64];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nf = flen[b];
    const int row = f < nf ? f2p[(size_t)b * Fcap + f] : (nf == 0 ? 0 : f2p[(size_t)b * Fcap + (nf - 1)]);
    const float* src = x + ((size_t)b * N + row) * C;
    float* dst = out + ((size_t)b * F + f) * Cp;
    if ((C & 3) == 0) {
        for (int i = tid; i < (C >> 2); i += blockDim.x) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int i = tid; i < C; i += blockDim.x) dst[i] = src[i];
    }
    const float* o = op + ((size_t)b * F + f) * 2;
    const float vuv = rintf(o[1]);                        // torch.round: half to even
    const float r = rng[b];
    const bool need_mean = vuv == 1.0f && r != 1.0f;      // (the same for every thread of the workgroup)
    if (need_mean) {
        if (tid < 64) {
            double s = 0.0;
            int c = 0;
            const int m = nf < F ? nf : F;
            for (int g = tid; g < m; g += 64) {
                const float* og = op + ((size_t)b * F + g) * 2;
                const float vg = rintf(og[1]);
                if (vg == 1.0f) {
                    s += (double)__fmul_rn(__fmul_rn(og[0], max_pitch), vg);
                    ++c;
                }
            }
            s_sum[tid] = s;
            s_cnt[tid] = c;
        }
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {
            if (tid < off) {
                s_sum[tid] += s_sum[tid + off];
                s_cnt[tid] += s_cnt[tid + off];
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        float p = __fmul_rn(__fmul_rn(o[0], max_pitch), vuv);
        if (vuv == 1.0f) {
            if (need_mean && s_cnt[0] > 0) {
                const float m = (float)(s_sum[0] / (double)s_cnt[0]);
                p = __fadd_rn(m, __fmul_rn(r, __fsub_rn(p, m)));
            }
            p = __fmul_rn(p, mul[(size_t)b * N + row]);
            p = fminf(fmaxf(p, 0.f), max_pitch);
        }
        pitch[(size_t)b * F + f] = p;
        const float inv = 1.0f / max_pitch;
        dst[C] = __fmul_rn(p, inv);
        for (int i = C + 1; i < Cp; ++i) dst[i] = 0.f;
    }
}

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_align_durations_ctl(const float* logits_dev, const int32_t* len_dev, int32_t B, int32_t N, int32_t D, int32_t* durs_dev,
                                        int32_t* f2p_dev, int32_t* flen_dev, int32_t Fcap, const int32_t* dur_scale_q16_dev,
                                        const int32_t* dur_set_dev, int32_t dcap, void* stream) {
    TTSC_REQUIRE(logits_dev && durs_dev && f2p_dev && flen_dev, "ttsc_align_durations_ctl: null argument");
    TTSC_REQUIRE(B > 0 && N > 0 && D > 0 && Fcap > 0 && dcap >= 0, "ttsc_align_durations_ctl: bad sizes (B=%d N=%d D=%d Fcap=%d dcap=%d)", B, N, D, Fcap,
                 dcap);
    hipLaunchKernelGGL(align_durations_ctl_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits_dev, len_dev, N, D, dur_scale_q16_dev,
                       dur_set_dev, dcap, durs_dev, f2p_dev, flen_dev, Fcap);
    return launch_checked("align_durations_ctl_kernel");
}

extern "C" int ttsc_cond_input_ctl(const float* g_dev, const int32_t* f2p_dev, const int32_t* flen_dev, const float* pitch_out_dev, float max_pitch,
                                   int32_t B, int32_t N, int32_t C, int32_t Cp, int32_t Fcap, int32_t F, float* pitch_dev, float* out_dev,
                                   const float* pitch_mul_dev, const float* pitch_range_dev, void* stream) {
    TTSC_REQUIRE(g_dev && f2p_dev && flen_dev && pitch_out_dev && pitch_dev && out_dev && pitch_mul_dev && pitch_range_dev,
                 "ttsc_cond_input_ctl: null argument");
    TTSC_REQUIRE(B > 0 && N > 0 && C > 0 && Cp > C && Fcap > 0 && F > 0 && max_pitch > 0.f, "ttsc_cond_input_ctl: bad sizes (B=%d N=%d C=%d Cp=%d F=%d)", B, N, C,
                 Cp, F);
    hipLaunchKernelGGL(cond_input_ctl_kernel, dim3((unsigned)F, (unsigned)B), dim3(C >= 1024 ? 256 : 64), 0, (hipStream_t)stream, g_dev, f2p_dev,
                       flen_dev, pitch_out_dev, max_pitch, pitch_mul_dev, pitch_range_dev, N, C, Cp, Fcap, F, pitch_dev, out_dev);
    return launch_checked("cond_input_ctl_kernel");
}
