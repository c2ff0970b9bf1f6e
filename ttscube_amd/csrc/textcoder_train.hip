// Training-only kernels of CubenetTextcoder (cube/networks/textcoder.py:191-226, modules.py:117-145) — gfx950.
//
// The PostNet is 4 x [ConvNorm k5 -> BatchNorm1d(512) -> Tanh -> Dropout(0.1)] + ConvNorm k5.  Inference folds the BatchNorm into the
// convolution (modules.py _ConvStack); training needs the batch statistics, so the block after each convolution is one launch here:
//   ttsc_bn_tanh_dropout_train_forward    y = keep * tanh(gamma * (x - mean) * invstd + beta) / (1 - p),  mean / biased var over the B x F
//                                         values of a channel; running_mean / running_var (UNBIASED variance) updated in the same launch
//   ttsc_bn_tanh_dropout_train_backward   dx, dgamma, dbeta
// One workgroup per channel: every reduction is a fixed-order per-thread walk plus a fixed shuffle / LDS tree (double accumulators), so two
// calls give the same bits.  No float atomics anywhere.  The dropout mask is injected ({0,1} floats, parity tests) or drawn from Philox-4x32-10
// (the counter scheme of melar.hip: counter (i >> 2, i >> 34, layer, tag), key = seed; word i & 3) — the backward pass draws the same words.
//
//   ttsc_textcoder_loss   the four loss terms of the step in ONE launch, values and gradients:
//       CE(dur logits, dur targets, ignore_index) and CE(pitch logits, pitch targets, ignore_index): mean over the non-ignored rows
//       mean |pre - t| and mean |post - t| over all values
//   A target outside [0, classes) that is not ignore_index sets a bit of a status word (1 duration, 2 pitch) and contributes nothing: the
//   host raises; there is no device assert.  Partial sums per workgroup are added in a fixed order by the last workgroup (ticket).
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "ce_loss.hpp"
#include "../../include/ttscube_math.h"

namespace ttsc {

namespace {

constexpr uint32_t TC_BN_TAG = 0x424E3131u;   // Philox counter word 3 of the PostNet dropout

struct BnArgs {
    const float* x;        // [B, C, F]
    const float* gamma;    // [C]
    const float* beta;     // [C]
    float* rmean;          // [C] (forward only)
    float* rvar;           // [C] (forward only)
    float* y;              // [B, C, F] forward output
    float* mean;           // [C] saved
    float* invstd;         // [C] saved
    const float* mask;     // [B, C, F] {0,1} or null (Philox)
    const float* dy;       // [B, C, F] (backward)
    float* dx;             // [B, C, F] (backward)
    float* dgamma;         // [C] (backward)
    float* dbeta;          // [C] (backward)
    uint64_t seed;
    int B, C, F;
    uint32_t layer;
    float p, scale, momentum, eps;
};

// dropout multipliers of 4 consecutive elements starting at global index i (i % 4 == 0 when V == 4)
template <int V>
__device__ __forceinline__ void keep_scales(const BnArgs& a, long i, float* k) {
    if (a.mask) {
#pragma unroll
        for (int v = 0; v < V; ++v) k[v] = a.mask[i + v] * a.scale;
        return;
    }
    uint32_t r4[4];
    ttsc_philox4x32((uint32_t)(i >> 2), (uint32_t)(i >> 34), a.layer, TC_BN_TAG, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r4);
#pragma unroll
    for (int v = 0; v < V; ++v) k[v] = ttsc_u01(r4[(i + v) & 3]) >= a.p ? a.scale : 0.f;
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float* out) {
    if (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else {
        out[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
    if (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// element walk of channel c: vector j of the B x (F / V) vectors -> global index of its first element
__device__ __forceinline__ long chan_index(const BnArgs& a, int c, long j, int FV, int V) {
    const long b = j / FV, f = (j - b * FV) * V;
    return ((long)b * a.C + c) * a.F + f;
}

template <int V>
__global__ __launch_bounds__(TC_THREADS) void bn_tanh_dropout_fwd_kernel(const BnArgs a) {
    __shared__ double red[TC_THREADS / 64];
    const int c = blockIdx.x;
    const int FV = a.F / V;
    const long nv = (long)a.B * FV;
    const double n = (double)a.B * a.F;
    double s = 0.0;
    for (long j = threadIdx.x; j < nv; j += TC_THREADS) {
        float v[V];
        load_v<V>(a.x + chan_index(a, c, j, FV, V), v);
#pragma unroll
        for (int q = 0; q < V; ++q) s += (double)v[q];
    }
    const double mean = tc_block_sum(s, red) / n;
    double s2 = 0.0;
    for (long j = threadIdx.x; j < nv; j += TC_THREADS) {
        float v[V];
        load_v<V>(a.x + chan_index(a, c, j, FV, V), v);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const double d = (double)v[q] - mean;
            s2 += d * d;
        }
    }
    const double m2 = tc_block_sum(s2, red);
    const double var = m2 / n;
    const float meanf = (float)mean;
    const float inv = (float)(1.0 / sqrt(var + (double)a.eps));
    const float g = a.gamma[c], be = a.beta[c];
    for (long j = threadIdx.x; j < nv; j += TC_THREADS) {
        const long i = chan_index(a, c, j, FV, V);
        float v[V], k[V], o[V];
        load_v<V>(a.x + i, v);
        keep_scales<V>(a, i, k);
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = tanhf(g * ((v[q] - meanf) * inv) + be) * k[q];
        store_v<V>(a.y + i, o);
    }
    if (threadIdx.x == 0) {
        a.mean[c] = meanf;
        a.invstd[c] = inv;
        const float m = a.momentum;
        a.rmean[c] = m * meanf + (1.f - m) * a.rmean[c];
        a.rvar[c] = m * (float)(m2 / (n - 1.0)) + (1.f - m) * a.rvar[c];
    }
}

template <int V>
__global__ __launch_bounds__(TC_THREADS) void bn_tanh_dropout_bwd_kernel(const BnArgs a) {
    __shared__ double red[TC_THREADS / 64];
    const int c = blockIdx.x;
    const int FV = a.F / V;
    const long nv = (long)a.B * FV;
    const double n = (double)a.B * a.F;
    const float meanf = a.mean[c], inv = a.invstd[c];
    const float g = a.gamma[c], be = a.beta[c];
    double s1 = 0.0, s2 = 0.0;
    for (long j = threadIdx.x; j < nv; j += TC_THREADS) {
        const long i = chan_index(a, c, j, FV, V);
        float v[V], d[V], k[V];
        load_v<V>(a.x + i, v);
        load_v<V>(a.dy + i, d);
        keep_scales<V>(a, i, k);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float xh = (v[q] - meanf) * inv;
            const float t = tanhf(g * xh + be);
            const float dz = d[q] * k[q] * (1.f - t * t);
            s1 += (double)dz;
            s2 += (double)dz * (double)xh;
        }
    }
    const double sum_dz = tc_block_sum(s1, red);
    const double sum_dzx = tc_block_sum(s2, red);
    const float c1 = (float)(sum_dz / n), c2 = (float)(sum_dzx / n);
    const float gi = g * inv;
    for (long j = threadIdx.x; j < nv; j += TC_THREADS) {
        const long i = chan_index(a, c, j, FV, V);
        float v[V], d[V], k[V], o[V];
        load_v<V>(a.x + i, v);
        load_v<V>(a.dy + i, d);
        keep_scales<V>(a, i, k);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float xh = (v[q] - meanf) * inv;
            const float t = tanhf(g * xh + be);
            const float dz = d[q] * k[q] * (1.f - t * t);
            o[q] = gi * (dz - c1 - xh * c2);
        }
        store_v<V>(a.dx + i, o);
    }
    if (threadIdx.x == 0) {
        a.dgamma[c] = (float)sum_dzx;
        a.dbeta[c] = (float)sum_dz;
    }
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------
struct TcLossArgs {
    const float* ld;  const int64_t* td;  float* gd;  int Rd, Kd;      // duration logits [Rd, Kd], targets [Rd], gradient
    const float* lp;  const int64_t* tp;  float* gp;  int Rp, Kp;      // pitch
    const float* pre; const float* post;  const float* tm;  float* gpre;  float* gpost;  long n;   // mel [n] (n % 4 == 0)
    long ignore;
    int nbd, nbp, nbm;
    double* partial;     // [2 * grid]
    unsigned* ticket;
    float* out;          // [4] dur, pitch, mel pre, mel post
    int* status;
};

__global__ __launch_bounds__(TC_THREADS) void textcoder_loss_kernel(const TcLossArgs a) {
    __shared__ double red[TC_THREADS / 64];
    __shared__ bool last;
    const int blk = blockIdx.x;
    double v0 = 0.0, v1 = 0.0;
    if (blk < a.nbd) {
        const double cnt = count_valid(a.td, a.Rd, a.Kd, a.ignore, red);
        v0 = ce_rows(a.ld, a.td, a.gd, a.Rd, a.Kd, a.ignore, blk, a.nbd, (float)(1.0 / cnt), a.status, 1);
    } else if (blk < a.nbd + a.nbp) {
        const double cnt = count_valid(a.tp, a.Rp, a.Kp, a.ignore, red);
        v0 = ce_rows(a.lp, a.tp, a.gp, a.Rp, a.Kp, a.ignore, blk - a.nbd, a.nbp, (float)(1.0 / cnt), a.status, 2);
    } else {
        const int mb = blk - a.nbd - a.nbp;
        const float sc = (float)(1.0 / (double)a.n);
        const long n4 = a.n >> 2;
        for (long j = (long)mb * TC_THREADS + threadIdx.x; j < n4; j += (long)a.nbm * TC_THREADS) {
            const float4 p = reinterpret_cast<const float4*>(a.pre)[j];
            const float4 q = reinterpret_cast<const float4*>(a.post)[j];
            const float4 t = reinterpret_cast<const float4*>(a.tm)[j];
            const float dp[4] = {p.x - t.x, p.y - t.y, p.z - t.z, p.w - t.w};
            const float dq[4] = {q.x - t.x, q.y - t.y, q.z - t.z, q.w - t.w};
            float gp_[4], gq_[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v0 += (double)fabsf(dp[e]);
                v1 += (double)fabsf(dq[e]);
                gp_[e] = dp[e] > 0.f ? sc : (dp[e] < 0.f ? -sc : 0.f);
                gq_[e] = dq[e] > 0.f ? sc : (dq[e] < 0.f ? -sc : 0.f);
            }
            reinterpret_cast<float4*>(a.gpre)[j] = make_float4(gp_[0], gp_[1], gp_[2], gp_[3]);
            reinterpret_cast<float4*>(a.gpost)[j] = make_float4(gq_[0], gq_[1], gq_[2], gq_[3]);
        }
    }
    v0 = tc_block_sum(v0, red);
    v1 = tc_block_sum(v1, red);
    if (threadIdx.x == 0) {
        a.partial[2 * blk] = v0;
        a.partial[2 * blk + 1] = v1;
        __threadfence();
        last = atomicAdd(a.ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // fixed-order final sums by the last workgroup
    const int lo[3] = {0, a.nbd, a.nbd + a.nbp}, hi[3] = {a.nbd, a.nbd + a.nbp, (int)gridDim.x};
    double tot[4];
    for (int term = 0; term < 4; ++term) {
        const int seg = term < 2 ? term : 2, slot = term == 3 ? 1 : 0;
        double s = 0.0;
        for (int i = lo[seg] + threadIdx.x; i < hi[seg]; i += TC_THREADS)
            s += __hip_atomic_load(a.partial + 2 * i + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot[term] = tc_block_sum(s, red);
    }
    const double cd = count_valid(a.td, a.Rd, a.Kd, a.ignore, red);
    const double cp = count_valid(a.tp, a.Rp, a.Kp, a.ignore, red);
    if (threadIdx.x == 0) {
        // (0 / 0 = NaN when every row is ignored, as torch's mean reduction gives)
        a.out[0] = (float)(tot[0] / cd);
        a.out[1] = (float)(tot[1] / cp);
        a.out[2] = (float)(tot[2] / (double)a.n);
        a.out[3] = (float)(tot[3] / (double)a.n);
        *a.ticket = 0u;
    }
}

static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_bn_tanh_dropout_train_forward(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* running_mean_dev,
                                                  float* running_var_dev, int32_t B, int32_t C, int32_t F, float momentum, float eps, float p,
                                                  const float* mask_dev, uint64_t seed, int32_t layer, float* y_dev, float* mean_dev,
                                                  float* invstd_dev, void* stream) {
    TTSC_REQUIRE(x_dev && gamma_dev && beta_dev && running_mean_dev && running_var_dev && y_dev && mean_dev && invstd_dev,
                 "ttsc_bn_tanh_dropout_train_forward: null argument");
    TTSC_REQUIRE(B > 0 && C > 0 && F > 0, "ttsc_bn_tanh_dropout_train_forward: empty shape [%d, %d, %d]", B, C, F);
    TTSC_REQUIRE((int64_t)B * F > 1, "ttsc_bn_tanh_dropout_train_forward: expected more than 1 value per channel when training (B * F = %lld)",
                 (long long)B * F);
    TTSC_REQUIRE(p >= 0.f && p < 1.f, "ttsc_bn_tanh_dropout_train_forward: dropout p must lie in [0, 1)");
    BnArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.rmean = running_mean_dev; a.rvar = running_var_dev;
    a.y = y_dev; a.mean = mean_dev; a.invstd = invstd_dev; a.mask = mask_dev; a.seed = seed;
    a.B = B; a.C = C; a.F = F; a.layer = (uint32_t)layer; a.p = p; a.scale = (float)(1.0 / (1.0 - (double)p));
    a.momentum = momentum; a.eps = eps;
    const bool vec = (F % 4 == 0) && aligned16(x_dev) && aligned16(y_dev) && (!mask_dev || aligned16(mask_dev));
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(bn_tanh_dropout_fwd_kernel<4>, dim3((unsigned)C), dim3(TC_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(bn_tanh_dropout_fwd_kernel<1>, dim3((unsigned)C), dim3(TC_THREADS), 0, s, a);
    return check_launch("bn_tanh_dropout_fwd_kernel");
}

extern "C" int ttsc_bn_tanh_dropout_train_backward(const float* dy_dev, const float* x_dev, const float* gamma_dev, const float* beta_dev,
                                                   const float* mean_dev, const float* invstd_dev, int32_t B, int32_t C, int32_t F, float p,
                                                   const float* mask_dev, uint64_t seed, int32_t layer, float* dx_dev, float* dgamma_dev,
                                                   float* dbeta_dev, void* stream) {
    TTSC_REQUIRE(dy_dev && x_dev && gamma_dev && beta_dev && mean_dev && invstd_dev && dx_dev && dgamma_dev && dbeta_dev,
                 "ttsc_bn_tanh_dropout_train_backward: null argument");
    TTSC_REQUIRE(B > 0 && C > 0 && F > 0, "ttsc_bn_tanh_dropout_train_backward: empty shape [%d, %d, %d]", B, C, F);
    TTSC_REQUIRE(p >= 0.f && p < 1.f, "ttsc_bn_tanh_dropout_train_backward: dropout p must lie in [0, 1)");
    BnArgs a{};
    a.x = x_dev; a.gamma = gamma_dev; a.beta = beta_dev; a.mean = const_cast<float*>(mean_dev); a.invstd = const_cast<float*>(invstd_dev);
    a.mask = mask_dev; a.seed = seed; a.dy = dy_dev; a.dx = dx_dev; a.dgamma = dgamma_dev; a.dbeta = dbeta_dev;
    a.B = B; a.C = C; a.F = F; a.layer = (uint32_t)layer; a.p = p; a.scale = (float)(1.0 / (1.0 - (double)p));
    const bool vec = (F % 4 == 0) && aligned16(x_dev) && aligned16(dy_dev) && aligned16(dx_dev) && (!mask_dev || aligned16(mask_dev));
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(bn_tanh_dropout_bwd_kernel<4>, dim3((unsigned)C), dim3(TC_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(bn_tanh_dropout_bwd_kernel<1>, dim3((unsigned)C), dim3(TC_THREADS), 0, s, a);
    return check_launch("bn_tanh_dropout_bwd_kernel");
}

static void tc_loss_grid(int32_t Rd, int32_t Rp, int64_t n, int* nbd, int* nbp, int* nbm) {
    *nbd = (int)std::min<int64_t>(ceil_div(Rd, 4), 256);
    *nbp = (int)std::min<int64_t>(ceil_div(Rp, 4), 512);
    *nbm = (int)std::max<int64_t>(std::min<int64_t>(ceil_div(n / 4, 4 * TC_THREADS), 512), 1);
}

extern "C" size_t ttsc_textcoder_loss_workspace_bytes(int32_t Rd, int32_t Rp, int64_t n) {
    int nbd, nbp, nbm;
    tc_loss_grid(Rd, Rp, n, &nbd, &nbp, &nbm);
    return 64 + (size_t)(nbd + nbp + nbm) * 2 * sizeof(double);
}

extern "C" int ttsc_textcoder_loss(const float* dur_logits_dev, const int64_t* dur_target_dev, int32_t Rd, int32_t Kd, const float* pitch_logits_dev,
                                   const int64_t* pitch_target_dev, int32_t Rp, int32_t Kp, const float* pre_dev, const float* post_dev,
                                   const float* mel_target_dev, int64_t n, int64_t ignore_index, float* out_dev, float* g_dur_dev,
                                   float* g_pitch_dev, float* g_pre_dev, float* g_post_dev, int32_t* status_dev, void* ws_dev, size_t ws_bytes,
                                   void* stream) {
    TTSC_REQUIRE(out_dev && status_dev && ws_dev, "ttsc_textcoder_loss: null argument");
    TTSC_REQUIRE(Rd >= 0 && Rp >= 0 && n > 0 && n % 4 == 0, "ttsc_textcoder_loss: bad sizes (Rd %d, Rp %d, n %lld; n must be a positive multiple of 4)",
                 Rd, Rp, (long long)n);
    TTSC_REQUIRE(Rd == 0 || (dur_logits_dev && dur_target_dev && g_dur_dev && Kd > 0), "ttsc_textcoder_loss: duration operands");
    TTSC_REQUIRE(Rp == 0 || (pitch_logits_dev && pitch_target_dev && g_pitch_dev && Kp > 0), "ttsc_textcoder_loss: pitch operands");
    TTSC_REQUIRE(pre_dev && post_dev && mel_target_dev && g_pre_dev && g_post_dev, "ttsc_textcoder_loss: mel operands");
    TTSC_REQUIRE(aligned16(pre_dev) && aligned16(post_dev) && aligned16(mel_target_dev) && aligned16(g_pre_dev) && aligned16(g_post_dev),
                 "ttsc_textcoder_loss: mel operands must be 16-byte aligned");
    TTSC_REQUIRE(ws_bytes >= ttsc_textcoder_loss_workspace_bytes(Rd, Rp, n), "ttsc_textcoder_loss: workspace too small");
    TcLossArgs a{};
    a.ld = dur_logits_dev; a.td = dur_target_dev; a.gd = g_dur_dev; a.Rd = Rd; a.Kd = Kd;
    a.lp = pitch_logits_dev; a.tp = pitch_target_dev; a.gp = g_pitch_dev; a.Rp = Rp; a.Kp = Kp;
    a.pre = pre_dev; a.post = post_dev; a.tm = mel_target_dev; a.gpre = g_pre_dev; a.gpost = g_post_dev; a.n = n;
    a.ignore = ignore_index;
    tc_loss_grid(Rd, Rp, n, &a.nbd, &a.nbp, &a.nbm);
    if (Rd == 0) a.nbd = 0;
    if (Rp == 0) a.nbp = 0;
    a.ticket = (unsigned*)ws_dev;
    a.partial = (double*)((char*)ws_dev + 64);
    a.out = out_dev;
    a.status = status_dev;
    hipStream_t s = (hipStream_t)stream;
    TTSC_HIP_CHECK(hipMemsetAsync(ws_dev, 0, 64, s));
    TTSC_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(textcoder_loss_kernel, dim3((unsigned)(a.nbd + a.nbp + a.nbm)), dim3(TC_THREADS), 0, s, a);
    return check_launch("textcoder_loss_kernel");
}
