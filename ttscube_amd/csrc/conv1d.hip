// Conv1d / ConvTranspose1d as an fp32-MFMA implicit GEMM for gfx950 (CDNA4).
//
//   out[b, co, q*os + oo] = act( ( bias[co] + resid + sum_{j<ntaps} sum_{ci} W_j[co, ci] *
//                                  lrelu(in_scale * x[b, ci, q + tap_base + j*tap_step]) ) * out_scale )
//
// A plain (dilated) Conv1d is one launch with tap_step = dilation, tap_base = -padding, os = 1.
// A ConvTranspose1d with stride s is s polyphase launches: phase r owns outputs o with
// (o + p) % s == r, its taps are k = r + j*s and it reads x[q - j]  (tap_step = -1).
//
// GEMM view per workgroup: M = output channels (MT rows), N = NT consecutive q positions, K = Cin*ntaps.
// v_mfma_f32_32x32x2_f32 is an exact k-ordered fp32 fmaf chain at the fp32 vector rate (157 TF/chip).  The B operand
// (activations, with the dilation halo) is staged per 16-channel chunk through double-buffered LDS with the leaky-relu
// prologue fused into the staging pass, the A operand (weights) is pre-packed into MFMA fragment order (on the host for
// inference, by pack_w_kernel from the live parameter for training) so every fragment is ONE coalesced 256-byte wave load
// that hits L2; both streams are software-pipelined explicitly (see conv_mfma_kernel).  Epilogue fuses bias, residual
// add, scaling, tanh, the running sum over residual blocks and — for data-gradient launches — the leaky-relu derivative.
// The split-precision kernels (conv_f16x3_kernel in conv_kernels.hpp, the wide / tall kernels in conv_f16x3_widetall.hpp, respair32_f16x3_kernel
// below) are the default for the generator.  This file keeps the C ABI, the weight packing and the forward dispatcher.
#include <climits>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "conv_f16x3_widetall.hpp"
#include "conv_kernels.hpp"

namespace ttsc {

// ---------------------------------------------------------------------------------------------------------------
// Fused residual pair for 32-channel stages (HiFi-GAN ResBlock1, last upsample stage):
//     y = x + conv2_{d=1}( lrelu( conv1_{d}( lrelu(x) ) ) )          [ + running sum ]
// The 32-channel stage is HBM-bound when its two convolutions run as separate launches (24..88 FLOP per byte moved);
// here the inner activation never leaves the CU: conv1 is evaluated on a 512-column grid (480 outputs + 16 columns of
// margin on each side, >= conv2's halo), its result is leaky-relu'ed, split into fp16 hi/lo and parked in LDS as
// [position][32 ch], and conv2 runs straight out of LDS.  Per pair the HBM traffic drops from 5 tensor passes to ~3.2.
// 8 waves side by side along time (2 MFMA column tiles each); with only 32 output channels the weight fragments of a
// 16-channel chunk fit in registers (K taps x hi/lo x 4 VGPRs), so the tap loop has no barriers and reads only the
// activation fragments from LDS.  K (3/7/11) is a template parameter so that the register-resident fragments are
// statically indexed.
struct PairArgs {
    const float* x;      // [B, 32, L]   input AND residual
    float* y;            // [B, 32, L]   must not alias x (neighbouring tiles read x's halo)
    const void* w1;      // f16x3 fragments of conv1 / conv2: [tap][2 chunks][1][2][64][8 half]
    const void* w2;
    const float* b1;
    const float* b2;
    const int* len;      // [B] valid length or null
    float unscale1, unscale2;
    int L, d1, accumulate;
};

template <int K, int NW>
__global__ __launch_bounds__(64 * NW, (NW == 8 ? 2 : 2)) void respair32_f16x3_kernel(PairArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int C = 32, NCOL = 64 * NW, MARG = 16, NTO = NCOL - 2 * MARG, XTP = NCOL + 16, H2 = (K - 1) / 2, NTHR = 64 * NW;
    const int span1 = NCOL + (K - 1) * a.d1;
    // plane layouts as in conv_f16x3_kernel: X planes (h, pl) of span1 items; T planes (chunk c, h, pl) of XTP items
    half8* Xp = reinterpret_cast<half8*>(smem_raw);
    half8* Tp = Xp + (size_t)4 * span1;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * NTO;
    const int lin = a.len ? a.len[b] : a.L;
    if (q0 >= lin) return;
    const int h1 = a.d1 * (K - 1) / 2;
    const int lo = q0 - MARG - h1;  // x position of X-LDS column 0
    const float* xb = a.x + (size_t)b * C * a.L;

    f32x16 acc[2];
    half8 ah[K], al[K];

    constexpr int XIT = ((NCOL + 64) * 2 + NTHR - 1) / NTHR;
    const int spanp = (span1 + 63) & ~63;
    float xr[XIT][8];
    auto x_issue = [&](int c) {
#pragma unroll
        for (int e = 0; e < XIT; ++e) {
            const int i = tid + e * NTHR;
            const int h = i >= spanp ? 1 : 0;
            const int p = i - h * spanp;
            int pos = lo + p;
            pos = pos > lin - 1 ? lin - 1 : pos;
            pos = pos < 0 ? 0 : pos;
            const int cb = c * 16 + h * 8;
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) xr[e][ch] = xb[(size_t)(cb + ch) * a.L + pos];
        }
    };
    auto x_commit = [&]() {
#pragma unroll
        for (int e = 0; e < XIT; ++e) {
            const int i = tid + e * NTHR;
            const int h = i >= spanp ? 1 : 0;
            const int p = i - h * spanp;
            const int pos = lo + p;
            const bool pok = pos >= 0 && pos < lin;
            if (p < span1 && i < 2 * spanp) {
                half8 vh, vl;
#pragma unroll
                for (int ch = 0; ch < 8; ++ch) {
                    float v = pok ? xr[e][ch] : 0.f;
                    v = fmaxf(v, v * 0.1f);
                    const _Float16 hh = (_Float16)v;
                    vh[ch] = hh;
                    vl[ch] = (_Float16)(v - (float)hh);
                }
                Xp[(size_t)(h * 2 + 0) * span1 + p] = vh;
                Xp[(size_t)(h * 2 + 1) * span1 + p] = vl;
            }
        }
    };
    auto load_a = [&](const void* w, int c) {
        const half8* src = reinterpret_cast<const half8*>(w);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            ah[j] = src[(size_t)(j * 2 + c) * 128 + lane];
            al[j] = src[(size_t)(j * 2 + c) * 128 + 64 + lane];
        }
    };

    // ---------------- conv1 (dilated) over the 512-column grid ----------------
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    x_issue(0);
    for (int c = 0; c < 2; ++c) {
        load_a(a.w1, c);
        if (c) __syncthreads();  // everyone finished reading chunk 0 of the activation tile
        x_commit();
        __syncthreads();
        if (c == 0) x_issue(1);
        const half8* xh = Xp + (unsigned)((half * 2 + 0) * span1 + wv * 64 + l31);
        const half8* xl = Xp + (unsigned)((half * 2 + 1) * span1 + wv * 64 + l31);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const half8 bh0 = xh[j * a.d1], bh1 = xh[j * a.d1 + 32];
            const half8 bl0 = xl[j * a.d1], bl1 = xl[j * a.d1 + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[j], bh0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[j], bh1, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bl0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bl1, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bh0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bh1, acc[1], 0, 0, 0);
        }
    }
    // conv1 epilogue -> LDS: xt = lrelu(conv1 + b1), zero outside the sequence (conv2 pads with zeros), hi/lo split.
    // A lane holds channels {4*half + (r&3) + 8*(r>>2)} of its column: four groups of 4 consecutive channels.
    load_a(a.w2, 0);  // conv2's first weight chunk travels while the epilogue runs
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int col = wv * 64 + n * 32 + l31;
        const int pos = q0 - MARG + col;
        const bool pok = pos >= 0 && pos < lin;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            typedef _Float16 half4 __attribute__((ext_vector_type(4)));
            half4 vh, vl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ch = 8 * g + 4 * half + e;
                float v = acc[n][4 * g + e] * a.unscale1 + a.b1[ch];
                v = fmaxf(v, v * 0.1f);
                v = pok ? v : 0.f;
                const _Float16 hh = (_Float16)v;
                vh[e] = hh;
                vl[e] = (_Float16)(v - (float)hh);
            }
            // channel group g (8 channels) = chunk g/2, channel-half g%2; this lane owns 4 of its 8 channels
            _Float16* th = reinterpret_cast<_Float16*>(Tp + (size_t)(g * 2 + 0) * XTP + (col + 8)) + 4 * half;
            _Float16* tl = reinterpret_cast<_Float16*>(Tp + (size_t)(g * 2 + 1) * XTP + (col + 8)) + 4 * half;
            *reinterpret_cast<half4*>(th) = vh;
            *reinterpret_cast<half4*>(tl) = vl;
        }
    }
    __syncthreads();
    // ---------------- conv2 (dilation 1) straight out of LDS ----------------
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    for (int c = 0; c < 2; ++c) {
        if (c) load_a(a.w2, 1);
        const half8* th = Tp + (unsigned)(((c * 2 + half) * 2 + 0) * XTP + wv * 64 + l31 + 8 - H2);
        const half8* tl = Tp + (unsigned)(((c * 2 + half) * 2 + 1) * XTP + wv * 64 + l31 + 8 - H2);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const half8 bh0 = th[j], bh1 = th[j + 32];
            const half8 bl0 = tl[j], bl1 = tl[j + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[j], bh0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[j], bh1, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bl0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bl1, acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bh0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[j], bh1, acc[1], 0, 0, 0);
        }
    }
    // conv2 epilogue: + b2 + x (residual) [+ running sum]; only the 480 central columns are outputs
    ConvArgs ea;
    ea.y = a.y;
    ea.resid = a.x;
    ea.bias = a.b2;
    ea.Cout = C;
    ea.Lout = a.L;
    ea.out_scale = 1.f;
    ea.out_act = TTSC_ACT_NONE;
    ea.accumulate = a.accumulate;
    ea.dbg = 0;
    ea.acc_init = 0;
    ea.epi_prefetch = 0;
    ea.swz_nx = ea.swz_ny = 0;
    ea.gate = nullptr;
    ea.gate_slope = 1.f;
    ea.vphase = 0;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int col = wv * 64 + n * 32 + l31;
        const int q = q0 + col - MARG;
        const bool qok = col >= MARG && col < MARG + NTO && q < lin;
        epilogue_tile(acc[n], ea, b, 0, q, qok, half, a.unscale2);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Single-output-channel Conv1d (HiFi-GAN conv_post: 32 -> 1, K = 7, tanh): an M = 1 problem wastes 31/32 of an MFMA
// tile and its time goes into staging, so it runs on the vector ALU as an fp32 fmaf chain (ci-major, tap-minor) and is
// bound by the one HBM read of its input.  1024 outputs per workgroup; 8-channel chunks of the activated input window
// go through LDS (coalesced dword loads in, conflict-free ds_read_b128 out); a thread owns 4 consecutive outputs.
__global__ __launch_bounds__(256) void conv_cout1_kernel(ConvArgs a) {
    constexpr int NT = 1024, CH = 8, HALO = 16;          // HALO >= (K - 1) * dilation, K <= 16, dilation 1
    __shared__ __attribute__((aligned(16))) float xs[CH][NT + 2 * HALO];
    __shared__ float ws[64 * 16];
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, b = blockIdx.y;
    const int q0 = blockIdx.x * NT;
    const int lin = a.in_len ? a.in_len[b] : a.Lin;
    if (a.out_len && q0 >= a.out_len[b]) return;
    const int K = a.ntaps;
    for (int i = tid; i < a.Cin * K; i += 256) ws[i] = a.wp[i];     // plain [Cin][K] fp32 weights (see conv_repack)
    const float* xb = a.x + (size_t)b * a.Cin * a.Lin;
    const int lo = q0 + a.tap_base;                                  // x position of LDS column 0
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < a.Cin; c0 += CH) {
        __syncthreads();
        // stage 8 channel rows: every thread issues 8 x 5 independent, clamped, unconditional loads (no integer division, no
        // branch around a load — the first version of this loop ran one dependent load at a time), then activates and stores
        {
            constexpr int PER = (NT + 2 * HALO + 255) / 256;   // 5 columns per thread and row
            float v[CH][PER];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ci = c0 + c < a.Cin ? c0 + c : a.Cin - 1;
                const float* row = xb + (size_t)ci * a.Lin;
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    int pos = lo + tid + k * 256;
                    pos = pos < 0 ? 0 : (pos > a.Lin - 1 ? a.Lin - 1 : pos);
                    v[c][k] = row[pos];
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const int p = tid + k * 256, pos = lo + p;
                    float t = v[c][k] * a.in_scale;
                    t = fmaxf(t, t * a.in_slope);
                    if (p < NT + 2 * HALO) xs[c][p] = (c0 + c < a.Cin && pos >= 0 && pos < lin) ? t : 0.f;
                }
        }
        __syncthreads();
        const int nc = a.Cin - c0 < CH ? a.Cin - c0 : CH;
        for (int c = 0; c < nc; ++c) {
            // outputs 4*tid .. 4*tid+3 read window columns 4*tid .. 4*tid + 3 + K - 1  (<= 4*tid + 18)
            float w[20];
#pragma unroll
            for (int v4 = 0; v4 < 5; ++v4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(&xs[c][4 * tid + 4 * v4]);
                w[4 * v4] = t[0]; w[4 * v4 + 1] = t[1]; w[4 * v4 + 2] = t[2]; w[4 * v4 + 3] = t[3];
            }
            const float* wk = ws + (c0 + c) * K;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < K) {
                    const float wj = wk[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = fmaf(wj, w[e + j], acc[e]);
                }
            }
        }
    }
    const float bv = a.bias ? a.bias[0] : 0.f;
    float* yb = a.y + (size_t)b * a.Lout;
    const float* rb = a.resid ? a.resid + (size_t)b * a.Lout : nullptr;
    const int q = q0 + 4 * tid;
    float res[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool ok = q + e < a.Lout;
        float t = (acc[e] + bv + (rb && ok ? rb[q + e] : 0.f)) * a.out_scale;
        t = apply_act(t, a.out_act);
        res[e] = t + (a.accumulate && ok ? yb[q + e] : 0.f);
    }
    if (a.nf_flag) {
        // range guard of the split-precision generator: an fp16 overflow anywhere upstream reaches the waveform as NaN (the hi and
        // lo halves of an overflowed value are +inf and -inf, their products cancel to NaN), so one test per output sample on this
        // HBM-bound kernel covers every layer (hifigan.cpp re-calibrates and reruns when the word is set)
        bool bad = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) bad = bad || (q + e < a.Lout && !(fabsf(res[e]) <= 3.0e38f));
        if (bad) atomicOr(a.nf_flag, 1u);
    }
    if (q + 3 < a.Lout && (((uintptr_t)(yb + q)) & 15) == 0) {
        const f32x4 o = {res[0], res[1], res[2], res[3]};
        *reinterpret_cast<f32x4*>(yb + q) = o;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q + e < a.Lout) yb[q + e] = res[e];
    }
}

template <int MI, int NJ, int TMAX>
static int launch_f16_t(const ConvArgs& a, int B, hipStream_t s) {
    constexpr int NT = 4 * NJ * 32;
    constexpr int MT = MI * 32;
    dim3 grid((unsigned)ceil_div(a.q_cnt, NT), (unsigned)(a.CoutP / MT), (unsigned)B);
    const size_t lds = (size_t)a.span_pad * 4 * 16 + (size_t)a.ntaps * MI * 2 * 64 * 16;
    if (int rc = ensure_full_lds((const void*)conv_f16x3_kernel<MI, NJ, TMAX>)) return rc;   // once per (device, kernel)
    hipLaunchKernelGGL((conv_f16x3_kernel<MI, NJ, TMAX>), grid, dim3(256), lds, s, a);
    return launch_checked("conv_f16x3_kernel");
}

template <int MI, int NJ>
static int launch_f16(const ConvArgs& a, int B, hipStream_t s) {
    if (a.ntaps <= 3) return launch_f16_t<MI, NJ, 3>(a, B, s);
    if (a.ntaps <= 7) return launch_f16_t<MI, NJ, 7>(a, B, s);
    if (a.ntaps <= 11) return launch_f16_t<MI, NJ, 11>(a, B, s);
    return launch_f16_t<MI, NJ, 16>(a, B, s);
}

template <int MI, int NJ, int WM, int WN>
static int launch_cfg(const ConvArgs& a, int B, hipStream_t s) {
    constexpr int NT = WN * NJ * 32;
    constexpr int MT = WM * MI * 32;
    dim3 grid((unsigned)ceil_div(a.q_cnt, NT), (unsigned)(a.CoutP / MT), (unsigned)B);
    dim3 block(WM * WN * 64);
    size_t lds = (size_t)2 * KC * a.span_pad * sizeof(float);
    TTSC_REQUIRE(lds <= 160 * 1024, "conv_mfma_kernel: receptive field too large for LDS (%zu bytes)", lds);
    if (lds > 64 * 1024)
        if (int rc = ensure_full_lds(reinterpret_cast<const void*>(conv_mfma_kernel<MI, NJ, WM, WN>))) return rc;
    hipLaunchKernelGGL((conv_mfma_kernel<MI, NJ, WM, WN>), grid, block, lds, s, a);
    return launch_checked("conv_mfma_kernel");
}

static long env_num(const char* name, long unset) {
    const char* ev = getenv(name);
    return ev ? atol(ev) : unset;
}

// The ONE place that reads the environment switches of the convolution dispatch (docs/KERNELS.md lists them); conv_plan decides from the values.
static ConvSwitches conv_switches() {
    // measurement switches, read once per process
    static const ConvSwitches once = [] {
        ConvSwitches s;
        s.big_only = env_num("TTSC_F16_TILE", 1) == 0;
        s.acc_init = (int)env_num("TTSC_CONV_ACC_INIT", 1);
        s.tall = env_num("TTSC_CONV_TALL", 1) != 0;
        s.want = env_num("TTSC_CONV_WANT", 512);
        s.narrow = (int)env_num("TTSC_CONV_NARROW", 1);
        s.epi_prefetch = (int)env_num("TTSC_CONV_EPI_PREFETCH", 1);
        s.tall_swizzle = (int)env_num("TTSC_TALL_SWIZZLE", 1);
        return s;
    }();
    // test switches, read at every launch so that one process can compare the variants
    ConvSwitches s = once;
    s.wide = (int)env_num("TTSC_CONV_WIDE", 1);
    s.lean = env_num("TTSC_CONV_LEAN", 1) != 0;
    // TTSC_CONV_TILE=<rows>x<cols> forces the tile of the general split kernel and of the fp32 kernel (tests: every tile variant at small shapes).
    // A tile the layer cannot take is an error at the launch, never another tile: the error is what proves which variant ran.
    if (const char* ev = getenv("TTSC_CONV_TILE"); ev && *ev) {
        char x = 0, tail = 0;
        const bool ok = sscanf(ev, "%d%c%d%c", &s.tile_rows, &x, &s.tile_cols, &tail) == 3 && (x == 'x' || x == 'X') && s.tile_rows > 0 && s.tile_cols > 0;
        s.tile_state = ok ? 1 : -1;
        s.tile_text = ev;
    }
    return s;
}

static int pick_mt(int Cout) {
    int best = 32, best_pad = (int)round_up(Cout, 32);
    for (int mt : {64, 128}) {
        int pad = (int)round_up(Cout, mt);
        if (pad <= best_pad) {
            best = mt;
            best_pad = pad;
        }
    }
    return best;
}

}  // namespace ttsc

using namespace ttsc;

#include "conv_internal.hpp"

extern "C" int ttsc_conv1d_create(const ttsc_conv1d_cfg* cfg, ttsc_conv1d** out) {
    TTSC_REQUIRE(cfg && out, "ttsc_conv1d_create: null argument");
    TTSC_REQUIRE(cfg->in_channels > 0 && cfg->out_channels > 0 && cfg->kernel_size > 0,
                 "ttsc_conv1d_create: bad channels/kernel (%d,%d,%d)", cfg->in_channels, cfg->out_channels,
                 cfg->kernel_size);
    TTSC_REQUIRE(cfg->stride >= 1 && cfg->dilation >= 1 && cfg->padding >= 0, "ttsc_conv1d_create: bad stride/dilation/padding");
    if (cfg->transposed) {
        TTSC_REQUIRE(cfg->dilation == 1, "ttsc_conv1d_create: ConvTranspose1d supports dilation 1 only");
    } else {
        TTSC_REQUIRE(cfg->stride == 1, "ttsc_conv1d_create: Conv1d supports stride 1 only");
    }
    const int groups = cfg->groups > 1 ? cfg->groups : 1;
    if (groups > 1) {
        TTSC_REQUIRE(!cfg->transposed, "ttsc_conv1d_create: groups need a Conv1d");
        TTSC_REQUIRE(cfg->in_channels % groups == 0 && cfg->out_channels % groups == 0, "ttsc_conv1d_create: channels (%d, %d) not divisible by groups %d",
                     cfg->in_channels, cfg->out_channels, groups);
    }
    ttsc_conv1d* c = new ttsc_conv1d();
    c->cfg = *cfg;
    c->cfg.groups = groups;
    c->vfused = cfg->transposed && (cfg->out_channels % 32 == 0) && cfg->stride > 1;
    c->CoutV = c->vfused ? cfg->stride * cfg->out_channels : cfg->out_channels;
    c->MT = pick_mt(c->CoutV);
    c->groups = groups;
    c->cin_g = cfg->in_channels / groups;
    c->cout_g = cfg->out_channels / groups;
    c->cin_tile = cfg->in_channels;
    if (groups > 1) {
        // an M tile must not straddle a group boundary unless it holds whole groups
        c->MT = c->cout_g >= 128 && c->cout_g % 128 == 0 ? 128 : (c->cout_g >= 64 && c->cout_g % 64 == 0 ? 64 : 32);
        if (!(c->cout_g % c->MT == 0 || c->MT % c->cout_g == 0)) {
            delete c;
            set_error("ttsc_conv1d_create: %d output channels per group do not tile into 32-row blocks", cfg->out_channels / groups);
            return TTSC_EINVAL;
        }
        c->cin_tile = (c->MT > c->cout_g ? c->MT / c->cout_g : 1) * c->cin_g;
    }
    c->NT = c->MT == 128 ? 128 : (c->MT == 64 ? 256 : 512);
    c->CinP = (int)round_up(c->cin_tile, KC);
    c->CoutP = (int)round_up(c->CoutV, c->MT);
    *out = c;
    return TTSC_OK;
}

static void free_phases(ttsc_conv1d* c) {
    for (auto& p : c->phases) {
        if (p.wp_dev) (void)hipFree(p.wp_dev);
        if (p.wph_dev) (void)hipFree(p.wph_dev);
    }
    c->phases.clear();
}

extern "C" void ttsc_conv1d_destroy(ttsc_conv1d* c) {
    if (!c) return;
    free_phases(c);
    if (c->bias_dev) (void)hipFree(c->bias_dev);
    if (c->w_plain_dev) (void)hipFree(c->w_plain_dev);
    delete c;
}

extern "C" int64_t ttsc_conv1d_out_len(const ttsc_conv1d* c, int64_t Lin) {
    if (!c) return TTSC_EINVAL;
    const auto& g = c->cfg;
    if (g.transposed) return (Lin - 1) * g.stride - 2 * g.padding + g.kernel_size;
    return Lin + 2 * g.padding - g.dilation * (g.kernel_size - 1);
}

// Pack W into MFMA A-fragment order: [tap][CinP/2][CoutP/32][lane], lane -> (co = cot*32 + (lane&31), ci = 2*cip + (lane>>5))
static void pack_phase(const ttsc_conv1d* c, const float* w, const std::vector<int>& taps_k, std::vector<float>& out) {
    const auto& g = c->cfg;
    const int Cin = g.in_channels, Cout = g.out_channels, K = g.kernel_size;
    const int cipN = c->CinP / 2, cotN = c->CoutP / 32;
    out.assign((size_t)taps_k.size() * cipN * cotN * 64, 0.f);
    for (size_t j = 0; j < taps_k.size(); ++j) {
        const int k = taps_k[j];
        for (int cip = 0; cip < cipN; ++cip)
            for (int cot = 0; cot < cotN; ++cot)
                for (int lane = 0; lane < 64; ++lane) {
                    int co = cot * 32 + (lane & 31);
                    const int ci = 2 * cip + (lane >> 5);
                    int kk = k;
                    bool ok = co < c->CoutV && ci < Cin;
                    if (c->vfused) {   // virtual row = phase r * Cout + co, tap index k -> kernel tap r + k*stride
                        const int r = co / Cout;
                        co -= r * Cout;
                        kk = r + k * g.stride;
                        ok = ok && kk < K;
                    }
                    float v = 0.f;
                    if (c->groups > 1) {   // ci counts from the first input channel of the row tile's group(s); weight [Cout, cin_g, K]
                        const int gco = co / c->cout_g, cig = ((co / c->MT) * c->MT / c->cout_g) * c->cin_g + ci;
                        ok = co < Cout && ci < c->cin_tile && cig / c->cin_g == gco;
                        if (ok) v = w[((size_t)co * c->cin_g + (cig - gco * c->cin_g)) * K + kk];
                    } else if (ok) v = g.transposed ? w[((size_t)ci * Cout + co) * K + kk] : w[((size_t)co * Cin + ci) * K + kk];
                    out[(((size_t)j * cipN + cip) * cotN + cot) * 64 + lane] = v;
                }
    }
}

// f16x3 packing: [tap][CinP/16][CoutP/32][2 (hi,lo)][64 lanes][8 half]; lane -> co = cot*32 + (lane&31),
// ci = 16*chunk + 8*(lane>>5) + e.  Weights are multiplied by `scale` (a power of two) before the split.
static void pack_phase_f16(const ttsc_conv1d* c, const float* w, const std::vector<int>& taps_k, float scale,
                           std::vector<_Float16>& out) {
    const auto& g = c->cfg;
    const int Cin = g.in_channels, Cout = g.out_channels, K = g.kernel_size;
    const int nch = c->CinP / 16, cotN = c->CoutP / 32;
    out.assign((size_t)taps_k.size() * nch * cotN * 2 * 64 * 8, (_Float16)0.f);
    for (size_t j = 0; j < taps_k.size(); ++j) {
        const int k = taps_k[j];
        for (int ch = 0; ch < nch; ++ch)
            for (int cot = 0; cot < cotN; ++cot)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        int co = cot * 32 + (lane & 31);
                        const int ci = ch * 16 + 8 * (lane >> 5) + e;
                        int kk = k;
                        bool ok = co < c->CoutV && ci < Cin;
                        if (c->vfused && c->vrow4) {   // rows interleaved co * 4 + r (see epilogue_tile_v4)
                            const int r = co & 3;
                            co >>= 2;
                            kk = r + k * g.stride;
                            ok = ok && kk < K;
                        } else if (c->vfused) {
                            const int r = co / Cout;
                            co -= r * Cout;
                            kk = r + k * g.stride;
                            ok = ok && kk < K;
                        }
                        float v = 0.f;
                        if (ok) v = g.transposed ? w[((size_t)ci * Cout + co) * K + kk] : w[((size_t)co * Cin + ci) * K + kk];
                        v *= scale;
                        const _Float16 hi = (_Float16)v;
                        const _Float16 lo = (_Float16)(v - (float)hi);
                        const size_t base = ((((size_t)j * nch + ch) * cotN + cot) * 2) * 64 * 8;
                        out[base + (size_t)lane * 8 + e] = hi;
                        out[base + (size_t)64 * 8 + (size_t)lane * 8 + e] = lo;
                    }
    }
}

static int conv_repack(ttsc_conv1d* c);

extern "C" int ttsc_conv1d_set_precision(ttsc_conv1d* c, int32_t precision) {
    TTSC_REQUIRE(c, "ttsc_conv1d_set_precision: null argument");
    TTSC_REQUIRE(precision == TTSC_PREC_FP32 || precision == TTSC_PREC_F16X3, "ttsc_conv1d_set_precision: unknown precision %d", precision);
    // the split kernel prefetches a fixed-size register window: tile + 64 positions of halo.  Layers with a larger
    // receptive field (none on the hot path) silently stay on the exact fp32 kernel.
    const int halo = c->cfg.transposed ? (c->cfg.kernel_size + c->cfg.stride - 1) / c->cfg.stride - 1
                                       : (c->cfg.kernel_size - 1) * c->cfg.dilation;
    const int taps = c->cfg.transposed ? (c->cfg.kernel_size + c->cfg.stride - 1) / c->cfg.stride : c->cfg.kernel_size;
    if (precision == TTSC_PREC_F16X3 && (halo > 64 || taps > 16 || c->groups > 1)) precision = TTSC_PREC_FP32;   // (grouped layers: fp32 kernel only)
    if (precision == c->precision) return TTSC_OK;
    TTSC_REQUIRE(!c->dev_weights, "ttsc_conv1d_set_precision: weights were set from device memory; switch the precision first");
    c->precision = precision;
    // kernel_size == stride == 4 (the last two upsamplers of HiFi-GAN V1): the split path interleaves the virtual rows so that a lane's
    // accumulator registers are four consecutive output samples (epilogue_tile_v4).  The precision changes nowhere else.
    c->vrow4 = conv_vrow4(c->cfg, c->vfused, precision);
    return c->has_weight ? conv_repack(c) : TTSC_OK;
}

extern "C" int ttsc_conv1d_set_weight(ttsc_conv1d* c, const float* w, const float* bias) {
    TTSC_REQUIRE(c && w, "ttsc_conv1d_set_weight: null argument");
    const auto& g0 = c->cfg;
    c->w_host.assign(w, w + (size_t)c->cin_g * g0.out_channels * g0.kernel_size);   // torch layout: [Cout, Cin / groups, K]
    c->has_bias = bias != nullptr;
    if (bias) c->b_host.assign(bias, bias + g0.out_channels);
    c->dev_weights = false;
    return conv_repack(c);
}

// Device-side packing for training: the weights change every optimizer step, so the fragment order is produced by a
// gather kernel straight from the torch parameter (same mapping as pack_phase above), no host round trip.
namespace ttsc {
struct PackArgs {
    const float* w;
    float* out;
    int Cin, Cout, K, CoutV, cipN, cotN, ntaps, k0, kstep, transposed, vfused, stride;
    int flipT;   // source is the forward weight [Cin(this), Cout(this), K] of the layer this handle differentiates
    int groups, cin_g, cout_g, cin_tile, MT;   // grouped Conv1d: see ttsc_conv1d (conv_internal.hpp)
};
__global__ void pack_w_kernel(PackArgs p) {
    const long total = (long)p.ntaps * p.cipN * p.cotN * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        long t = i >> 6;
        const int cot = (int)(t % p.cotN);
        t /= p.cotN;
        const int cip = (int)(t % p.cipN);
        const int j = (int)(t / p.cipN);
        int co = cot * 32 + (lane & 31);
        const int ci = 2 * cip + (lane >> 5);
        int kk = p.k0 + j * p.kstep;
        bool ok = co < p.CoutV && ci < p.Cin;
        if (p.vfused) {
            const int r = co / p.Cout;
            co -= r * p.Cout;
            kk = r + (p.k0 + j * p.kstep) * p.stride;
            ok = ok && kk < p.K;
        }
        float v = 0.f;
        if (p.groups > 1) {
            // ci counts from the first input channel of the row tile's group(s).  Forward weight [Cout, cin_g, K]; as the data
            // gradient of a grouped layer the source is THAT layer's weight [Cin(this), cout_g(this), K], flipped in k.
            const int gco = co / p.cout_g, cig = ((co / p.MT) * p.MT / p.cout_g) * p.cin_g + ci;
            if (co < p.Cout && ci < p.cin_tile && cig / p.cin_g == gco)
                v = p.flipT ? p.w[((size_t)cig * p.cout_g + (co - gco * p.cout_g)) * p.K + (p.K - 1 - kk)]
                            : p.w[((size_t)co * p.cin_g + (cig - gco * p.cin_g)) * p.K + kk];
        } else if (ok) {
            if (p.flipT)
                v = p.w[((size_t)ci * p.Cout + co) * p.K + (p.K - 1 - kk)];
            else
                v = p.transposed ? p.w[((size_t)ci * p.Cout + co) * p.K + kk] : p.w[((size_t)co * p.Cin + ci) * p.K + kk];
        }
        p.out[i] = v;
    }
}
}  // namespace ttsc

static int set_weight_device_impl(ttsc_conv1d* c, const float* w_dev, const float* bias_dev, int flipT, void* stream);

extern "C" int ttsc_conv1d_set_weight_device(ttsc_conv1d* c, const float* w_dev, const float* bias_dev, void* stream) {
    return set_weight_device_impl(c, w_dev, bias_dev, 0, stream);
}

extern "C" int ttsc_conv1d_set_weight_device_dgrad(ttsc_conv1d* c, const float* fwd_weight_dev, void* stream) {
    TTSC_REQUIRE(c && !c->cfg.transposed, "ttsc_conv1d_set_weight_device_dgrad: the data-gradient handle must be a Conv1d");
    return set_weight_device_impl(c, fwd_weight_dev, nullptr, 1, stream);
}

static int set_weight_device_impl(ttsc_conv1d* c, const float* w_dev, const float* bias_dev, int flipT, void* stream) {
    TTSC_REQUIRE(c && w_dev, "ttsc_conv1d_set_weight_device: null argument");
    TTSC_REQUIRE(c->precision == TTSC_PREC_FP32, "ttsc_conv1d_set_weight_device: only TTSC_PREC_FP32 handles take device weights");
    const auto& g = c->cfg;
    if (c->phases.empty() || (bias_dev != nullptr) != (c->bias_dev != nullptr)) {
        // first call: lay out the phase buffers (zero weights), later calls only overwrite them
        c->w_host.assign((size_t)c->cin_g * g.out_channels * g.kernel_size, 0.f);   // (cin_g == in_channels unless grouped)
        c->has_bias = bias_dev != nullptr;
        c->b_host.assign(g.out_channels, 0.f);
        int rc = conv_repack(c);
        if (rc) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    for (auto& ph : c->phases) {
        PackArgs p;
        p.w = w_dev;
        p.out = ph.wp_dev;
        p.Cin = g.in_channels;
        p.Cout = g.out_channels;
        p.K = g.kernel_size;
        p.CoutV = c->CoutV;
        p.cipN = c->CinP / 2;
        p.cotN = c->CoutP / 32;
        p.ntaps = ph.ntaps;
        p.k0 = ph.taps.empty() ? 0 : ph.taps[0];
        p.kstep = ph.taps.size() > 1 ? ph.taps[1] - ph.taps[0] : 1;
        p.transposed = g.transposed;
        p.vfused = c->vfused ? 1 : 0;
        p.stride = g.stride;
        p.flipT = flipT;
        p.groups = c->groups;
        p.cin_g = c->cin_g;
        p.cout_g = c->cout_g;
        p.cin_tile = c->cin_tile;
        p.MT = c->MT;
        const long total = (long)p.ntaps * p.cipN * p.cotN * 64;
        const int blocks = (int)std::min<long>((total + 255) / 256, 2048);
        hipLaunchKernelGGL(pack_w_kernel, dim3(blocks), dim3(256), 0, s, p);
    }
    c->bias_ext = bias_dev;   // read straight from the caller's tensor by the launches that follow (no copy)
    c->w_plain_ext = flipT ? nullptr : w_dev;   // torch layout, used as is by the single-output-channel kernel
    if (int rc = launch_checked("pack_w_kernel")) return rc;
    c->dev_weights = true;
    return TTSC_OK;
}

static int conv_repack(ttsc_conv1d* c) {
    const float* w = c->w_host.data();
    const float* bias = c->has_bias ? c->b_host.data() : nullptr;
    TTSC_REQUIRE(c && w, "ttsc_conv1d_set_weight: null argument");
    const auto& g = c->cfg;
    free_phases(c);
    std::vector<float> packed;
    std::vector<_Float16> packed_h;
    // power-of-two weight scale for the split path: max|w| * 2^s in [512, 1024) keeps the low halves normal in fp16
    float wscale = 1.f;
    if (c->precision == TTSC_PREC_F16X3) {
        float mx = 0.f;
        for (float v : c->w_host) mx = fmaxf(mx, fabsf(v));
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) {
            (void)frexpf(mx, &e);   // mx = m * 2^e, m in [0.5, 1)
            e = 10 - e;             // mx * 2^e in [512, 1024)
            if (e > 24) e = 24;
            if (e < -8) e = -8;
        }
        wscale = ldexpf(1.f, e);
        c->w_unscale = ldexpf(1.f, -e);
    }
    // the phases are a function of the configuration (conv_plan.hpp); here they get their packed weights
    const std::vector<ConvPhaseGeom> geom = conv_phases(g, c->vfused);
    if (g.transposed) {   // (phase by phase: some phase would have no tap)
        TTSC_REQUIRE(g.kernel_size >= g.stride, "ConvTranspose1d with kernel_size < stride is not supported");
    }
    for (const ConvPhaseGeom& pg : geom) {
        ConvPhase ph;
        static_cast<ConvPhaseGeom&>(ph) = pg;
        if (c->precision == TTSC_PREC_F16X3) {
            pack_phase_f16(c, w, ph.taps, wscale, packed_h);
            TTSC_HIP_CHECK(hipMalloc((void**)&ph.wph_dev, packed_h.size() * sizeof(_Float16)));
            TTSC_HIP_CHECK(hipMemcpy(ph.wph_dev, packed_h.data(), packed_h.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        } else {
            pack_phase(c, w, ph.taps, packed);
            TTSC_HIP_CHECK(hipMalloc((void**)&ph.wp_dev, packed.size() * sizeof(float)));
            TTSC_HIP_CHECK(hipMemcpy(ph.wp_dev, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        c->phases.push_back(ph);
    }
    if (c->bias_dev) {
        (void)hipFree(c->bias_dev);
        c->bias_dev = nullptr;
    }
    if (bias) {
        TTSC_HIP_CHECK(hipMalloc((void**)&c->bias_dev, g.out_channels * sizeof(float)));
        TTSC_HIP_CHECK(hipMemcpy(c->bias_dev, bias, g.out_channels * sizeof(float), hipMemcpyHostToDevice));
    }
    if (c->w_plain_dev) {
        (void)hipFree(c->w_plain_dev);
        c->w_plain_dev = nullptr;
    }
    if (conv_wants_plain(g)) {   // conv_cout1_kernel reads the weights in torch layout [1][Cin][K]
        TTSC_HIP_CHECK(hipMalloc((void**)&c->w_plain_dev, c->w_host.size() * sizeof(float)));
        TTSC_HIP_CHECK(hipMemcpy(c->w_plain_dev, c->w_host.data(), c->w_host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    c->w_plain_ext = nullptr;
    c->has_weight = true;
    return TTSC_OK;
}

extern "C" int ttsc_conv1d_forward(const ttsc_conv1d* c, const float* x, int32_t B, int64_t Lin, float* y,
                                   const float* resid, const ttsc_conv1d_epilogue* ep, void* stream) {
    return ttsc_conv1d_forward_ragged(c, x, B, Lin, y, resid, ep, nullptr, nullptr, stream);
}

extern "C" int32_t ttsc_conv1d_in_channels(const ttsc_conv1d* c) { return c ? c->cfg.in_channels : 0; }

// Split precision carries an fp32 value as two fp16 halves, so an activation tensor must sit inside fp16's range: with |x|
// below ~2^-3 the low half goes subnormal (the accuracy degrades towards fp16's), above 65504 the high half overflows.  The
// layer's input is therefore multiplied by a power of two while it is staged (exact) and the accumulated result by its
// inverse in the epilogue (exact; leaky-relu is positively homogeneous).  scale = 1 restores the plain behaviour.
extern "C" int ttsc_conv1d_set_activation_scale(ttsc_conv1d* c, float scale) {
    TTSC_REQUIRE(c, "ttsc_conv1d_set_activation_scale: null argument");
    int e = 0;
    TTSC_REQUIRE(scale > 0.f && std::isfinite(scale) && frexpf(scale, &e) == 0.5f, "ttsc_conv1d_set_activation_scale: scale must be a power of two, got %g", scale);
    c->act_scale = scale;
    return TTSC_OK;
}
extern "C" float ttsc_conv1d_get_activation_scale(const ttsc_conv1d* c) { return c ? c->act_scale : 0.f; }

extern "C" int ttsc_conv1d_set_nonfinite_flag(ttsc_conv1d* c, uint32_t* flag_dev) {
    TTSC_REQUIRE(c, "ttsc_conv1d_set_nonfinite_flag: null argument");
    c->nf_flag = flag_dev;
    return TTSC_OK;
}

namespace ttsc {
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
    __shared__ float red[4];
    float m = 0.f;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {   // 16-byte loads over the aligned body, the tail element-wise
        const long n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        for (long i = i0; i < n4; i += stride) {
            const float4 v = x4[i];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
        for (long i = (n4 << 2) + i0; i < n; i += stride) m = fmaxf(m, fabsf(x[i]));
    } else {
        for (long i = i0; i < n; i += stride) m = fmaxf(m, fabsf(x[i]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    // ONE atomic per workgroup (the first version sent one per wave from up to 4096 workgroups to the same word: 0.19 ms for a 16 MB tensor)
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));   // non-negative floats order like their bit patterns
}
}  // namespace ttsc

// out_dev (one float, device) = max(out_dev, max_i |x_i|); the caller zeroes it first.  Non-finite inputs end up as a NaN/inf
// bit pattern, which compares above every finite value: the caller sees it.
extern "C" int ttsc_absmax(const float* x_dev, int64_t n, float* out_dev, void* stream) {
    TTSC_REQUIRE(x_dev && out_dev && n > 0, "ttsc_absmax: bad argument");
    const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256 + 1, 1024);
    hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x_dev, (long)n, reinterpret_cast<unsigned*>(out_dev));
    return launch_checked("absmax_kernel");
}

// the plan's LDS size of the wide and tall kernels is the pipeline's
static_assert(WidePipe<256, 11, 5, true>::LDS_BYTES == conv_pipe_lds(256 + 10 * 5, 2) && TallPipe<512, 4, 4, 2, true>::LDS_BYTES == conv_pipe_lds(128 + 3, 4) &&
              TallPipe<256, 6, 2, 4, false>::LDS_BYTES == conv_pipe_lds(256 + 5, 2), "conv_plan.hpp: conv_pipe_lds");

// conv_plan's view of a handle and of a call.  Without weights the plain-layout copy counts as present when set_weight would create it.
static ConvLayer conv_layer_of(const ttsc_conv1d* c) {
    const bool has_plain = c->has_weight ? (c->dev_weights ? c->w_plain_ext : c->w_plain_dev) != nullptr : conv_wants_plain(c->cfg);
    return ConvLayer{c->cfg, c->MT, c->NT, c->CinP, c->CoutP, c->groups, c->precision, c->vfused, c->vrow4, has_plain, c->act_scale};
}
static ConvLaunch conv_launch_of(int B, int64_t Lin, int64_t Lout, const ttsc_conv1d_epilogue* ep) {
    return ConvLaunch{B, Lin, Lout, ep && ep->gate_dev, ep ? ep->out_act : TTSC_ACT_NONE, ep ? ep->out_scale : 1.f, ep ? ep->in_scale : 1.f};
}

extern "C" int ttsc_conv1d_forward_ragged(const ttsc_conv1d* c, const float* x, int32_t B, int64_t Lin, float* y,
                                          const float* resid, const ttsc_conv1d_epilogue* ep, const int32_t* in_len_dev,
                                          const int32_t* out_len_dev, void* stream) {
    return ttsc_conv1d_forward_pitched(c, x, B, Lin, y, resid, ep, in_len_dev, out_len_dev, 0, stream);
}

extern "C" int ttsc_conv1d_forward_pitched(const ttsc_conv1d* c, const float* x, int32_t B, int64_t Lin, float* y,
                                           const float* resid, const ttsc_conv1d_epilogue* ep, const int32_t* in_len_dev,
                                           const int32_t* out_len_dev, int64_t Lout_pitch, void* stream) {
    TTSC_REQUIRE(c && x && y, "ttsc_conv1d_forward: null argument");
    TTSC_REQUIRE(Lout_pitch == 0 || (Lout_pitch > 0 && in_len_dev && out_len_dev),
                 "ttsc_conv1d_forward_pitched: an output pitch needs per-utterance lengths (in_len_dev, out_len_dev)");
    if (!c->has_weight) {
        set_error("ttsc_conv1d_forward: weights not set");
        return TTSC_ESTATE;
    }
    TTSC_REQUIRE(B > 0 && Lin > 0, "ttsc_conv1d_forward: bad B/Lin (%d, %lld)", B, (long long)Lin);
    TTSC_REQUIRE(!ep || (ep->in_slope >= 0.f && ep->in_slope <= 1.f), "ttsc_conv1d_forward: in_slope must be in [0,1]");
    const auto& g = c->cfg;
    // (with a pitch, positions between an utterance's real length and the pitch are computed from zero-padded input and land in the row's padding)
    const int64_t Lout = Lout_pitch > 0 ? Lout_pitch : ttsc_conv1d_out_len(c, Lin);
    TTSC_REQUIRE(Lout > 0, "ttsc_conv1d_forward: output length %lld <= 0", (long long)Lout);
    TTSC_REQUIRE(Lin < (1ll << 30) && Lout < (1ll << 30), "ttsc_conv1d_forward: length too large");
    hipStream_t s = (hipStream_t)stream;
    const ConvSwitches sw = conv_switches();
    const ConvLayer layer = conv_layer_of(c);
    const ConvLaunch launch = conv_launch_of(B, Lin, Lout, ep);
    for (const auto& ph : c->phases) {
        // 1. what does not depend on the plan
        ConvArgs a;
        a.x = x;
        a.y = y;
        a.resid = resid;
        a.nf_flag = nullptr;
        a.wp = ph.wp_dev;
        a.wph = ph.wph_dev;
        a.w_unscale = c->w_unscale;
        a.bias = (c->dev_weights && c->bias_ext) ? c->bias_ext : c->bias_dev;
        a.in_len = in_len_dev;
        a.out_len = out_len_dev;
        a.dbg = 0;
        a.fold_S = 0;
        a.amax_x = a.amax_w = nullptr;
        a.amax_out = nullptr;
#ifdef TTSC_ABLATE
        if (const char* ev = getenv("TTSC_CONV_DBG")) a.dbg = atoi(ev);
        a.prof = nullptr;
        if (const char* ev = getenv("TTSC_PROF_PTR")) a.prof = reinterpret_cast<unsigned long long*>(strtoull(ev, nullptr, 0));
#endif
        a.vphase = c->vfused ? (c->vrow4 ? -4 : g.out_channels) : 0;
        if (a.vphase == -4) {
            TTSC_REQUIRE(!(ep && ep->gate_dev), "ttsc_conv1d_forward: the gate epilogue is not available on this transposed layer");
            TTSC_REQUIRE(((uintptr_t)y % 16 == 0) && (!resid || (uintptr_t)resid % 16 == 0), "ttsc_conv1d_forward: y / resid must be 16-byte aligned for ConvTranspose1d(k=4, s=4)");
        }
        a.Cin = c->groups > 1 ? c->cin_tile : g.in_channels;
        a.CinTot = g.in_channels;
        a.groups = c->groups;
        a.cin_g = c->cin_g;
        a.cout_g = c->cout_g;
        a.CinP = c->CinP;
        a.Cout = g.out_channels;
        a.CoutP = c->CoutP;
        a.Lin = (int)Lin;
        a.Lout = (int)Lout;
        a.ntaps = ph.ntaps;
        a.tap_base = ph.tap_base;
        a.tap_step = ph.tap_step;
        a.out_stride = ph.out_stride;
        a.out_off = ph.out_off;
        a.in_scale = launch.in_scale;
        a.in_slope = ep ? ep->in_slope : 1.f;
        a.out_scale = launch.out_scale;
        a.out_act = launch.out_act;
        a.accumulate = ep ? ep->accumulate : 0;
        a.gate = ep ? ep->gate_dev : nullptr;
        a.gate_slope = ep ? ep->gate_slope : 1.f;
        // 2. kernel family, tile and what follows from them
        ConvPlan p;
        if (!conv_plan(layer, ph, launch, sw, p)) {
            set_error("%s", p.error);
            return TTSC_EINVAL;
        }
        if (p.family == TTSC_CONV_PATH_NONE) continue;
        // 3. the plan's part of the arguments
        a.q_lo = p.q_lo;
        a.q_cnt = p.q_cnt;
        a.min_shift = p.min_shift;
        a.span = p.span;
        a.span_pad = p.span_pad;
        a.acc_init = p.acc_init;
        a.epi_prefetch = p.epi_prefetch;
        a.swz_nx = p.swz_nx;
        a.swz_ny = p.swz_ny;
        a.fold_B = p.fold_B;
        a.lean = p.lean;
        a.short_from = p.short_from;
        if (c->precision == TTSC_PREC_F16X3 && p.family != TTSC_CONV_PATH_COUT1) {   // activation pre-scale (exact powers of two, see ttsc_conv1d_set_activation_scale)
            a.in_scale *= c->act_scale;
            a.w_unscale = c->w_unscale / c->act_scale;
        }
        // 4. the instantiation the plan names
        int rc = TTSC_EINVAL;
        switch (p.family) {
            case TTSC_CONV_PATH_COUT1:
                a.wp = c->dev_weights ? c->w_plain_ext : c->w_plain_dev;
                a.nf_flag = c->nf_flag;
                hipLaunchKernelGGL(conv_cout1_kernel, dim3(p.grid[0], p.grid[1]), dim3(256), 0, s, a);
                rc = launch_checked("conv_cout1_kernel");
                break;
            case TTSC_CONV_PATH_TALL:
                rc = p.inst == 0 ? launch_f16_tall<512, 4, 4, 2>(a, B, s) : launch_f16_tall<256, 6, 2, 4>(a, B, s);
                break;
            case TTSC_CONV_PATH_WIDE:
                rc = g.out_channels == 256 ? launch_f16_wide_k<256>(a, B, g.dilation, s) : launch_f16_wide_k<128>(a, B, g.dilation, s);
                break;
            case TTSC_CONV_PATH_F16X3:
                switch (p.inst) {
                    case F16_2x2: rc = launch_f16<2, 2>(a, B, s); break;
                    case F16_2x1: rc = launch_f16<2, 1>(a, B, s); break;
                    case F16_1x4: rc = launch_f16<1, 4>(a, B, s); break;
                    case F16_1x2: rc = launch_f16<1, 2>(a, B, s); break;
                    case F16_1x1: rc = launch_f16<1, 1>(a, B, s); break;
                }
                break;
            case TTSC_CONV_PATH_FP32:
                switch (p.inst) {
                    case CFG_2222: rc = launch_cfg<2, 2, 2, 2>(a, B, s); break;
                    case CFG_1222: rc = launch_cfg<1, 2, 2, 2>(a, B, s); break;
                    case CFG_1122: rc = launch_cfg<1, 1, 2, 2>(a, B, s); break;
                    case CFG_2214: rc = launch_cfg<2, 2, 1, 4>(a, B, s); break;
                    case CFG_1414: rc = launch_cfg<1, 4, 1, 4>(a, B, s); break;
                    case CFG_1214: rc = launch_cfg<1, 2, 1, 4>(a, B, s); break;
                    case CFG_1114: rc = launch_cfg<1, 1, 1, 4>(a, B, s); break;
                }
                break;
        }
        if (rc) return rc;
    }
    return TTSC_OK;
}

// Which kernel the launcher above takes, without launching: the same conv_switches(), the same conv_plan() — the query cannot drift from the
// launcher.  No HIP call; a handle without weights plans the phases (and the plain-layout copy) ttsc_conv1d_set_weight would create.
extern "C" int32_t ttsc_conv1d_plan(const ttsc_conv1d* c, int32_t B, int64_t Lin, const ttsc_conv1d_epilogue* ep, int32_t phase, int32_t* info) {
    TTSC_REQUIRE(c && info, "ttsc_conv1d_plan: null argument");
    TTSC_REQUIRE(B > 0 && Lin > 0, "ttsc_conv1d_forward: bad B/Lin (%d, %lld)", B, (long long)Lin);
    const int64_t Lout = ttsc_conv1d_out_len(c, Lin);
    TTSC_REQUIRE(Lout > 0, "ttsc_conv1d_forward: output length %lld <= 0", (long long)Lout);
    TTSC_REQUIRE(Lin < (1ll << 30) && Lout < (1ll << 30), "ttsc_conv1d_forward: length too large");
    const std::vector<ConvPhaseGeom> geom = conv_phases(c->cfg, c->vfused);   // (what set_weight uploads, or will)
    TTSC_REQUIRE(phase >= 0 && phase < (int)geom.size(), "ttsc_conv1d_plan: the layer has %d phase(s), asked for phase %d", (int)geom.size(), phase);
    ConvPlan p;
    if (!conv_plan(conv_layer_of(c), geom[phase], conv_launch_of(B, Lin, Lout, ep), conv_switches(), p)) {
        set_error("%s", p.error);
        return TTSC_EINVAL;
    }
    const int32_t out[10] = {p.rows, p.cols, p.tap_bucket, (int32_t)p.grid[0], (int32_t)p.grid[1], (int32_t)p.grid[2], (int32_t)p.lds, p.lean, p.acc_init, p.short_from};
    std::copy(out, out + 10, info);
    return p.family;
}

// Fused  y = x + conv2(lrelu(conv1(lrelu(x))))  for 32-channel ResBlock1 pairs (see respair32_f16x3_kernel).
extern "C" int ttsc_respair_supported(const ttsc_conv1d* c1, const ttsc_conv1d* c2) {
    if (!c1 || !c2) return 0;
    const auto &g1 = c1->cfg, &g2 = c2->cfg;
    const int k = g1.kernel_size;
    if (g1.transposed || g2.transposed) return 0;
    if (g1.in_channels != 32 || g1.out_channels != 32 || g2.in_channels != 32 || g2.out_channels != 32) return 0;
    if (g2.kernel_size != k || !(k == 3 || k == 7 || k == 11)) return 0;
    if (g2.dilation != 1 || g2.padding != (k - 1) / 2 || g1.padding != g1.dilation * (k - 1) / 2) return 0;
    if ((k - 1) * g1.dilation > 64) return 0;
    if (c1->precision != TTSC_PREC_F16X3 || c2->precision != TTSC_PREC_F16X3) return 0;
    if (!c1->has_weight || !c2->has_weight || !c1->bias_dev || !c2->bias_dev) return 0;
    return 1;
}

extern "C" int ttsc_respair_forward(const ttsc_conv1d* c1, const ttsc_conv1d* c2, const float* x, int32_t B, int64_t L, float* y,
                                    int32_t accumulate, const int32_t* len_dev, void* stream) {
    TTSC_REQUIRE(c1 && c2 && x && y, "ttsc_respair_forward: null argument");
    TTSC_REQUIRE(ttsc_respair_supported(c1, c2), "ttsc_respair_forward: this pair of layers is not eligible for the fused kernel");
    TTSC_REQUIRE(x != y, "ttsc_respair_forward: y must not alias x");
    TTSC_REQUIRE(B > 0 && L > 0 && L < (1ll << 30), "ttsc_respair_forward: bad B/L");
    PairArgs a;
    a.x = x;
    a.y = y;
    a.w1 = c1->phases[0].wph_dev;
    a.w2 = c2->phases[0].wph_dev;
    a.b1 = c1->bias_dev;
    a.b2 = c2->bias_dev;
    a.len = len_dev;
    a.unscale1 = c1->w_unscale;
    a.unscale2 = c2->w_unscale;
    a.L = (int)L;
    a.d1 = c1->cfg.dilation;
    a.accumulate = accumulate;
    const int k = c1->cfg.kernel_size;
    // 4 waves / 256 columns (224 outputs) per workgroup: two workgroups share a CU and hide each other's load latency
    constexpr int NW = 4, NCOL = 64 * NW, NTO = NCOL - 32;
    const int span1 = NCOL + (k - 1) * a.d1;
    const size_t lds = (size_t)span1 * 16 * 2 * 2 + (size_t)(NCOL + 16) * 32 * 2 * 2;
    dim3 grid((unsigned)ceil_div(L, NTO), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_full_lds((const void*)respair32_f16x3_kernel<3, NW>)) return rc;
    if (int rc = ensure_full_lds((const void*)respair32_f16x3_kernel<7, NW>)) return rc;
    if (int rc = ensure_full_lds((const void*)respair32_f16x3_kernel<11, NW>)) return rc;
    if (k == 3)
        hipLaunchKernelGGL((respair32_f16x3_kernel<3, NW>), grid, dim3(64 * NW), lds, s, a);
    else if (k == 7)
        hipLaunchKernelGGL((respair32_f16x3_kernel<7, NW>), grid, dim3(64 * NW), lds, s, a);
    else
        hipLaunchKernelGGL((respair32_f16x3_kernel<11, NW>), grid, dim3(64 * NW), lds, s, a);
    return launch_checked("respair32_f16x3_kernel");
}
