// Device code shared by the convolution translation units (conv1d.hip: inference and exact-fp32 training launches; conv_train.hip:
// split-precision training launches): launch arguments, the fused epilogues, the exact-fp32 implicit-GEMM kernel and the general
// split-precision kernel.  The wide / tall split-precision kernels live in conv_f16x3_widetall.hpp, the pieces all three share in
// conv_f16x3_tile.hpp.
#pragma once
#include "common.hpp"
#include "conv_f16x3_tile.hpp"
#include "conv_internal.hpp"

namespace ttsc {

// Ablation switches exist only in the measurement build (-DTTSC_ABLATE, tools/ablate.cpp); the product library compiles
// them to constants, so no environment variable can make a shipped kernel skip work.
#ifdef TTSC_ABLATE
#define TTSC_DBG(args, bit) (((args).dbg & (bit)) != 0)
// phase timeline of a workgroup (tools/wg_timeline.py): thread 0 writes the 100 MHz wall clock into slot `i` of its workgroup's 24-slot record
#define TTSC_STAMP(args, wg, i)                                                                              \
    do {                                                                                                     \
        if ((args).prof && threadIdx.x == 0) (args).prof[(size_t)(wg) * 24 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define TTSC_STAMP_HWID(args, wg, i)                                                                         \
    do {                                                                                                     \
        if ((args).prof && threadIdx.x == 0) {                                                               \
            unsigned hw, xcc;                                                                                \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                 \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                               \
            (args).prof[(size_t)(wg) * 24 + (i)] = ((unsigned long long)(xcc & 0xf) << 32) | hw;            \
        }                                                                                                    \
    } while (0)
#else
#define TTSC_DBG(args, bit) false
#define TTSC_STAMP(args, wg, i) do {} while (0)
#define TTSC_STAMP_HWID(args, wg, i) do {} while (0)
#endif

static constexpr int KC = 16;  // input channels staged per LDS chunk

struct ConvArgs {
    const float* x;
    float* y;
    const float* resid;
    const float* wp;    // fp32 path: [ntaps][CinP/2][CoutP/32][64]
    const void* wph;    // f16x3 path: [ntaps][CinP/16][CoutP/32][2 (hi,lo)][64 lanes][8 half]
    float w_unscale;    // f16x3 path: weights are stored multiplied by 2^s; the epilogue multiplies by 2^-s
    const float* bias;  // [Cout] or null
    const int* in_len;  // [B] per-utterance valid input length (ragged batches) or null
    const int* out_len; // [B] per-utterance valid output length or null (tiles wholly beyond it are skipped)
    int Cin, CinP, Cout, CoutP;   // Cin = input channels a workgroup stages (grouped: those of its rows' groups), CinP = rounded up to 16
    int CinTot;                   // channels of the input tensor (batch stride); == Cin unless grouped
    int groups, cin_g, cout_g;    // grouped Conv1d (fp32 kernel only): the workgroup's first input channel = (its first row / cout_g) * cin_g
    int Lin, Lout;
    int ntaps, tap_base, tap_step;
    int out_stride, out_off;
    int q_lo, q_cnt;
    int span, span_pad, min_shift;
    float in_scale, in_slope, out_scale;
    int out_act, accumulate;
    int vphase;       // fused ConvTranspose1d phases: GEMM row v = r * vphase + co (vphase = real Cout), output o += r; 0 = off;
                      // -4 = rows interleaved v = co * 4 + r (kernel_size == stride == 4): see epilogue_tile_v4
    int acc_init;     // wide kernel: bias, residual and running sum enter the sum as the INITIAL value of the accumulators (loaded in the prologue,
                      // all at once) instead of in the epilogue; requires out_scale == 1, no activation, no gate (set by launch_f16_wide)
    int epi_prefetch; // wide kernel: residual / running-sum operands of the epilogue fetched several tiles ahead (same arithmetic as epilogue_tile)
    int swz_nx, swz_ny;   // tall kernel, XCD-aware 1-D launch (swz_nx > 0): workgroup id -> (q tile, row tile, utterance) such that the row tiles (= the
                          // phases of a transposed convolution) of one q tile run on ONE XCD, back to back: see conv_f16x3_tall_kernel
    int lean;         // wide / tall kernels: launch the LEAN instantiation (staging loads through a buffer descriptor, zero taps skipped); decided per
                      // launch by the host (TTSC_CONV_LEAN, Cin * Lin * 4 < 2^31, finite positive in_scale), 0 = the kernels as they were
    int short_from;   // tall kernel, lean launches: row tiles (= phases of the transposed convolution) at or beyond this index lack the last of the
                      // `ntaps` taps (kernel tap r + (ntaps-1)*stride >= kernel_size: the packers store zero weights there) and skip it.  Computed by
                      // the host from kernel_size, stride and the row-tile height, never from weights; INT_MAX when a row tile spans several phases
    int dbg;          // ablation switches, ONLY in -DTTSC_ABLATE builds (tools/ablate.cpp; never in libttscube_hip.so): see TTSC_DBG
#ifdef TTSC_ABLATE
    unsigned long long* prof;   // workgroup phase timeline (TTSC_STAMP) or null; env TTSC_PROF_PTR
#endif
    unsigned* nf_flag;  // conv_cout1_kernel: set to 1 when a non-finite output sample is produced (split-precision range guard), or null
    const float* gate;  // data-gradient launches: [B,Cout,Lout] pre-activation saved by the forward; the conv result is
    float gate_slope;   // multiplied by d lrelu/dx = (gate > 0 ? 1 : gate_slope) BEFORE the residual is added; null = off
    // split-precision TRAINING launches (conv_train.hip, conv_f16x3_kernel<.., FOLD = true>):
    //   * the batch is folded into the GEMM's column dimension: column v of the launch is position v % fold_S of sequence v / fold_S,
    //     fold_S >= Lin + padding so that a tap that leaves a sequence lands in the (zero) gap before the next one — training crops and
    //     the deep discriminator layers are 50 .. 1 200 positions long, far below a useful tile width;
    //   * both power-of-two scales are derived IN the kernel from device-side maxima (*amax_x = max |x|, *amax_w = max |w|, written by
    //     the launches before this one): activations and gradients move every step, no host round trip decides their range.
    int fold_S, fold_B;
    const float* amax_x;
    const float* amax_w;
    //   * `amax_out` (or null): the launch ALSO leaves max |y| over the elements it stores in this word (atomic max on the bit pattern; the word is
    //     zero before the launch) — the next launch that reads y (the following layer's forward, the preceding layer's data gradient, the weight
    //     gradient) takes its range from it instead of running a reduction launch over y (round 6: 445 amax2_kernel launches per Cubegan step).
    unsigned* amax_out;
};

// power of two that moves a magnitude m = f * 2^e (f in [0.5, 1)) to [2^(target-1), 2^target); 1 for zero, subnormal and non-finite m
// (a non-finite tensor then reaches the output as NaN / inf instead of being hidden)
__device__ __forceinline__ float pow2_to(float m, int target) {
    const int ex = (int)((__float_as_uint(m) >> 23) & 0xffu);
    if (ex == 0 || ex == 255) return 1.f;
    int s = target - (ex - 126);
    s = s > 100 ? 100 : (s < -100 ? -100 : s);
    return __uint_as_float((unsigned)(127 + s) << 23);
}
// conv_train.hip: *out_x = max |x|, *out_w = max |w| in one launch; a null tensor is skipped (its word was measured by an earlier launch of the layer)
int launch_amax2(const float* x, long nx, float* out_x, const float* w, long nw, float* out_w, hipStream_t s, bool prezeroed = false);
static constexpr int SPLIT_X_TARGET = 15, SPLIT_W_TARGET = 10;   // |x| < 2^15 (fp16 max 65504), |w| < 2^10 (as the host-side packing)

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == TTSC_ACT_TANH) return tanhf(v);
    if (act == TTSC_ACT_RELU) return fmaxf(v, 0.f);
    if (act == TTSC_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
    return v;
}

// Epilogue of one 32x32 MFMA tile held by a wave: bias + residual + scale + activation (+ running sum) and store.
// All residual / running-sum loads of the tile are issued BEFORE the first store: `resid` and `y` may alias
// (in-place residual stream), which otherwise forces the compiler to order every load behind the previous store and
// serialises 16 dependent round trips per tile.  Each lane only reads the addresses it writes, so this is safe.
// C/D layout of v_mfma_*_32x32: column (time) = lane & 31, row (channel) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
__device__ __forceinline__ void epilogue_tile(const f32x16& acc, const ConvArgs& a, int b, int co_base, long o, bool qok,
                                              int half, float acc_scale, float* amax_acc = nullptr) {
    // NOTE: the optional operands are tested once per row group (wave-uniform branches around straight-line load
    // groups).  A per-element `ptr ? ptr[i] : 0` makes hipcc branch around every single load and wait for each one in turn.
    // The tile is processed as four groups of four rows (= the four 8-channel items a lane contributes to): all loads
    // of a group are issued before its stores, and only ~4 values per operand are live at a time (register pressure).
    const long o_c = qok ? o : 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float rv[4], yv[4], bv[4], res[4];
        size_t idx[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co_base + 8 * g + 4 * half + e;
            const int co_c = co < a.Cout ? co : a.Cout - 1;
            idx[e] = ((size_t)b * a.Cout + co_c) * a.Lout + o_c;
        }
        if (a.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co_base + 8 * g + 4 * half + e;
                bv[e] = a.bias[co < a.Cout ? co : a.Cout - 1];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = 0.f;
        }
        if (a.resid) {
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[e] = a.resid[idx[e]];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) rv[e] = 0.f;
        }
        if (a.accumulate) {
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[e] = a.y[idx[e]];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[e] = 0.f;
        }
        if (a.gate) {   // backward of the fused leaky-relu prologue (training only)
            float gv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = a.gate[idx[e]];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                res[e] = ((acc[4 * g + e] * acc_scale + bv[e]) * (gv[e] > 0.f ? 1.f : a.gate_slope) + rv[e]) * a.out_scale + yv[e];
        } else if (a.out_act == TTSC_ACT_NONE) {   // the common case gets its own straight-line copy (no inlined tanh/exp bodies)
#pragma unroll
            for (int e = 0; e < 4; ++e) res[e] = (acc[4 * g + e] * acc_scale + bv[e] + rv[e]) * a.out_scale + yv[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) res[e] = apply_act((acc[4 * g + e] * acc_scale + bv[e] + rv[e]) * a.out_scale, a.out_act) + yv[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co_base + 8 * g + 4 * half + e;
            if (qok && co < a.Cout) {
                a.y[idx[e]] = res[e];
                if (amax_acc) *amax_acc = fmaxf(*amax_acc, fabsf(res[e]));   // (fmaxf drops NaN, as amax2_kernel does)
            }
        }
    }
}

// Epilogue of a 32x32 tile of a ConvTranspose1d with kernel_size == stride == 4 whose GEMM rows are interleaved as
// v = co * 4 + r (phase r of output channel co): the four consecutive accumulator registers of a lane are the four phases of
// ONE output channel at ONE input position q, i.e. four CONSECUTIVE output samples o = 4q .. 4q+3 — one 16-byte store per
// lane, 512 contiguous bytes per half-wave.  (With rows ordered r * Cout + co every lane writes single floats at a 16-byte
// stride and the four phases arrive in four separate store instructions: 1.2 ms instead of ~0.4 ms for the last upsampler.)
__device__ __forceinline__ void epilogue_tile_v4(const f32x16& acc, const ConvArgs& a, int b, int row_base, int q, bool qok, int half,
                                                 float acc_scale) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = (row_base >> 2) + 2 * g + half;
        const bool ok = qok && co < a.Cout;
        const int co_c = co < a.Cout ? co : a.Cout - 1;
        const size_t idx = ((size_t)b * a.Cout + co_c) * a.Lout + (size_t)(ok ? q : 0) * 4;
        const float bv = a.bias ? a.bias[co_c] : 0.f;
        f32x4 rv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
        if (a.resid) rv = *reinterpret_cast<const f32x4*>(a.resid + idx);
        if (a.accumulate) yv = *reinterpret_cast<const f32x4*>(a.y + idx);
        f32x4 res;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = (acc[4 * g + e] * acc_scale + bv + rv[e]) * a.out_scale;
            res[e] = (a.out_act == TTSC_ACT_NONE ? t : apply_act(t, a.out_act)) + yv[e];
        }
        if (ok) *reinterpret_cast<f32x4*>(a.y + idx) = res;
    }
}

template <int MI, int NJ, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64, 2) void conv_mfma_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [2][KC][span_pad]  (double-buffered activation chunk)
    constexpr int NT = WN * NJ * 32;
    constexpr int NTHREADS = WM * WN * 64;
    constexpr int SPC = NT + 64;                                   // staged positions per channel covered by the register prefetch
    constexpr int NWAVES = WM * WN;
    constexpr int SMAIN = KC * NT / NTHREADS;                      // prefetch registers per thread: tile columns
    constexpr int SHALO = KC / NWAVES;                             //                                halo strip
    static_assert(KC * NT % NTHREADS == 0 && KC % NWAVES == 0, "staging split");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int b = blockIdx.z;
    const int q0 = a.q_lo + blockIdx.x * NT;
    const int lin = a.in_len ? a.in_len[b] : a.Lin;   // positions >= lin read as zero (== that utterance run alone)
    if (a.out_len && (long)q0 * a.out_stride + a.out_off >= a.out_len[b]) return;  // padding-only tile
    const int cot0 = (blockIdx.y * WM + wm) * MI;  // first 32-row tile of this wave
    const int cotN = a.CoutP >> 5;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // grouped convolution: this workgroup's rows only meet the input channels of their own group(s)
    const int cin0 = a.groups > 1 ? ((blockIdx.y * (WM * MI * 32)) / a.cout_g) * a.cin_g : 0;
    const float* xb = a.x + ((size_t)b * a.CinTot + cin0) * a.Lin;
    const int cin_n = a.groups > 1 ? min(a.Cin, a.CinTot - cin0) : a.Cin;   // (the last row tile of a grouped layer may hold fewer groups than a full one)
    const int lo = q0 + a.min_shift;  // x position of LDS column 0
    const int cipN = a.CinP >> 1;
    const int nchunks = a.CinP / KC;
    const int bufsz = KC * a.span_pad;
    const bool wide = a.span > SPC;   // receptive field beyond the prefetch window: extra columns are staged synchronously

    // ---- software pipeline -------------------------------------------------------------------------------------
    // Left to itself hipcc issues every global load right before its use and waits vmcnt(0) for it: one L2 round trip
    // per MFMA and per staged element, which only many resident workgroups can hide.  Training crops and short
    // utterances run at <= 1 workgroup per CU, so both operand streams are pipelined explicitly:
    //   * activations: chunk c+1 is fetched into registers (sreg) while chunk c is multiplied; LDS is double-buffered,
    //     one barrier per chunk;
    //   * weights: the 8*MI fragments of (chunk, tap) g+1 are in flight while (chunk, tap) g is multiplied (wa / wb).
    // The fmaf chain order (chunk, tap, channel pair) is unchanged, results stay bit-identical.
    // prefetch registers: the NT tile columns of the 16 channels (e = tid + i*NTHREADS -> channel e / NT, column e % NT,
    // powers of two) plus a 64-column halo strip (channel = wave + i*NWAVES, column = NT + lane)
    float sreg[SMAIN + SHALO];
    // sload only ISSUES the loads (clamped addresses); masking, scaling and the leaky-relu happen in scommit, so that no
    // use of a loaded value sits between the loads (hipcc would wait for each one in turn)
    auto sload = [&](int cc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SMAIN; ++i) {
            const int e = tid + i * NTHREADS;
            const int c = e / NT, p = e % NT;
            const int ci = min(cc + c, cin_n - 1), pos = min(max(lo + p, 0), a.Lin - 1);
            sreg[i] = xb[(unsigned)(ci * a.Lin + pos)];
        }
#pragma unroll
        for (int i = 0; i < SHALO; ++i) {
            const int c = wave + i * NWAVES, p = NT + lane;
            const int ci = min(cc + c, cin_n - 1), pos = min(max(lo + p, 0), a.Lin - 1);
            sreg[SMAIN + i] = xb[(unsigned)(ci * a.Lin + pos)];
        }
    };
    auto scommit = [&](float* buf, int cc) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < SMAIN; ++i) {
            const int e = tid + i * NTHREADS;
            const int c = e / NT, p = e % NT;
            const int ci = cc + c, pos = lo + p;
            float v = sreg[i] * a.in_scale;
            v = v > 0.f ? v : v * a.in_slope;
            if (p < a.span) buf[c * a.span_pad + p] = (ci < cin_n && pos >= 0 && pos < lin) ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < SHALO; ++i) {
            const int c = wave + i * NWAVES, p = NT + lane;
            const int ci = cc + c, pos = lo + p;
            float v = sreg[SMAIN + i] * a.in_scale;
            v = v > 0.f ? v : v * a.in_slope;
            if (p < a.span) buf[c * a.span_pad + p] = (ci < cin_n && pos >= 0 && pos < lin) ? v : 0.f;
        }
        if (wide) {
            for (int c = wave; c < KC; c += NWAVES) {
                const int ci = cc + c;
                for (int p = SPC + lane; p < a.span; p += 64) {
                    const int pos = lo + p;
                    float v = 0.f;
                    if (ci < cin_n && pos >= 0 && pos < lin) {
                        v = xb[(size_t)ci * a.Lin + pos] * a.in_scale;
                        v = v > 0.f ? v : v * a.in_slope;
                    }
                    buf[c * a.span_pad + p] = v;
                }
            }
        }
    };
    auto loadA = [&](float (&w)[KC / 2][MI], int ch, int j) __attribute__((always_inline)) {
        const float* wj = a.wp + ((size_t)(j * cipN + ch * (KC / 2)) * cotN + cot0) * 64 + lane;
#pragma unroll
        for (int cp = 0; cp < KC / 2; ++cp)
#pragma unroll
            for (int i = 0; i < MI; ++i) w[cp][i] = wj[((size_t)cp * cotN + i) * 64];
    };
    int chC = 0, jC = 0;   // compute cursor
    auto step = [&](const float (&w)[KC / 2][MI]) __attribute__((always_inline)) {
        if (jC == 0 && chC > 0) {   // chunk switch: publish the prefetched activations, fetch the chunk after
            scommit(xs + (chC & 1) * bufsz, chC * KC);
            __syncthreads();
            if (chC + 1 < nchunks) sload((chC + 1) * KC);
        }
        const int shift = a.tap_base + jC * a.tap_step - a.min_shift;  // >= 0
        const float* bj = xs + (chC & 1) * bufsz + half * a.span_pad + wn * (NJ * 32) + l31 + shift;
#pragma unroll
        for (int cp = 0; cp < KC / 2; ++cp) {
            float bf[NJ];
#pragma unroll
            for (int n = 0; n < NJ; ++n) bf[n] = bj[(2 * cp) * a.span_pad + n * 32];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int n = 0; n < NJ; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cp][i], bf[n], acc[i][n], 0, 0, 0);
        }
        if (++jC == a.ntaps) {
            jC = 0;
            ++chC;
        }
    };
    int chL = 0, jL = 0;   // weight-load cursor (one (chunk, tap) ahead of the compute cursor)
    auto advL = [&]() __attribute__((always_inline)) {
        if (++jL == a.ntaps) {
            jL = 0;
            ++chL;
        }
    };
    float wa[KC / 2][MI], wb[KC / 2][MI];
    const int total = nchunks * a.ntaps;
    loadA(wa, 0, 0);
    advL();
    sload(0);
    scommit(xs, 0);
    __syncthreads();
    if (nchunks > 1) sload(KC);
    for (int g = 0; g < total; g += 2) {
        if (g + 1 < total) {
            loadA(wb, chL, jL);
            advL();
        }
        step(wa);
        if (g + 2 < total) {
            loadA(wa, chL, jL);
            advL();
        }
        if (g + 1 < total) step(wb);
    }

    // ---- epilogue: bias + residual + scale + activation (+ running sum) --------------------------
    const int q_hi = a.q_lo + a.q_cnt;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int n = 0; n < NJ; ++n) {
            const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
            const long o = (long)q * a.out_stride + a.out_off;
            const bool qok = (q < q_hi) && (o >= 0) && (o < a.Lout);
            int cb = (cot0 + i) * 32;
            long oo = o;
            bool ok = qok;
            if (a.vphase) {   // virtual row tile -> (phase r, real channel tile); tiles never straddle phases (Cout % 32 == 0)
                const int r = cb / a.vphase;
                cb -= r * a.vphase;
                oo += r;
                ok = (q < q_hi) && (oo >= 0) && (oo < a.Lout) && (r < a.out_stride);
            }
            epilogue_tile(acc[i][n], a, b, cb, oo, ok, half, 1.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Split-precision path: every fp32 value v is carried as two halves  v = hi + lo  (hi = fp16(v), lo = fp16(v - hi),
// 22 significant bits) and the product is evaluated as  hi_w*hi_x + hi_w*lo_x + lo_w*hi_x  on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation: fp16 x fp16 products are exact in fp32, the dropped lo*lo term is
// 2^-22 relative, so the result carries ~fp32 accuracy at 16/3 = 5.3x the fp32-MFMA rate.  Weights are pre-scaled by a
// power of two so that their low halves stay in fp16's normal range (unscaled exactly in the epilogue).
// Activations are expected within fp16 range (|x| < 65504).
//
// Workgroup = 4 waves side by side along N (time); all four share the M tile, so the weight fragments are staged
// ONCE per workgroup through LDS (double-buffered, prefetched one tap ahead) instead of once per wave from L2.
// Activation tile: LDS [position][16 channels] fp16 (hi and lo planes), so a B fragment (8 consecutive channels of
// one position) is a single 16-byte ds_read; the fp32 -> (hi,lo) split and the leaky-relu prologue happen while staging.
template <int MI, int NJ, int TMAX, bool FOLD = false>
__global__ __launch_bounds__(256, 2) void conv_f16x3_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NT = 4 * NJ * 32;
    constexpr int AFR = MI * 2 * 64;  // half8 items of one (tap, chunk) weight block of this workgroup's M tile
    // activation tile: four planes [channel-half h][hi|lo][position] of 16-byte items (8 fp16 channels), so that the 32
    // lanes of a half-wave read 32 CONSECUTIVE 16-byte slots (conflict-free ds_read_b128) and staging writes likewise
    half8* Xp = reinterpret_cast<half8*>(smem_raw);            // plane (h, pl) at Xp + (h*2 + pl) * span_pad
    half8* Ap = Xp + (size_t)4 * a.span_pad;                    // [ntaps][AFR]: ALL taps of the current channel chunk

    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = FOLD ? 0 : blockIdx.z;
    const int q0 = a.q_lo + blockIdx.x * NT;          // FOLD: first column of the folded sequence
    const int lin = (!FOLD && a.in_len) ? a.in_len[b] : a.Lin;
    if (!FOLD && a.out_len && (long)q0 * a.out_stride + a.out_off >= a.out_len[b]) return;
    const int cot0 = blockIdx.y * MI;
    const int cotN = a.CoutP >> 5;
    const int nchunks = a.CinP >> 4;
    float in_scale = a.in_scale, w_unscale = a.w_unscale;
    if (FOLD) {   // device-side range: see ConvArgs::amax_x
        const float sx = pow2_to(*a.amax_x * a.in_scale, SPLIT_X_TARGET), sw = pow2_to(*a.amax_w, SPLIT_W_TARGET);
        in_scale *= sx;
        w_unscale = 1.f / (sx * sw);
    }

    f32x16 acc[MI][NJ];
    bool acc_init = false;
    if constexpr (!FOLD) acc_init = a.acc_init != 0;
    if (acc_init) {
        // The square layers of the wide stages start their sums at (residual + running sum + bias) / w_unscale: the acc_init_add / acc_init_scale steps
        // conv_f16x3_wide_kernel calls too, so that a layer gives the same bits whichever of the two kernels the machine-fill rule picks (a short
        // utterance run alone takes this kernel, the same utterance inside a large batch the wide one).  Host guarantees: plain stride-1
        // convolution, no activation, no gate, out_scale == 1, B * Cout * Lout < 2^32.
        const float inv = 1.f / a.w_unscale;
        const float* first = a.resid ? a.resid : (a.accumulate ? a.y : nullptr);
        const float* second = (a.resid && a.accumulate) ? a.y : nullptr;
        const unsigned L1 = (unsigned)a.Lout;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const unsigned row0 = ((unsigned)b * a.Cout + (cot0 + i) * 32 + 4 * half) * L1;
            float bv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) bv[r] = 0.f;
            if (a.bias) {
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = a.bias[(cot0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
            }
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
                const unsigned o = row0 + (unsigned)(q < a.Lout ? q : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.f;
                if (first) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][n][r] = first[o + (unsigned)((r & 3) + 8 * (r >> 2)) * L1];
                }
                if (second) {
                    float sv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) sv[r] = second[o + (unsigned)((r & 3) + 8 * (r >> 2)) * L1];
                    acc_init_add(acc[i][n], sv);
                }
                acc_init_add(acc[i][n], bv);
                acc_init_scale(acc[i][n], inv);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    // FOLD (training) launches also take grouped layers: a row tile only meets the input channels of its own group(s), a.Cin of them
    const int cin0 = (FOLD && a.groups > 1) ? ((blockIdx.y * (MI * 32)) / a.cout_g) * a.cin_g : 0;
    const float* xb = a.x + (FOLD ? (size_t)cin0 * a.Lin : (size_t)b * a.Cin * a.Lin);
    const int cin_n = (FOLD && a.groups > 1) ? min(a.Cin, a.CinTot - cin0) : a.Cin;   // (the last row tile may hold fewer groups than a full one)
    const int lo = q0 + a.min_shift;
    const half8* wsrc = reinterpret_cast<const half8*>(a.wph);

    // Both operands are software-pipelined through registers ONE CHANNEL CHUNK ahead: the global loads of chunk c+1
    // (activation window and the weight fragments of all taps) are issued before the MFMA loop of chunk c and
    // committed to LDS after it, so their latency hides behind ntaps*MI*NJ*3 MFMAs and the tap loop itself has no
    // barrier and no global access.  Addresses are clamped and loads unconditional (selects zero the padding) so the
    // compiler never branches around a load.
    constexpr int APT = (TMAX * AFR + 255) / 256;  // weight items per thread per chunk
    const int a_items = a.ntaps * AFR;
    half8 areg[APT];
    auto a_issue = [&](int c) {
#pragma unroll
        for (int e = 0; e < APT; ++e) {
            int idx = tid + e * 256;
            idx = idx < a_items ? idx : a_items - 1;
            const int j = idx / AFR, r = idx - j * AFR;
            areg[e] = wsrc[((size_t)(j * nchunks + c) * cotN + cot0) * 128 + r];
        }
    };
    auto a_commit = [&]() {
#pragma unroll
        for (int e = 0; e < APT; ++e) {
            const int idx = tid + e * 256;
            if (idx < a_items) Ap[idx] = areg[e];
        }
    };
    // ---- activation staging: fp32 [B,C,L]; work item = (position p, channel group h of 8): 8 dword loads, leaky-relu + hi/lo
    // split in x_commit
    constexpr int XIT = ((NT + 64) * 2 + 255) / 256;
    const int spanp = (a.span + 63) & ~63;
    float xr[XIT][8];
    unsigned xoff[XIT];
    int xslot[XIT];   // LDS item index, or -1
    bool xok[XIT];
    int xh[XIT];      // channel half (0/1)
#pragma unroll
    for (int e = 0; e < XIT; ++e) {
        const int i = tid + e * 256;
        const int h = i / spanp;              // spanp is a multiple of 64: cheap shifts would do, this runs once
        const int p = i - h * spanp;
        const int pos = lo + p;
        if (FOLD) {   // folded coordinate -> (sequence, position); the gap between sequences and everything outside the batch reads as zero
            const int sq = pos >= 0 ? pos / a.fold_S : 0;
            const int pp = pos - sq * a.fold_S;
            xok[e] = pos >= 0 && sq < a.fold_B && pp < lin;
            xoff[e] = xok[e] ? (unsigned)sq * (unsigned)(a.CinTot * a.Lin) + (unsigned)pp : 0u;
        } else {
            xok[e] = pos >= 0 && pos < lin;
            int pc = pos > lin - 1 ? lin - 1 : pos;
            pc = pc < 0 ? 0 : pc;
            xoff[e] = (unsigned)pc;
        }
        xh[e] = h;
        xslot[e] = (p < a.span && h < 2) ? (h * 2) * a.span_pad + p : -1;
    }
    auto x_issue = [&](int c) {
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
            // the two channel rows (h = 0 / 1) of this step are wave-uniform scalars: sgpr base + vgpr offset
            const int c0 = c * 16 + ch, c1 = c * 16 + 8 + ch;
            const float* r0 = xb + (size_t)(c0 < cin_n ? c0 : cin_n - 1) * a.Lin;
            const float* r1 = xb + (size_t)(c1 < cin_n ? c1 : cin_n - 1) * a.Lin;
#pragma unroll
            for (int e = 0; e < XIT; ++e) xr[e][ch] = (xh[e] ? r1 : r0)[xoff[e]];
        }
    };
    auto x_commit = [&](int c) {
#pragma unroll
        for (int e = 0; e < XIT; ++e) {
            if (xslot[e] >= 0) {
                const int cb = c * 16 + xh[e] * 8;
                const half8x2 v = lrelu_split8(xr[e], in_scale, a.in_slope, [&](int ch) { return xok[e] && cb + ch < cin_n; });
                Xp[xslot[e]] = v.hi;
                Xp[xslot[e] + a.span_pad] = v.lo;
            }
        }
    };

    x_issue(0);
    a_issue(0);
    for (int c = 0; c < nchunks; ++c) {
        if (c) __syncthreads();  // everyone finished reading chunk c-1 from LDS
        if (!TTSC_DBG(a, 1)) {
            x_commit(c);
            a_commit();
        }
        __syncthreads();
        if (c + 1 < nchunks && !TTSC_DBG(a, 8)) {
            x_issue(c + 1);
            a_issue(c + 1);
        }
        if (TTSC_DBG(a, 2)) continue;
        // per-lane LDS bases are loop invariants; inside the tap loop only `shift` / the tap's block offset are added
        // (32-bit LDS addressing, immediate offsets for the fragment index) — VALU work per MFMA matters here because
        // VALU and MFMA issue from the same in-order wave
        const half8* xh = Xp + (unsigned)((half * 2 + 0) * a.span_pad + wn * (NJ * 32) + l31);
        const half8* xl = Xp + (unsigned)((half * 2 + 1) * a.span_pad + wn * (NJ * 32) + l31);
        const half8* al_base = Ap + lane;
        int shift = a.tap_base - a.min_shift;
        for (int j = 0; j < a.ntaps; ++j, shift += a.tap_step) {
            const half8* Ab = al_base + j * AFR;
            half8 ah[MI], al[MI], bh[NJ], bl[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = Ab[(i * 2 + 0) * 64];
                al[i] = Ab[(i * 2 + 1) * 64];
            }
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                bh[n] = xh[shift + n * 32];
                bl[n] = xl[shift + n * 32];
            }
            TTSC_MFMA3_F16X3(MI, NJ, acc, ah, al, bh, bl);
        }
    }

    const int q_hi = a.q_lo + a.q_cnt;
    if (TTSC_DBG(a, 4)) {
        if (acc[0][0][0] == 12345.678f) a.y[0] = 1.f;  // keep the accumulators alive
        return;
    }
    float ymax = 0.f;                                  // FOLD: max |y| over this lane's stored elements (ConvArgs::amax_out)
    float* const ymax_p = (FOLD && a.amax_out) ? &ymax : nullptr;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int n = 0; n < NJ; ++n) {
            const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
            if (FOLD) {   // column of the folded sequence -> (sequence, position)
                const int sq = q / a.fold_S, pp = q - sq * a.fold_S;
                epilogue_tile(acc[i][n], a, sq < a.fold_B ? sq : 0, (cot0 + i) * 32, (long)pp, sq < a.fold_B && pp < a.Lout, half, w_unscale, ymax_p);
                continue;
            }
            if (acc_init) {   // everything but the weight scale is in the sum already
                if (q < q_hi && q < a.Lout) {
                    acc_init_store(acc[i][n], a.w_unscale, a.y + ((size_t)b * a.Cout + (cot0 + i) * 32 + 4 * half) * a.Lout + q, a.Lout);
                }
                continue;
            }
            const long o = (long)q * a.out_stride + a.out_off;
            const bool qok = (q < q_hi) && (o >= 0) && (o < a.Lout);
            int cb = (cot0 + i) * 32;
            long oo = o;
            bool ok = qok;
            if (a.vphase == -4) {   // interleaved rows (phase, channel): four consecutive samples per lane
                epilogue_tile_v4(acc[i][n], a, b, cb, q, (q < q_hi) && (q >= 0) && ((long)q * 4 + 3 < a.Lout), half, w_unscale);
                continue;
            }
            if (a.vphase) {   // virtual row tile -> (phase r, real channel tile); tiles never straddle phases (Cout % 32 == 0)
                const int r = cb / a.vphase;
                cb -= r * a.vphase;
                oo += r;
                ok = (q < q_hi) && (oo >= 0) && (oo < a.Lout) && (r < a.out_stride);
            }
            epilogue_tile(acc[i][n], a, b, cb, oo, ok, half, w_unscale);
        }
    }
    if constexpr (FOLD) {
        if (a.amax_out) {   // one atomic per workgroup, and only when it can still raise the word (most workgroups find it raised already)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ymax = fmaxf(ymax, __shfl_xor(ymax, off));
            float* red = reinterpret_cast<float*>(smem_raw);
            __syncthreads();   // the last chunk's fragment reads are done
            if (lane == 0) red[wn] = ymax;
            __syncthreads();
            if (tid == 0) {
                const unsigned bits = __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
                if (bits > __hip_atomic_load(a.amax_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.amax_out, bits);
            }
        }
    }
}

}  // namespace ttsc
