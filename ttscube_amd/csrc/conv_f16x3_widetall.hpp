// The wide- and tall-tile split-precision convolution kernels (conv_f16x3_wide_kernel: the square ResBlock layers of the wide stages;
// conv_f16x3_tall_kernel: the first two upsamplers), the tile pipeline both are built on, and their launchers.  Included by conv1d.hip only.
#pragma once
#include <type_traits>

#include "conv_kernels.hpp"

namespace ttsc {

// ---------------------------------------------------------------------------------------------------------------
// Wide-tile variant for the square layers of the wide stages (Cin = Cout in {128, 256}, K in {3, 7, 11}, dilation 1/3/5).
// What bounds conv_f16x3_kernel there (PMC, round 1: MFMA pipe 47 % busy, 4.8 VALU per MFMA, a third of the wave cycles
// parked at barriers) is structural: a workgroup owns 64 output channels, so the same activation window is loaded,
// leaky-relu'ed and split by Cout/64 workgroups, and every channel chunk costs two barriers with nothing in flight.
// Here
//   * a wave owns 64 x 128 outputs (MI = 2, NJ = 4: 24 MFMAs per tap for 8 activation- and 4 weight-fragment reads), four
//     waves form a 128 x 256 workgroup tile: the activation window is staged once per 128 output channels;
//   * weight fragments travel global -> LDS by LDS-DMA one tap ahead (no VGPRs, two 1-KB instructions per wave and tap) and
//     are shared by the two waves of a row tile; the barrier that ends a tap publishes them.  (Round-2 ablation: per-wave
//     global -> register fragment loads cost ~30 % of this kernel's time in the CU's vector-memory path.)
//   * the activation tile is double-buffered in LDS: chunk c+1 is converted and written while chunk c is multiplied
//     (the conversion's VALU work sits between MFMAs of the same wave);
//   * the global loads of chunk c+2 are issued right after chunk c+1 left the staging registers.
// K and the dilation are template parameters: the tap loop is unrolled and every LDS address is base register + immediate.
// Staging, weight DMA and tap loop are F16x3TilePipe below, shared with the tall kernel.
// (Round 5, measured and dropped: FOUR weight slots with the fragments of two steps travelling together and a barrier every second step —
// 4 / 8 / 12 barriers per two chunks for K = 3 / 7 / 11 instead of 6 / 14 / 22: 42.84-42.93 ms per forward against 42.96-43.03 with two slots in
// the product build, i.e. inside the noise, and 30-55 % SLOWER in the -DTTSC_ABLATE build of the very same source (profiles/r05_wg_timeline_slots.log) —
// a schedule that fragile is not worth 0.1 ms.)
// LEAN (wide and tall kernels; host switch TTSC_CONV_LEAN, default on): the staging pass carries no address arithmetic and no padding selects.
//   * the eight loads of a staging item go through ONE raw buffer descriptor per workgroup (its utterance's input: base x + b*C*Lin, C*Lin*4 bytes,
//     stride 0) with ONE 32-bit per-lane byte offset; the channel row is the instruction's scalar offset (wave-uniform: scalar adds, no
//     v_lshl_add_u64 per load);
//   * a raw buffer load returns 0 for an offset outside the descriptor, so lanes whose position lies outside [0, lin) — and the lanes that only
//     feed the dump slot — carry LEAN_OOB as their offset and the per-value `xok ? v * scale : 0` select goes: 0.0f * in_scale (finite, positive:
//     checked by the host), the leaky-relu and the split of +0 give the bits the select gave.  Whether the hardware's range check adds the scalar
//     offset or not does not matter: the host requires C*Lin*4 < 2^31, so LEAN_OOB alone is beyond the range and LEAN_OOB + row offset does not
//     wrap, while every real access (per-lane offset + row offset) ends below C*Lin*4 either way.
// LEAN = false is the kernel as it was (also taken when the input is too large for 32-bit byte offsets).
static constexpr unsigned LEAN_OOB = 0x80000000u;
__device__ __forceinline__ float lean_load(__amdgpu_buffer_rsrc_t rs, unsigned voff, int soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, soff, 0));
}

// fragment column of tap j inside the staged window: a Conv1d tap reads x[q - pad + j * D], a transposed tap x[q - j] (the window starts J - 1 early)
template <int D>
struct ColDilated {
    static constexpr int at(int j) { return j * D; }
};
template <int J>
struct ColReversed {
    static constexpr int at(int j) { return J - 1 - j; }
};

// The tile pipeline of the wide and tall kernels: 2 x 2 waves of MI x NJ MFMA tiles; per 16-channel chunk the activation window of SPAN
// positions sits in one of two LDS buffers as four planes (channel half h, hi | lo) of 16-byte items plus a dump slot pair, the weight
// fragments of one (tap, chunk) step in one of two LDS slots.  A kernel keeps its tile decoding, accumulators, prologue order, tap count and
// epilogue to itself.
template <int CIN, int SPAN, int MI, int NJ, bool LEAN, class COL>
struct F16x3TilePipe {
    static constexpr int SPANP = (SPAN + 63) & ~63;
    static constexpr int BUFSZ = 4 * SPAN + 2;            // items per activation buffer: 4 planes + the dump slot pair
    static constexpr int NCHUNK = CIN / 16;
    static constexpr int AITEMS = 2 * MI * 2 * 64;        // weight items of one (tap, chunk) for the workgroup's 2 * MI row tiles
    static constexpr int XIT = (2 * SPANP + 255) / 256;   // staging items per thread and chunk
    static constexpr size_t LDS_BYTES = (size_t)2 * BUFSZ * 16 + (size_t)2 * AITEMS * 16;   // activations + 2 weight slots
    static_assert(NCHUNK % 2 == 0, "slot parity: chunks in pairs (two chunks of NTAPS taps each end on the slot they started on)");

    // the ConvArgs fields the pipeline reads, as copies: a reference to the kernel's argument struct handed to the constructor keeps the struct
    // in memory until the call is inlined, and the wide kernel then compiles its operand selection into branches (30 more per kernel)
    int Lin;
    float in_scale, in_slope;
    int dbg;
    half8* Xp;   // [2 buffers][plane (h, pl)][SPAN] 16-byte items
    half8* Aw;   // [2 slots][AITEMS] weight fragments
    const float* xb;
    const half8* wsrc;
    int cotN;       // 32-row tiles of the layer: the (tap, chunk) blocks of the packed weights are cotN * 128 items apart
    int wave;       // index of the wave's blocks in the weight DMA (a vector or a scalar value: the kernel's choice)
    __amdgpu_buffer_rsrc_t xrs;
    int xrow;       // bytes per channel row
    const half8* xbase;
    const half8* abase;
    // activation staging: work item = (channel half h, position p) = 8 fp32 channels -> one (hi, lo) pair of items
    float xr[XIT][8];
    unsigned xoff[XIT];
    int xslot[XIT];
    bool xok[XIT], xlive[XIT];   // position inside [0, lin) / item inside the window (else: dump slot)

    // xb: the utterance's input; lo: x position of LDS column 0; wsrc: this lane's item of the workgroup's first row tile in block (0, 0)
    __device__ __forceinline__ F16x3TilePipe(const ConvArgs& a, char* smem, const float* xb_, int lo, int lin, const half8* wsrc_, int cotN_,
                                             int wave_, int wm, int wn)
        : Lin(a.Lin), in_scale(a.in_scale), in_slope(a.in_slope), dbg(a.dbg), Xp(reinterpret_cast<half8*>(smem)), Aw(Xp + 2 * BUFSZ), xb(xb_), wsrc(wsrc_), cotN(cotN_), wave(wave_) {
        const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
#pragma unroll
        for (int e = 0; e < XIT; ++e) {
            const int i = tid + e * 256;
            const int h = i >= SPANP ? 1 : 0;
            const int p = i - h * SPANP;
            const int pos = lo + p;
            xok[e] = pos >= 0 && pos < lin;
            int pc = pos > lin - 1 ? lin - 1 : pos;
            pc = pc < 0 ? 0 : pc;
            xoff[e] = (unsigned)(h * 8 * Lin + pc);   // channel half folded into the offset
            // lanes beyond the window write to a dump slot behind the planes (no divergent branch around the LDS stores)
            xlive[e] = p < SPAN && i < 2 * SPANP;
            xslot[e] = xlive[e] ? (h * 2) * SPAN + p : 4 * SPAN;
            if (LEAN) xoff[e] = (xok[e] && xlive[e]) ? xoff[e] * 4u : LEAN_OOB;   // byte offset, or one no access can have: the load returns 0
        }
        xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, LEAN ? CIN * Lin * 4 : 0, 0x00020000);
        xrow = Lin * 4;
        // all LDS reads of a wave hang off two base registers: buffer, plane, slot and tap offsets are immediates (the tap columns and the tile
        // are template parameters) — per-tap address registers were what pushed the first version of the wide kernel into scratch
        xbase = Xp + (unsigned)((half * 2) * SPAN + wn * (NJ * 32) + l31);
        abase = Aw + (unsigned)(wm * (MI * 128) + lane);
    }

    // weights: global -> LDS by LDS-DMA, one (tap, chunk) step ahead; the two waves that share a row tile read them back as ds_read_b128.
    // Fetched per wave straight into registers (the first version of the wide kernel) the fragments cost ~30 % of the run time in the CU's
    // vector-memory path.
    __device__ __forceinline__ void stage_A(int c, int j, int slot) const {
        if (TTSC_DBG(*this, 8)) return;
        const half8* wj = wsrc + (size_t)(j * NCHUNK + c) * ((size_t)cotN * 128);
#pragma unroll
        for (int i = 0; i < AITEMS / 64 / 4; ++i) {
            const int blk = wave + i * 4;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wj + blk * 64),
                                             (__attribute__((address_space(3))) void*)(Aw + slot * AITEMS + blk * 64), 16, 0, 0);
        }
    }
    // the eight loads of staging item e for chunk c
    __device__ __forceinline__ void issue(int e, int c) {
        if constexpr (LEAN) {
            const int s0 = c * 16 * xrow;   // the chunk's first row: scalar, like the seven that follow
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) xr[e][ch] = lean_load(xrs, xoff[e], s0 + ch * xrow);
        } else {
            const float* rc = xb + (size_t)(c * 16) * Lin;
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) xr[e][ch] = rc[(size_t)ch * Lin + xoff[e]];
        }
    }
    // staging item e -> activation buffer `buf` (LEAN: a lane outside the data loaded 0.0f, see LEAN_OOB)
    __device__ __forceinline__ void commit(int e, int buf) {
        half8* dst = Xp + buf * BUFSZ;
        const half8x2 v = lrelu_split8(xr[e], in_scale, in_slope, [&](int) { return LEAN || xok[e]; });
        dst[xslot[e]] = v.hi;
        dst[xslot[e] + (xlive[e] ? SPAN : 1)] = v.lo;   // (the dump slot's partner is the item right behind it)
    }

    // One channel chunk: NTAPS taps on activation buffer BUF; meanwhile chunk c+1 is converted into the other buffer and the loads of
    // chunk c+2 are issued (item e at tap NTAPS-1-e, so that a tap carries at most one item's conversion).  PAR = weight slot of the
    // chunk's first tap (it flips from chunk to chunk when NTAPS is odd).  One barrier per tap: it publishes the next tap's weights and,
    // after the last tap, the next chunk's activations.
    template <int BUF, int PAR, int NTAPS>
    __device__ __forceinline__ void chunk(int c, f32x16 (&acc)[MI][NJ]) {
        static_assert(XIT <= NTAPS, "one staging item per tap");
#pragma unroll
        for (int j = 0; j < NTAPS; ++j) {
            const int slot = (PAR + j) & 1;
            // the next step's weights leave first, then (staging taps) the loads of chunk c+2 ...
            if (j + 1 < NTAPS)
                stage_A(c, j + 1, slot ^ 1);
            else
                stage_A(c + 1 < NCHUNK ? c + 1 : c, 0, slot ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            half8 ah[MI], al[MI], bh[NJ], bl[NJ];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = abase[slot * AITEMS + i * 128];
                al[i] = abase[slot * AITEMS + i * 128 + 64];
            }
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                bh[n] = xbase[BUF * BUFSZ + COL::at(j) + n * 32];
                bl[n] = xbase[BUF * BUFSZ + SPAN + COL::at(j) + n * 32];
            }
            // ... then, on the staging taps (the last XIT taps of a chunk, one item each), chunk c+1 is converted and published and the
            // staging registers are refilled with chunk c+2 — the compiler interleaves this VALU work with the tap's MFMAs (past the last
            // chunk it handles clamped garbage nobody reads: no branches)
            const int e = NTAPS - 1 - j;
            if (e < XIT && !TTSC_DBG(*this, 1)) {
                commit(e, 1 - BUF);
                issue(e, c + 2 < NCHUNK ? c + 2 : NCHUNK - 1);
            }
            TTSC_MFMA3_F16X3(MI, NJ, acc, ah, al, bh, bl);
            __builtin_amdgcn_sched_barrier(0);
            if (!TTSC_DBG(*this, 2)) __syncthreads();
        }
    }
    // all chunks, NTAPS taps each; on entry chunk 0 is in buffer 0, chunk 1 in the staging registers and the first weight step on its way
    template <int NTAPS>
    __device__ __forceinline__ void run(f32x16 (&acc)[MI][NJ]) {
        for (int c = 0; c < NCHUNK; c += 2) {
            chunk<0, 0, NTAPS>(c, acc);
            chunk<1, (NTAPS & 1), NTAPS>(c + 1, acc);
        }
    }
};

// wide: 256 positions + the "same" padding's halo (K-1)*D staged per channel; tall: 2 * NJ * 32 input positions + the J - 1 earlier ones
template <int C, int K, int D, bool LEAN>
using WidePipe = F16x3TilePipe<C, 256 + (K - 1) * D, 2, 4, LEAN, ColDilated<D>>;
template <int CIN, int J, int MI, int NJ, bool LEAN>
using TallPipe = F16x3TilePipe<CIN, 2 * NJ * 32 + (J - 1), MI, NJ, LEAN, ColReversed<J>>;

template <int C, int K, int D, bool LEAN>
__global__ __launch_bounds__(256, 2) void conv_f16x3_wide_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int WM = 2, WN = 2;                   // 128 output channels x 256 positions per workgroup (grid.y = C / 128)
    constexpr int MI = 2, NJ = 4, NT = WN * NJ * 32;
    typedef WidePipe<C, K, D, LEAN> Pipe;
    constexpr int XIT = Pipe::XIT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const int q0 = blockIdx.x * NT;
    const int lin = a.in_len ? a.in_len[b] : a.Lin;
    if (a.out_len && q0 >= a.out_len[b]) return;
    const int cotg = blockIdx.y * (WM * MI);        // first 32-row tile of the workgroup
#ifdef TTSC_ABLATE
    const unsigned wg_lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
#endif
    TTSC_STAMP(a, wg_lin, 0);
    TTSC_STAMP_HWID(a, wg_lin, 15);

    // Accumulators.  With `acc_init` they START at (bias + residual + running sum) / w_unscale (w_unscale is a power of two: exact), so the
    // epilogue is 128 independent stores per lane.  Why: as epilogue operands the residual tile was fetched four rows at a time, load ->
    // wait -> store, 32 dependent round trips per wave with 1 KB in flight each — the workgroup timeline (tools/wg_timeline.py, round 5) put
    // 41-45 % of a workgroup's life into that epilogue for the K = 3 / K = 7 layers (56 us for 256 KB), and since the workgroups of a launch
    // run in step, the whole chip sat in it together.  Here all of a lane's 128 (256 with the running sum) loads leave back to back at the top
    // of the kernel, in front of the first activation chunk's, and land while the prologue waits for that chunk anyway.
    f32x16 acc[MI][NJ];
    // acc_init: operand sources and this lane's element offsets (32-bit: B * C * L < 2^32 checked by the host)
    const float* ai_first = a.acc_init ? (a.resid ? a.resid : (a.accumulate ? a.y : nullptr)) : nullptr;
    const float* ai_second = (a.acc_init && a.resid && a.accumulate) ? a.y : nullptr;
    const unsigned ai_L = (unsigned)a.Lout;
    const unsigned ai_row0 = ((unsigned)b * a.Cout + (cotg + wm * MI) * 32 + 4 * half) * ai_L;
    const int ai_qw = q0 + wn * (NJ * 32) + l31;
    // row tile i of the accumulators <- first operand (or zero); the loads of a row tile leave back to back
    auto acc_load_first = [&](int i) __attribute__((always_inline)) {
        if (ai_first) {
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                const int q = ai_qw + n * 32;
                const unsigned o = ai_row0 + (unsigned)(i * 32) * ai_L + (unsigned)(q < a.Lout ? q : 0);   // (columns beyond the row are never stored)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    unsigned og = o + (unsigned)(8 * g) * ai_L;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[i][n][4 * g + e] = ai_first[og];
                        og += ai_L;
                    }
                }
            }
        } else {
#pragma unroll
            for (int n = 0; n < NJ; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.f;
        }
    };
    // the rest of the initial value, in the order of acc_init_add / acc_init_scale: + running sum (when both operands are present), + bias, / weight scale
    auto acc_init_finish = [&]() __attribute__((always_inline)) {
        const float inv = 1.f / a.w_unscale;
        if (ai_second) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int n0 = 0; n0 < NJ; n0 += 2) {
                    float t[2][16];
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int q = ai_qw + (n0 + n) * 32;
                        const unsigned o = ai_row0 + (unsigned)(i * 32) * ai_L + (unsigned)(q < a.Lout ? q : 0);
#pragma unroll
                        for (int r = 0; r < 16; ++r) t[n][r] = ai_second[o + (unsigned)((r & 3) + 8 * (r >> 2)) * ai_L];
                    }
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc_init_add(acc[i][n0 + n], t[n]);
                }
        }
        if (a.bias) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                float bv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = a.bias[(cotg + wm * MI + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
                for (int n = 0; n < NJ; ++n) acc_init_add(acc[i][n], bv);
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int n = 0; n < NJ; ++n) acc_init_scale(acc[i][n], inv);
    };
    if (a.acc_init) {
        // (filled in the prologue below, between the activation loads: see acc_load_first / acc_init_finish)
    } else if (a.epi_prefetch && a.bias && (a.resid || a.accumulate)) {
        // prefetched epilogue: the bias starts the sum (divided by the weight scale, a power of two: exact), so the epilogue holds no bias registers
        const float inv = 1.f / a.w_unscale;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bv = a.bias[(cotg + wm * MI + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] * inv;
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j][r] = bv;
            }
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    const float* xb = a.x + (size_t)b * C * a.Lin;
    const int lo = q0 - D * ((K - 1) / 2);
    const half8* wsrc = reinterpret_cast<const half8*>(a.wph) + (size_t)cotg * 128 + lane;
    Pipe pipe(a, smem_raw, xb, lo, lin, wsrc, C / 32, wave, wm, wn);
    // prologue: chunk 0 -> buffer 0, chunk 1 into the staging registers, first weight step
    pipe.stage_A(0, 0, 0);
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.issue(e, 0);
    if (a.acc_init) {
        // the first row tile's operand loads leave BEHIND the first chunk's (loads return in order: the chunk's conversion below then waits for
        // its own loads only), the second row tile's behind the second chunk's; the arithmetic on them comes last
        __builtin_amdgcn_sched_barrier(0);
        acc_load_first(0);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.commit(e, 0);
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.issue(e, 1);
    if (a.acc_init) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 1; i < MI; ++i) acc_load_first(i);
        acc_init_finish();
    }
    __syncthreads();
    TTSC_STAMP(a, wg_lin, 1);
    pipe.template run<K>(acc);
    TTSC_STAMP(a, wg_lin, 2);

    if (TTSC_DBG(a, 4)) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int n = 0; n < NJ; ++n) t += acc[i][n][0] + acc[i][n][7];
        if (t == 12345.678f) a.y[0] = 1.f;   // keep the accumulators alive
        return;
    }
    if (a.acc_init) {
        // everything but the weight scale is already in the sum: independent stores, nothing to wait for
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
                if (q < a.Lout) acc_init_store(acc[i][n], a.w_unscale, a.y + ((size_t)b * a.Cout + (cotg + wm * MI + i) * 32 + 4 * half) * a.Lout + q, a.Lout);
            }
    } else if (a.epi_prefetch && (a.resid || a.accumulate)) {
        // Deep-prefetched epilogue.  Same arithmetic as epilogue_tile EXCEPT that the bias already sits in the accumulators (it started the sum, see their
        // initialisation: not bit-identical to the general kernel, which adds the bias after the sum — ADVICE r5): the residual (and running-sum) operands of the NEXT tiles
        // are in flight while a tile is finished and stored — four tiles ahead with one operand, two with both (64 registers: the fragment and
        // staging registers of the main loop are free now).  epilogue_tile fetched four rows at a time, load -> wait -> store: 32 dependent
        // round trips per wave with 1 KB in flight each; the workgroup timeline (tools/wg_timeline.py, round 5) put 41-45 % of a workgroup's
        // life into that for the K = 3 / K = 7 layers (56 us for 256 KB), and the workgroups of a launch run in step, so the chip sat in it together.
        const float* rsrc = a.resid;
        const float* ysrc = a.accumulate ? a.y : nullptr;
        constexpr int NTILE = MI * NJ;
        // 32-bit element offsets from the tensor base (B * C * L < 2^32 is checked by the host); the 16 rows of a tile follow from its first by adds
        const unsigned L1 = (unsigned)a.Lout;
        const unsigned row0 = ((unsigned)b * a.Cout + (cotg + wm * MI) * 32 + 4 * half) * L1;
        const int qw = q0 + wn * (NJ * 32) + l31;
        auto tile_off = [&](int t) __attribute__((always_inline)) -> unsigned {
            const int i = t / NJ, n = t % NJ;
            const int q = qw + n * 32;
            return row0 + (unsigned)(i * 32) * L1 + (unsigned)(q < a.Lout ? q : 0);
        };
        // MODE 0: residual only, 1: running sum only, 2: both (compile-time: no per-element selects)
        auto body = [&](auto mode_tag) __attribute__((always_inline)) {
            constexpr int MODE = decltype(mode_tag)::value;
            constexpr bool BOTH = MODE == 2;
            constexpr int DEPTH = BOTH ? 1 : 3;   // (register budget: 128 accumulators + 48 / 32 operand registers)
            const float* s0 = MODE == 1 ? ysrc : rsrc;
            float t0[DEPTH][16], t1[BOTH ? DEPTH : 1][16];
            auto issue = [&](int t) __attribute__((always_inline)) {
                unsigned o = tile_off(t);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    unsigned og = o + (unsigned)(8 * g) * L1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        t0[t % DEPTH][4 * g + e] = s0[og];
                        if constexpr (BOTH) t1[t % DEPTH][4 * g + e] = ysrc[og];
                        og += L1;
                    }
                }
            };
            // (the bias is already in the accumulators: see their initialisation)
#pragma unroll
            for (int t = 0; t < DEPTH; ++t) issue(t);
#pragma unroll
            for (int t = 0; t < NTILE; ++t) {
                const int i = t / NJ, n = t % NJ;
                float res[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float u = acc[i][n][r] * a.w_unscale;
                    if constexpr (MODE == 0) res[r] = (u + t0[t % DEPTH][r]) * a.out_scale + 0.f;
                    if constexpr (MODE == 1) res[r] = (u + 0.f) * a.out_scale + t0[t % DEPTH][r];
                    if constexpr (MODE == 2) res[r] = (u + t0[t % DEPTH][r]) * a.out_scale + t1[t % DEPTH][r];
                }
                if (qw + n * 32 < a.Lout) {
                    unsigned o = tile_off(t);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        unsigned og = o + (unsigned)(8 * g) * L1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            a.y[og] = res[4 * g + e];
                            og += L1;
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // (the next tile's loads stay behind this tile's stores)
                if (t + DEPTH < NTILE) issue(t + DEPTH);
            }
        };
        if (rsrc && ysrc)
            body(std::integral_constant<int, 2>());
        else if (rsrc)
            body(std::integral_constant<int, 0>());
        else
            body(std::integral_constant<int, 1>());
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int n = 0; n < NJ; ++n) {
                const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
                epilogue_tile(acc[i][n], a, b, (cotg + wm * MI + i) * 32, q, q < a.Lout, half, a.w_unscale);
            }
        }
    }
#ifdef TTSC_ABLATE
    if (a.prof) {
        __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0): the stores have been accepted
        TTSC_STAMP(a, wg_lin, 3);
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// Tall-tile variant for the first two upsamplers (ConvTranspose1d 512 -> 256, k16 s5 and 256 -> 128, k16 s3).  As GEMMs they are 1280 / 768
// "virtual rows" (phase, channel) x CIN * J deep over the INPUT positions, J = ceil(K / stride) taps reading x[q - j].  The general kernel
// runs them as 20 / 12 M tiles of 64 rows that each load, leaky-relu and split the same input window: the ablation (tools/ablate.py --ups)
// puts 45 % of their time into that staging.  Here a workgroup owns 256 rows x 128 input positions (2 x 2 waves of 4 x 2 MFMA tiles: the
// same 24 MFMAs per 12 fragment reads as the wide kernel), so the window is staged 5 / 3 times instead of 20 / 12, on the wide kernel's
// pipeline (F16x3TilePipe): weights by LDS-DMA one tap ahead, activations double-buffered, conversion of chunk c+1 spread over the last taps of chunk c.
// (MI, NJ) = (4, 2): 256 rows x 128 positions (ups.0: 1280 rows); (2, 4): 128 rows x 256 positions (ups.1: 384 rows = 3 tiles instead of 6).
// LEAN (see conv_f16x3_wide_kernel): the staging loads go through the buffer descriptor, and a workgroup whose row tile is a phase without the
// last tap (phase r has ceil((K - r) / stride) real taps: 4 3 3 3 3 of J = 4 for ups.0, 6 5 5 of J = 6 for ups.1; the packers fill tap J - 1 of
// the others with zero weights) runs J - 1 taps per chunk: no weight LDS-DMA, no fragment reads, no 24 MFMAs and no barrier for the zero tap.
// The real taps and their order are unchanged, so every finite output keeps its bits (a zero tap only ever added +0 to a sum that started at +0).
template <int CIN, int J, int MI, int NJ, bool LEAN>
__global__ __launch_bounds__(256, 2) void conv_f16x3_tall_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int WM = 2, WN = 2, NT = WN * NJ * 32;
    typedef TallPipe<CIN, J, MI, NJ, LEAN> Pipe;
    constexpr int XIT = Pipe::XIT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    // Which tile?  The row tiles of a transposed convolution are its PHASES: they write interleaved samples of the same output rows, every
    // 128-byte line of the output gets a fifth (stride 5) / a third (stride 3) of its bytes from each of them.  Dispatched as a 3-D grid the
    // phases of a q tile land on different XCDs — workgroup i runs on XCD i mod 8 (tools/probes/xcc_probe.hip) — whose L2s cannot merge the
    // partial lines: the 512 -> 256, k16 s5 upsampler wrote 1311 MB for a 262 MB tensor (round-4 PMC).  As a 1-D launch the id is decoded so
    // that the phases of one q tile are consecutive workgroups of ONE XCD: its L2 sees all pieces of a line within a few microseconds.
    int bx, by, bz;
    if (a.swz_nx > 0) {
        const unsigned id = blockIdx.x, xcd = id & 7u, u = id >> 3;
        by = (int)(u % (unsigned)a.swz_ny);
        const unsigned t = (u / (unsigned)a.swz_ny) * 8u + xcd;      // q tile x utterance, linear
        bx = (int)(t % (unsigned)a.swz_nx);
        bz = (int)(t / (unsigned)a.swz_nx);
        if (bz >= a.fold_B) return;   // (padding of the launch to a multiple of 8 tiles; fold_B carries the batch size here)
    } else {
        bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    }
    const int b = bz;
    const int q0 = a.q_lo + bx * NT;          // first INPUT position of the tile
    const int lin = a.in_len ? a.in_len[b] : a.Lin;
    if (a.out_len && (long)q0 * a.out_stride + a.out_off >= a.out_len[b]) return;
    const int cotg = by * (WM * MI);
    const int cotN = a.CoutP >> 5;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const float* xb = a.x + (size_t)b * CIN * a.Lin;
    const int lo = q0 - (J - 1);                      // x position of LDS column 0 (tap j reads column (q - q0) + J - 1 - j)
    const half8* wsrc = reinterpret_cast<const half8*>(a.wph) + (size_t)cotg * 128 + lane;
    // (LEAN: the wave index as a scalar, so that the block addresses of the weight LDS-DMA are scalar arithmetic; as a vector value its 64-bit
    // copy was live across the tap loops and, with two of them in the kernel, went to scratch in the <256, 6, 2, 4> instantiation)
    const int wave_s = LEAN ? __builtin_amdgcn_readfirstlane(wave) : wave;
    Pipe pipe(a, smem_raw, xb, lo, lin, wsrc, cotN, wave_s, wm, wn);
    pipe.stage_A(0, 0, 0);
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.issue(e, 0);
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.commit(e, 0);
#pragma unroll
    for (int e = 0; e < XIT; ++e) pipe.issue(e, 1);
    __syncthreads();
    // a row tile that is one phase with J - 1 real taps (workgroup-uniform) runs J - 1 taps per chunk; the staging items sit on the last XIT taps that EXIST
    if (LEAN && by >= a.short_from)
        pipe.template run<J - 1>(acc);
    else
        pipe.template run<J>(acc);
    // epilogue: virtual row tile -> (phase r, real channel tile); output position o = q * stride + r - padding
    const int q_hi = a.q_lo + a.q_cnt;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int n = 0; n < NJ; ++n) {
            const int q = q0 + wn * (NJ * 32) + n * 32 + l31;
            int cb = (cotg + wm * MI + i) * 32;
            const int r = cb / a.vphase;
            cb -= r * a.vphase;
            const long oo = (long)q * a.out_stride + a.out_off + r;
            const bool ok = (q < q_hi) && (oo >= 0) && (oo < a.Lout) && (r < a.out_stride);
            epilogue_tile(acc[i][n], a, b, cb, oo, ok, half, a.w_unscale);
        }
    }
}

template <int C, int K, int D, bool LEAN>
static int launch_f16_wide_l(const ConvArgs& a, int B, hipStream_t s) {
    constexpr int NT = 256;
    dim3 grid((unsigned)ceil_div(a.Lout, NT), (unsigned)(C / 128), (unsigned)B);
    // (a.acc_init — the operands as the accumulators' initial value, see the kernel — and a.epi_prefetch are decided by conv_plan for the LAYER,
    // not per kernel: the general kernel evaluates the same layer with the same arithmetic when the machine-fill rule sends it there)
    if (int rc = ensure_full_lds((const void*)conv_f16x3_wide_kernel<C, K, D, LEAN>)) return rc;   // once per (device, kernel)
    hipLaunchKernelGGL((conv_f16x3_wide_kernel<C, K, D, LEAN>), grid, dim3(256), (WidePipe<C, K, D, LEAN>::LDS_BYTES), s, a);
    return launch_checked("conv_f16x3_wide_kernel");
}

template <int C, int K, int D>
static int launch_f16_wide(const ConvArgs& a, int B, hipStream_t s) {
    return a.lean ? launch_f16_wide_l<C, K, D, true>(a, B, s) : launch_f16_wide_l<C, K, D, false>(a, B, s);
}

template <int CIN, int J, int MI, int NJ, bool LEAN>
static int launch_f16_tall_l(const ConvArgs& a, int B, hipStream_t s) {
    constexpr int NT = 2 * NJ * 32, MT = 2 * MI * 32;
    dim3 grid((unsigned)ceil_div(a.q_cnt, NT), (unsigned)(a.CoutP / MT), (unsigned)B);
    if (a.swz_nx > 0) {   // XCD-aware 1-D launch (see the kernel; conv_plan set swz_nx = grid.x, swz_ny = grid.y, fold_B = B)
        const unsigned tiles = (unsigned)round_up((int64_t)grid.x * B, 8);
        grid = dim3(tiles * grid.y, 1, 1);
    }
    if (int rc = ensure_full_lds((const void*)conv_f16x3_tall_kernel<CIN, J, MI, NJ, LEAN>)) return rc;
    hipLaunchKernelGGL((conv_f16x3_tall_kernel<CIN, J, MI, NJ, LEAN>), grid, dim3(256), (TallPipe<CIN, J, MI, NJ, LEAN>::LDS_BYTES), s, a);
    return launch_checked("conv_f16x3_tall_kernel");
}

template <int CIN, int J, int MI, int NJ>
static int launch_f16_tall(const ConvArgs& a, int B, hipStream_t s) {
    return a.lean ? launch_f16_tall_l<CIN, J, MI, NJ, true>(a, B, s) : launch_f16_tall_l<CIN, J, MI, NJ, false>(a, B, s);
}

template <int C, int K>
static int launch_f16_wide_d(const ConvArgs& a, int B, int d, hipStream_t s) {
    if (d == 1) return launch_f16_wide<C, K, 1>(a, B, s);
    if (d == 3) return launch_f16_wide<C, K, 3>(a, B, s);
    return launch_f16_wide<C, K, 5>(a, B, s);
}

template <int C>
static int launch_f16_wide_k(const ConvArgs& a, int B, int d, hipStream_t s) {
    if (a.ntaps == 3) return launch_f16_wide_d<C, 3>(a, B, d, s);
#ifdef TTSC_PROBE_EVENK
    if (a.ntaps == 4) return launch_f16_wide<C, 4, 1>(a, B, s);
    if (a.ntaps == 6) return launch_f16_wide<C, 6, 1>(a, B, s);
#endif
    if (a.ntaps == 7) return launch_f16_wide_d<C, 7>(a, B, d, s);
    return launch_f16_wide_d<C, 11>(a, B, d, s);
}

}  // namespace ttsc
