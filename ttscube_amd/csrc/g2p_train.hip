// Training side of the word-level G2P decoder (cube/networks/modules.py:58-88 Attention, 258-297 Seq2Seq.forward with gs_output, TRAIN mode) — gfx950.
// The reference's teacher-forced loop is ~15 small ops per decoder step forward and as many backward on a batch of 32 short words.  Here:
//   ttsc_g2p_train_forward    the start step and all T teacher-forced steps of every word in ONE launch; saves what the backward reads
//   ttsc_g2p_train_backward   the whole backward-through-time loop in ONE launch: per-step gate gradients (rows for the weight-gradient GEMMs),
//                             d query rows, and per word d enc, d pe and a partial of d v
//   ttsc_dropout_scale        y = x * keep / (1 - p) (the encoder's inter-layer dropout; the adjoint is the same call on dy)
// The shape of g2p.hip: one workgroup owns one word for all of its steps, nothing between workgroups (a word's bits do not depend on what else is
// in the launch), weights stream from L2 through rnn_chain.hpp's packed 16-byte loads, sizes come from the tensors.  The backward streams the
// TRANSPOSED matrices in the same packing ([W_ih1^T; W_hh1^T], [W_hh0^T; W_ic^T], W_aq^T): thread k owns input unit k.
// Rows: r = 0 is the start step (zero input, zero state), r = t + 1 is teacher-forced step t; every saved tensor has T + 1 rows per word.
// The energies tanh(aq + pe) are NOT stored ([B, T, N, A]): the backward recomputes them from the saved query projection aq [B, T, A].
// Accumulations over steps (d enc, d pe, d v) are read-modify-writes of words the same thread owns at every step, t descending: no atomics,
// the same bits every run.  Dropout masks are injected ({0,1} floats) or drawn from Philox-4x32-10: counter (element >> 2, row, word, tag +
// stream id), key = seed, word element & 3 — the backward draws the forward's words.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "../../include/ttscube_math.h"
#include "rnn_chain.hpp"

namespace ttsc {

unsigned* g2p_status_word();      // g2p.hip

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_NW = GT_THREADS / 64;
constexpr int GT_MAX_LDS = 64 * 1024;
constexpr unsigned GT_BAD_LABEL = 2u;
constexpr uint32_t GT_TAG_DEC = 0x47324400u, GT_TAG_ATT = 0x47324100u, GT_TAG_DROP = 0x47324500u;

struct GtLaunch {
    ttsc_g2p_train_args a;
    unsigned* status;
    float s_att, s_dec;      // 1 / (1 - p)
};

// dropout multiplier of one element: injected mask value, or Philox
__device__ __forceinline__ float gt_keep(const float* mask, size_t at, uint32_t idx, uint32_t row, uint32_t word, uint32_t tag, uint64_t seed, float p,
                                         float scale) {
    if (mask) return mask[at] * scale;
    if (p <= 0.f) return 1.f;
    uint32_t r4[4];
    ttsc_philox4x32(idx >> 2, row, word, tag, (uint32_t)seed, (uint32_t)(seed >> 32), r4);
    return ttsc_u01(r4[idx & 3]) >= p ? scale : 0.f;
}

// the multipliers of four consecutive elements (idx % 4 == 0): they are the four words of ONE Philox block
__device__ __forceinline__ void gt_keep4(const float* mask, size_t at, uint32_t idx, uint32_t row, uint32_t word, uint32_t tag, uint64_t seed, float p,
                                         float scale, float* k) {
    if (mask) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = mask[at + q] * scale;
        return;
    }
    if (p <= 0.f) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = 1.f;
        return;
    }
    uint32_t r4[4];
    ttsc_philox4x32(idx >> 2, row, word, tag, (uint32_t)seed, (uint32_t)(seed >> 32), r4);
#pragma unroll
    for (int q = 0; q < 4; ++q) k[q] = ttsc_u01(r4[q]) >= p ? scale : 0.f;
}

// the chain with g2p.hip's unrolls (pipelined when K / 4 is a multiple of the unroll, as at the reference's sizes; any K % 4 == 0 runs)
template <int NG>
__device__ __forceinline__ void gt_chain(float (&acc)[1][NG], const float* wp, int rows, int gstride, int row, const float* v, int K) {
    lstm_chain<1, NG, (NG > 2 ? 2 : 5)>(acc, wp, rows, gstride, row, v, 0, K);
}

__global__ __launch_bounds__(GT_THREADS) void g2p_train_fwd_kernel(const GtLaunch p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ttsc_g2p_train_args& a = p.a;
    const int E = a.E, A = a.A, D = a.D, N = a.N, T = a.T, D4 = 4 * a.D, XW = a.E + a.Em, R = a.T + 1;
    const int tid = threadIdx.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    float* h1 = sm;               // [2][D] layer 0's h (what its own recurrence reads: no dropout)
    float* h2 = h1 + 2 * D;       // [2][D]
    float* h1m = h2 + 2 * D;      // [D]    layer 0's h through the inter-layer dropout (what layer 1 reads)
    float* c1 = h1m + D;          // [D]
    float* c2 = c1 + D;           // [D]    (the attention query)
    float* aq = c2 + D;           // [A]
    float* ctx = aq + A;          // [E]
    const float* enc = a.enc_dev + (size_t)b * N * E;
    const float* pe = a.pe_dev + (size_t)b * N * A;
    float* sc = a.scratch_dev + (size_t)b * 2 * N;     // raw scores

    for (int j = tid; j < D; j += GT_THREADS) h1[j] = h2[j] = c1[j] = c2[j] = 0.f;
    for (int e = tid; e < E; e += GT_THREADS) ctx[e] = 0.f;
    __syncthreads();

    int cur = 0;
    for (int r = 0; r < R; ++r) {
        const int nxt = cur ^ 1;
        const size_t row = (size_t)b * R + r;
        if (r > 0) {
            const size_t bt = (size_t)b * T + (r - 1);
            // ---- attention, query half: aq = W_att[:, :D] . c2 (saved: the backward recomputes the energies from it) ----
            for (int j = tid; j < A; j += GT_THREADS) {
                float acc[1][1] = {{0.f}};
                gt_chain<1>(acc, a.w_aq, A, 0, j, c2, D);
                aq[j] = acc[0][0];
                a.aq_dev[bt * A + j] = acc[0][0];
            }
            __syncthreads();
            // ---- scores: sc_i = v . dropout(tanh(aq + pe_i)); a wave per position, butterfly sum ----
            for (int i = wave; i < N; i += GT_NW) {
                float s = 0.f;
                // a lane takes four consecutive j: they share one Philox block (A % 4 == 0, so i * A + j0 is a multiple of 4)
                for (int j0 = 4 * lane; j0 < A; j0 += 256) {
                    float k4[4];
                    gt_keep4(a.att_mask_dev, (bt * N + i) * A + j0, (uint32_t)(i * A + j0), (uint32_t)r, (uint32_t)b, GT_TAG_ATT + (uint32_t)a.stream_id,
                             a.seed, a.p_att, p.s_att, k4);
                    const float4 q4 = *reinterpret_cast<const float4*>(aq + j0);
                    const float4 p4 = *reinterpret_cast<const float4*>(pe + (size_t)i * A + j0);
                    const float4 v4 = *reinterpret_cast<const float4*>(a.v + j0);
                    s = fmaf(v4.x, ttsc_tanhf(q4.x + p4.x) * k4[0], s);
                    s = fmaf(v4.y, ttsc_tanhf(q4.y + p4.y) * k4[1], s);
                    s = fmaf(v4.z, ttsc_tanhf(q4.z + p4.z) * k4[2], s);
                    s = fmaf(v4.w, ttsc_tanhf(q4.w + p4.w) * k4[3], s);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0) sc[i] = s;
            }
            __syncthreads();
            // ---- softmax over ALL N positions (nothing is masked); every wave computes the same max and sum ----
            {
                float* at = a.att_dev + bt * N;
                float mx = -INFINITY;
                for (int i = lane; i < N; i += 64) mx = fmaxf(mx, sc[i]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                float sum = 0.f;
                for (int i = lane; i < N; i += 64) sum += ttsc_expf(sc[i] - mx);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
                for (int i = tid; i < N; i += GT_THREADS) at[i] = ttsc_expf(sc[i] - mx) / sum;
            }
            __syncthreads();
            // ---- context = sum_i a_i enc_i (i ascending), written into the decoder-input row [ctx; emb_prev] ----
            {
                const float* at = a.att_dev + bt * N;
                for (int e = tid; e < E; e += GT_THREADS) {
                    float acc = 0.f;
                    for (int i = 0; i < N; ++i) acc = fmaf(at[i], enc[(size_t)i * E + e], acc);
                    ctx[e] = acc;
                    a.x0_dev[row * XW + e] = acc;
                }
            }
            __syncthreads();
        }
        // ---- the teacher label fed back: 0 (zero embedding) at the start step and the first step, y[t - 1] after ----
        int last = -1;
        if (r >= 2) {
            last = a.y_dev[(size_t)b * T + (r - 2)];
            if (last < 0 || last >= a.L) {
                if (tid == 0) atomicOr(p.status, GT_BAD_LABEL);
                last = -1;
            }
        }
        // ---- LSTM layer 0: gates = b + W_ih0[:, :E] . ctx + tab[last] + W_hh0 . h1 ----
        for (int j = tid; j < D; j += GT_THREADS) {
            float acc[1][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[0][g] = a.b0[g * D + j];
            if (r > 0) {
                gt_chain<4>(acc, a.w_ic, D4, D, j, ctx, E);
                if (last >= 0) {
                    const float* tr = a.tab + (size_t)last * D4 + j;
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[0][g] += tr[g * D];
                }
                gt_chain<4>(acc, a.w_hh0, D4, D, j, h1 + cur * D, D);
            }
            const float ig = ttsc_sigmoidf(acc[0][0]), fg = ttsc_sigmoidf(acc[0][1]), gg = ttsc_tanhf(acc[0][2]), og = ttsc_sigmoidf(acc[0][3]);
            const float c = fmaf(fg, c1[j], ig * gg);
            const float h = og * ttsc_tanhf(c);
            c1[j] = c;
            h1[nxt * D + j] = h;
            float* gr = a.gates0_dev + row * D4 + j;
            gr[0] = ig; gr[D] = fg; gr[2 * D] = gg; gr[3 * D] = og;
            a.cells0_dev[row * D + j] = c;
            a.h1_dev[row * D + j] = h;
            const float hm = h * gt_keep(a.dec_mask_dev, row * D + j, (uint32_t)j, (uint32_t)r, (uint32_t)b, GT_TAG_DEC + (uint32_t)a.stream_id, a.seed,
                                         a.p_dec, p.s_dec);
            h1m[j] = hm;
            a.h1m_dev[row * D + j] = hm;
        }
        __syncthreads();
        // ---- LSTM layer 1 ----
        for (int j = tid; j < D; j += GT_THREADS) {
            float acc[1][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[0][g] = a.b1[g * D + j];
            gt_chain<4>(acc, a.w_ih1, D4, D, j, h1m, D);
            if (r > 0) gt_chain<4>(acc, a.w_hh1, D4, D, j, h2 + cur * D, D);
            const float ig = ttsc_sigmoidf(acc[0][0]), fg = ttsc_sigmoidf(acc[0][1]), gg = ttsc_tanhf(acc[0][2]), og = ttsc_sigmoidf(acc[0][3]);
            const float c = fmaf(fg, c2[j], ig * gg);
            const float h = og * ttsc_tanhf(c);
            c2[j] = c;
            h2[nxt * D + j] = h;
            float* gr = a.gates1_dev + row * D4 + j;
            gr[0] = ig; gr[D] = fg; gr[2 * D] = gg; gr[3 * D] = og;
            a.cells1_dev[row * D + j] = c;
            a.h2_dev[row * D + j] = h;
        }
        __syncthreads();
        cur = nxt;
    }
}

// gradients of one LSTM unit's four pre-activations from d h and the running d c; returns d c of the previous step
__device__ __forceinline__ float gt_gate_grads(const float* gates, int D, float c, float c_prev, float dh, float dc_in, float* out4) {
    const float ig = gates[0], fg = gates[D], gg = gates[2 * D], og = gates[3 * D];
    const float tc = ttsc_tanhf(c);
    const float dc = fmaf(dh * og, 1.f - tc * tc, dc_in);
    out4[0] = dc * gg * ig * (1.f - ig);
    out4[1] = dc * c_prev * fg * (1.f - fg);
    out4[2] = dc * ig * (1.f - gg * gg);
    out4[3] = dh * tc * og * (1.f - og);
    return dc * fg;
}

__global__ __launch_bounds__(GT_THREADS) void g2p_train_bwd_kernel(const GtLaunch p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ttsc_g2p_train_args& a = p.a;
    const int E = a.E, A = a.A, D = a.D, N = a.N, T = a.T, D4 = 4 * a.D, R = a.T + 1;
    const int tid = threadIdx.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    float* dg1 = sm;              // [4D] layer 1's gate gradients of this step
    float* dg0 = dg1 + D4;        // [4D]
    float* dh1c = dg0 + D4;       // [D]  d h1 carried from step t + 1 (through W_hh0^T)
    float* dh2c = dh1c + D;       // [D]
    float* dc1 = dh2c + D;        // [D]
    float* dc2 = dc1 + D;         // [D]  (takes the attention query's gradient)
    float* dctx = dc2 + D;        // [E]
    float* dq = dctx + E;         // [A]
    const float* enc = a.enc_dev + (size_t)b * N * E;
    const float* pe = a.pe_dev + (size_t)b * N * A;
    float* denc = a.denc_dev + (size_t)b * N * E;
    float* dpe = a.dpe_dev + (size_t)b * N * A;
    float* dv = a.dv_dev + (size_t)b * A;
    float* da = a.scratch_dev + (size_t)b * 2 * N;     // d a_i = d ctx . enc_i

    for (int j = tid; j < D; j += GT_THREADS) dh1c[j] = dh2c[j] = dc1[j] = dc2[j] = 0.f;
    for (int i = tid; i < N * E; i += GT_THREADS) denc[i] = 0.f;
    for (int i = tid; i < N * A; i += GT_THREADS) dpe[i] = 0.f;
    for (int j = tid; j < A; j += GT_THREADS) dv[j] = 0.f;
    __syncthreads();

    for (int r = T; r >= 0; --r) {
        const size_t row = (size_t)b * R + r;
        // ---- layer 1: gate gradients from d h2 (the output layer's + the next step's recurrence) and d c2 ----
        for (int j = tid; j < D; j += GT_THREADS) {
            const float dh = dh2c[j] + (r > 0 ? a.dh2_dev[((size_t)b * T + (r - 1)) * D + j] : 0.f);
            const float cp = r > 0 ? a.cells1_dev[(row - 1) * D + j] : 0.f;
            float g4[4];
            dc2[j] = gt_gate_grads(a.gates1_dev + row * D4 + j, D, a.cells1_dev[row * D + j], cp, dh, dc2[j], g4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                dg1[g * D + j] = g4[g];
                a.dgates1_dev[row * D4 + g * D + j] = g4[g];
            }
        }
        __syncthreads();
        // ---- [W_ih1^T; W_hh1^T] . dg1 -> d h1 (through the inter-layer mask) and the carried d h2; then layer 0's gate gradients ----
        for (int k = tid; k < D; k += GT_THREADS) {
            float acc[1][2] = {{0.f, 0.f}};
            gt_chain<2>(acc, a.w_l1t, 2 * D, D, k, dg1, D4);
            dh2c[k] = acc[0][1];
            const float keep = gt_keep(a.dec_mask_dev, row * D + k, (uint32_t)k, (uint32_t)r, (uint32_t)b, GT_TAG_DEC + (uint32_t)a.stream_id, a.seed,
                                       a.p_dec, p.s_dec);
            const float dh = fmaf(keep, acc[0][0], dh1c[k]);
            const float cp = r > 0 ? a.cells0_dev[(row - 1) * D + k] : 0.f;
            float g4[4];
            dc1[k] = gt_gate_grads(a.gates0_dev + row * D4 + k, D, a.cells0_dev[row * D + k], cp, dh, dc1[k], g4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                dg0[g * D + k] = g4[g];
                a.dgates0_dev[row * D4 + g * D + k] = g4[g];
            }
        }
        __syncthreads();
        if (r == 0) break;       // the start step has a zero input and a zero state: nothing flows further
        const size_t bt = (size_t)b * T + (r - 1);
        // ---- [W_hh0^T; W_ic^T] . dg0 -> the carried d h1 and d ctx ----
        for (int q = tid; q < D + E; q += GT_THREADS) {
            float acc[1][1] = {{0.f}};
            gt_chain<1>(acc, a.w_l0t, D + E, 0, q, dg0, D4);
            if (q < D)
                dh1c[q] = acc[0][0];
            else
                dctx[q - D] = acc[0][0];
        }
        __syncthreads();
        // ---- attention backward: d a_i = d ctx . enc_i (a wave per position); d enc_i += a_i d ctx ----
        const float* at = a.att_dev + bt * N;
        for (int i = wave; i < N; i += GT_NW) {
            float s = 0.f;
            for (int e = lane; e < E; e += 64) s = fmaf(dctx[e], enc[(size_t)i * E + e], s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) da[i] = s;
        }
        for (int i = tid; i < N * E; i += GT_THREADS) denc[i] = fmaf(at[i / E], dctx[i % E], denc[i]);
        __syncthreads();
        // ---- softmax adjoint d s_i = a_i (d a_i - sum_k a_k d a_k); then v, the energy mask and 1 - tanh^2 (energies recomputed);
        //      thread j owns column j of the projection: d pe[:, j], d q_j, d v_j ----
        {
            float dot = 0.f;
            for (int i = lane; i < N; i += 64) dot = fmaf(at[i], da[i], dot);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
            for (int j = tid; j < A; j += GT_THREADS) {
                const float aqj = a.aq_dev[bt * A + j], vj = a.v[j];
                float dqj = 0.f, dvj = 0.f;
                for (int i = 0; i < N; ++i) {
                    const float en = ttsc_tanhf(aqj + pe[(size_t)i * A + j]);
                    const float k = gt_keep(a.att_mask_dev, (bt * N + i) * A + j, (uint32_t)(i * A + j), (uint32_t)r, (uint32_t)b,
                                            GT_TAG_ATT + (uint32_t)a.stream_id, a.seed, a.p_att, p.s_att);
                    const float ds = at[i] * (da[i] - dot);
                    const float dpre = ds * vj * k * (1.f - en * en);
                    dpe[(size_t)i * A + j] += dpre;
                    dqj += dpre;
                    dvj = fmaf(ds * k, en, dvj);
                }
                dq[j] = dqj;
                a.dq_dev[row * A + j] = dqj;
                dv[j] += dvj;
            }
        }
        __syncthreads();
        // ---- W_aq^T . d q into the CELL gradient of step t - 1 (the query is the top layer's cell state) ----
        for (int k = tid; k < D; k += GT_THREADS) {
            float acc[1][1] = {{0.f}};
            gt_chain<1>(acc, a.w_aqt, D, 0, k, dq, A);
            dc2[k] += acc[0][0];
        }
        // (no barrier: dc2[k] belongs to thread k; dq, dctx and da are next written behind the next step's barriers)
    }
}

__global__ __launch_bounds__(256) void dropout_scale_kernel(const float* __restrict__ x, const float* __restrict__ mask, long n, float p, float scale,
                                                            uint64_t seed, uint32_t stream_id, float* __restrict__ y) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float k;
        if (mask) {
            k = mask[i] * scale;
        } else {
            uint32_t r4[4];
            ttsc_philox4x32((uint32_t)(i >> 2), (uint32_t)(i >> 34), stream_id, GT_TAG_DROP, (uint32_t)seed, (uint32_t)(seed >> 32), r4);
            k = ttsc_u01(r4[i & 3]) >= p ? scale : 0.f;
        }
        y[i] = x[i] * k;
    }
}

int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// what both launches check; fills the launch record
int prepare(const ttsc_g2p_train_args* args, const char* who, GtLaunch* out) {
    TTSC_REQUIRE(args, "%s: null argument", who);
    const ttsc_g2p_train_args& a = *args;
    TTSC_REQUIRE(a.B > 0 && a.N > 0 && a.T > 0 && a.L > 0 && a.Em > 0, "%s: bad sizes (B=%d N=%d T=%d L=%d Em=%d)", who, a.B, a.N, a.T, a.L, a.Em);
    TTSC_REQUIRE(a.E > 0 && a.A > 0 && a.D > 0 && a.E % 4 == 0 && a.A % 4 == 0 && a.D % 4 == 0,
                 "%s: encoder width, attention width and decoder size must be positive multiples of 4 (E=%d A=%d D=%d)", who, a.E, a.A, a.D);
    TTSC_REQUIRE((int64_t)a.N * a.A < (1ll << 31) && (int64_t)a.N * a.E < (1ll << 31), "%s: N * A and N * E must stay below 2^31", who);
    TTSC_REQUIRE(a.p_att >= 0.f && a.p_att < 1.f && a.p_dec >= 0.f && a.p_dec < 1.f, "%s: dropout probabilities must lie in [0, 1)", who);
    TTSC_REQUIRE(a.enc_dev && a.pe_dev && a.y_dev && a.v && a.aq_dev && a.att_dev && a.gates0_dev && a.cells0_dev && a.gates1_dev && a.cells1_dev &&
                     a.scratch_dev,
                 "%s: null tensor", who);
    unsigned* st = g2p_status_word();
    TTSC_REQUIRE(st, "%s: cannot allocate the status word", who);
    out->a = a;
    out->status = st;
    out->s_att = 1.0f / (1.0f - a.p_att);
    out->s_dec = 1.0f / (1.0f - a.p_dec);
    return TTSC_OK;
}

}  // namespace

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_g2p_train_forward(const ttsc_g2p_train_args* args, void* stream) {
    GtLaunch p;
    const int rc = prepare(args, "ttsc_g2p_train_forward", &p);
    if (rc != TTSC_OK) return rc;
    const ttsc_g2p_train_args& a = p.a;
    TTSC_REQUIRE(a.w_aq && a.w_ic && a.tab && a.w_hh0 && a.b0 && a.w_ih1 && a.w_hh1 && a.b1 && a.h1_dev && a.h1m_dev && a.h2_dev && a.x0_dev,
                 "ttsc_g2p_train_forward: null tensor");
    TTSC_REQUIRE(al16(a.w_aq) && al16(a.w_ic) && al16(a.w_hh0) && al16(a.w_ih1) && al16(a.w_hh1) && al16(a.pe_dev) && al16(a.v),
                 "ttsc_g2p_train_forward: pe, v and the packed matrices must be 16-byte aligned");
    const int64_t fl = 7 * (int64_t)a.D + a.A + a.E;
    TTSC_REQUIRE(fl * 4 <= GT_MAX_LDS, "ttsc_g2p_train_forward: 7 D + A + E = %lld floats exceed the workgroup's LDS", (long long)fl);
    hipLaunchKernelGGL(g2p_train_fwd_kernel, dim3((unsigned)a.B), dim3(GT_THREADS), (size_t)fl * sizeof(float), (hipStream_t)stream, p);
    return launched("g2p_train_fwd_kernel");
}

extern "C" int ttsc_g2p_train_backward(const ttsc_g2p_train_args* args, void* stream) {
    GtLaunch p;
    const int rc = prepare(args, "ttsc_g2p_train_backward", &p);
    if (rc != TTSC_OK) return rc;
    const ttsc_g2p_train_args& a = p.a;
    TTSC_REQUIRE(a.w_l1t && a.w_l0t && a.w_aqt && a.dh2_dev && a.dgates0_dev && a.dgates1_dev && a.dq_dev && a.denc_dev && a.dpe_dev && a.dv_dev,
                 "ttsc_g2p_train_backward: null tensor");
    TTSC_REQUIRE(al16(a.w_l1t) && al16(a.w_l0t) && al16(a.w_aqt), "ttsc_g2p_train_backward: the packed matrices must be 16-byte aligned");
    const int64_t fl = 12 * (int64_t)a.D + a.E + a.A;
    TTSC_REQUIRE(fl * 4 <= GT_MAX_LDS, "ttsc_g2p_train_backward: 12 D + E + A = %lld floats exceed the workgroup's LDS", (long long)fl);
    hipLaunchKernelGGL(g2p_train_bwd_kernel, dim3((unsigned)a.B), dim3(GT_THREADS), (size_t)fl * sizeof(float), (hipStream_t)stream, p);
    return launched("g2p_train_bwd_kernel");
}

extern "C" int ttsc_dropout_scale(const float* x_dev, int64_t n, float p, const float* mask_dev, uint64_t seed, int32_t stream_id, float* y_dev,
                                  void* stream) {
    TTSC_REQUIRE(x_dev && y_dev, "ttsc_dropout_scale: null argument");
    TTSC_REQUIRE(n > 0 && p >= 0.f && p < 1.f, "ttsc_dropout_scale: bad arguments (n=%lld p=%g)", (long long)n, (double)p);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(n, 256), 2048);
    hipLaunchKernelGGL(dropout_scale_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, x_dev, mask_dev, (long)n, p, 1.0f / (1.0f - p), seed,
                       (uint32_t)stream_id, y_dev);
    return launched("dropout_scale_kernel");
}
