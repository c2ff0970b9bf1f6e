// Autoregressive attention decoder of the word-level G2P (cube/networks/modules.py:208-297 Seq2Seq.forward, 58-88 Attention; eval mode) as ONE
// launch — gfx950.  The reference runs a Python loop: per step an attention (repeat, cat, 1x1 conv, tanh, two bmm, softmax), one step of a 2-layer
// LSTM, a Linear, an arg-max and an embedding lookup, ~15 launches on a batch of a dozen short words.  Here one workgroup owns one word for all
// of its steps (the shape of melar.hip's loop plus what that kernel lacks: attention over encoder states, arg-max feedback, a per-word stop):
//   * two projections do not depend on the recurrence and come hoisted from the caller: pe = enc . W_att[:, D:]^T + b (all positions) and
//     tab = output_emb . W_ih0[:, E:]^T, which turns the fed-back embedding into one row lookup;
//   * the word's encoder rows and projected rows are copied to LDS once when they fit (n <= ~24 at the reference's sizes), else every step reads
//     them from global memory (L2): no n is refused;
//   * weights (3.4 MB fp32 at the reference's sizes) stream from L2 through rnn_chain.hpp's packed 16-byte loads: thread j owns row j of the
//     attention projection, unit j of both LSTM layers (4 gate rows each) and label j of the output; c1 / c2 / h live in LDS (c2 is next step's
//     attention query); 8 workgroup barriers per step, nothing between workgroups — a word's bits do not depend on what else is in the launch.
// Every loop over rows is strided by the workgroup size: sizes come from the tensors (D, E, A multiples of 4).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>

#include "common.hpp"
#include "../../include/ttscube_math.h"
#include "rnn_chain.hpp"

namespace ttsc {

namespace {

constexpr int G2P_THREADS = 256;
constexpr int G2P_MAX_LDS = 64 * 1024;
constexpr unsigned G2P_BAD_TOKEN = 1u, G2P_BAD_LABEL = 2u, G2P_BAD_N = 4u;

struct G2pLaunch {
    ttsc_g2p_args a;
    unsigned* status;
    int ncap;          // a word with n <= ncap keeps enc / pe / scores in LDS
};

__device__ __forceinline__ int r4(int x) { return (x + 3) & ~3; }

__global__ __launch_bounds__(G2P_THREADS) void g2p_decode_kernel(const G2pLaunch p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ttsc_g2p_args& a = p.a;
    const int E = a.E, A = a.A, D = a.D, L = a.L, D4 = 4 * a.D;
    const int tid = threadIdx.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int NW = G2P_THREADS / 64;
    float* h1 = sm;                 // [2][D]
    float* h2 = h1 + 2 * D;         // [2][D]
    float* c1 = h2 + 2 * D;         // [D]
    float* c2 = c1 + D;             // [D]  (the attention query)
    float* aq = c2 + D;             // [A]
    float* ctx = aq + A;            // [E]
    float* lg = ctx + E;            // [L]
    int* last_s = reinterpret_cast<int*>(lg + r4(L));   // [1] (+3 pad): the label fed back, from wave 0 to everybody
    float* res = lg + r4(L) + 4;    // resident rows: enc [n][E], pe [n][A], scores [2][r4(n)]

    int n = a.n_dev ? a.n_dev[b] : a.Nmax;
    if (n < 1 || n > a.Nmax) {
        if (tid == 0) atomicOr(p.status, G2P_BAD_N);
        n = n < 1 ? 1 : a.Nmax;
    }
    const bool resident = n <= p.ncap;
    const float* enc = a.enc_dev + (size_t)b * a.Nmax * E;
    const float* pe = a.pe_dev + (size_t)b * a.Nmax * A;
    float* sc = a.scratch_dev + (size_t)b * a.Nmax;                       // raw scores
    float* at = a.scratch_dev + ((size_t)a.B + b) * a.Nmax;               // attention weights
    if (resident) {
        float* enc_l = res;
        float* pe_l = enc_l + n * E;
        for (int i = tid; i < (n * E) >> 2; i += G2P_THREADS) reinterpret_cast<float4*>(enc_l)[i] = reinterpret_cast<const float4*>(enc)[i];
        for (int i = tid; i < (n * A) >> 2; i += G2P_THREADS) reinterpret_cast<float4*>(pe_l)[i] = reinterpret_cast<const float4*>(pe)[i];
        enc = enc_l;
        pe = pe_l;
        sc = pe_l + n * A;
        at = sc + r4(n);
    }

    // ---- start state: one decoder step on a zero input from a zero state (modules.py:266): gates = biases (layer 1), b + W_ih1 . h1 (layer 2)
    for (int j = tid; j < D; j += G2P_THREADS) {
        const float ig = ttsc_sigmoidf(a.b0[j]), gg = ttsc_tanhf(a.b0[2 * D + j]), og = ttsc_sigmoidf(a.b0[3 * D + j]);
        const float c = ig * gg;
        c1[j] = c;
        h1[j] = og * ttsc_tanhf(c);
        h2[j] = 0.f;
    }
    __syncthreads();
    for (int j = tid; j < D; j += G2P_THREADS) {
        float acc[1][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[0][g] = a.b1[g * D + j];
        lstm_chain<1, 4, 2>(acc, a.w_ih1, D4, D, j, h1, 0, D);
        const float ig = ttsc_sigmoidf(acc[0][0]), gg = ttsc_tanhf(acc[0][2]), og = ttsc_sigmoidf(acc[0][3]);
        const float c = ig * gg;
        c2[j] = c;
        h2[j] = og * ttsc_tanhf(c);
    }
    __syncthreads();

    int nsteps = a.T;
    if (a.stop) {
        const long cap = 10l * n + 1;          // the reference's give-up: index > 10 N after the step
        if (cap < nsteps) nsteps = (int)cap;
    }
    int cur = 0, last = -1, t = 0;             // last < 0: the fed-back embedding is zero
    for (; t < nsteps; ++t) {
        const int nxt = cur ^ 1;
        // ---- attention, query half: aq = W_att[:, :D] . c2 ----
        for (int j = tid; j < A; j += G2P_THREADS) {
            float acc[1][1] = {{0.f}};
            lstm_chain<1, 1, 5>(acc, a.w_aq, A, 0, j, c2, 0, D);
            aq[j] = acc[0][0];
        }
        __syncthreads();
        // ---- scores: sc_n = v . tanh(aq + pe_n); a wave per position, lanes over the projection, butterfly sum (the same bits in every lane) ----
        for (int i = wave; i < n; i += NW) {
            float s = 0.f;
            for (int j = lane; j < A; j += 64) s = fmaf(a.v[j], ttsc_tanhf(aq[j] + pe[(size_t)i * A + j]), s);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) sc[i] = s;
        }
        __syncthreads();
        // ---- softmax over ALL n positions (the reference masks nothing); every wave computes the same max and sum ----
        {
            float mx = -INFINITY;
            for (int i = lane; i < n; i += 64) mx = fmaxf(mx, sc[i]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            float sum = 0.f;
            for (int i = lane; i < n; i += 64) sum += ttsc_expf(sc[i] - mx);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            for (int i = tid; i < n; i += G2P_THREADS) at[i] = ttsc_expf(sc[i] - mx) / sum;
        }
        __syncthreads();
        // ---- context = sum_n a_n enc_n (n ascending) ----
        for (int e = tid; e < E; e += G2P_THREADS) {
            float acc = 0.f;
            for (int i = 0; i < n; ++i) acc = fmaf(at[i], enc[(size_t)i * E + e], acc);
            ctx[e] = acc;
        }
        __syncthreads();
        // ---- LSTM layer 1: gates = b + W_ih0[:, :E] . context + tab[last] + W_hh0 . h1 ----
        for (int j = tid; j < D; j += G2P_THREADS) {
            float acc[1][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[0][g] = a.b0[g * D + j];
            lstm_chain<1, 4, 2>(acc, a.w_ic, D4, D, j, ctx, 0, E);
            if (last >= 0) {
                const float* tr = a.tab + (size_t)last * D4 + j;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[0][g] += tr[g * D];
            }
            lstm_chain<1, 4, 2>(acc, a.w_hh0, D4, D, j, h1 + cur * D, 0, D);
            const float ig = ttsc_sigmoidf(acc[0][0]), fg = ttsc_sigmoidf(acc[0][1]), gg = ttsc_tanhf(acc[0][2]), og = ttsc_sigmoidf(acc[0][3]);
            const float c = fmaf(fg, c1[j], ig * gg);
            c1[j] = c;
            h1[nxt * D + j] = og * ttsc_tanhf(c);
        }
        __syncthreads();
        // ---- LSTM layer 2 ----
        for (int j = tid; j < D; j += G2P_THREADS) {
            float acc[1][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[0][g] = a.b1[g * D + j];
            lstm_chain<1, 4, 2>(acc, a.w_ih1, D4, D, j, h1 + nxt * D, 0, D);
            lstm_chain<1, 4, 2>(acc, a.w_hh1, D4, D, j, h2 + cur * D, 0, D);
            const float ig = ttsc_sigmoidf(acc[0][0]), fg = ttsc_sigmoidf(acc[0][1]), gg = ttsc_tanhf(acc[0][2]), og = ttsc_sigmoidf(acc[0][3]);
            const float c = fmaf(fg, c2[j], ig * gg);
            c2[j] = c;
            h2[nxt * D + j] = og * ttsc_tanhf(c);
        }
        __syncthreads();
        // ---- logits = W_out . h2 + b ----
        for (int l = tid; l < L; l += G2P_THREADS) {
            float acc[1][1] = {{a.b_out[l]}};
            lstm_chain<1, 1, 5>(acc, a.w_out, L, 0, l, h2 + nxt * D, 0, D);
            lg[l] = acc[0][0];
            if (a.logits_dev) a.logits_dev[((size_t)b * a.T + t) * L + l] = acc[0][0];
        }
        __syncthreads();
        // ---- the label of this step: first maximum (torch.argmax's rule; NaN never wins, as ttsc_tag_argmax); fed back unless a teacher label is ----
        if (wave == 0) {
            float best = -INFINITY;
            int best_i = L;
            for (int l = lane; l < L; l += 64) {
                const float v = lg[l];
                if (v > best) {
                    best = v;
                    best_i = l;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(best_i, o, 64);
                if (ov > best || (ov == best && oi < best_i)) {
                    best = ov;
                    best_i = oi;
                }
            }
            if (best_i >= L) best_i = 0;
            if (lane == 0) {
                if (a.idx_dev) a.idx_dev[(size_t)b * a.T + t] = best_i;
                int fb = best_i;
                if (a.gs_dev) {
                    fb = a.gs_dev[(size_t)b * a.T + t];
                    if (fb < 0 || fb >= L) {
                        atomicOr(p.status, G2P_BAD_LABEL);
                        fb = -1;
                    }
                }
                *last_s = fb;
            }
        }
        __syncthreads();
        last = *last_s;
        cur = nxt;
        if (a.stop && last == a.eos) {
            ++t;
            break;
        }
    }
    if (tid == 0 && a.count_dev) a.count_dev[b] = t;
    // steps beyond this word's own are zero
    for (int s = t; s < a.T; ++s) {
        if (a.idx_dev && tid == 0) a.idx_dev[(size_t)b * a.T + s] = 0;
        if (a.logits_dev)
            for (int l = tid; l < L; l += G2P_THREADS) a.logits_dev[((size_t)b * a.T + s) * L + l] = 0.f;
    }
}

// out[r, :] = table[ids[r], :], zeros for an id outside the table
__global__ __launch_bounds__(256) void g2p_embed_kernel(const int* __restrict__ ids, const float* __restrict__ table, long R, int G, int Em,
                                                        float* __restrict__ out, unsigned* __restrict__ status) {
    const long total = R * Em;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / Em;
        const int c = (int)(i - r * Em);
        const int id = ids[r];
        float v = 0.f;
        if (id >= 0 && id < G)
            v = table[(size_t)id * Em + c];
        else
            atomicOr(status, G2P_BAD_TOKEN);
        out[i] = v;
    }
}

// sticky status word of these kernels, one per device (the pattern of phonemizer.hip)
std::mutex g_mu;
std::map<int, unsigned*> g_words;

unsigned* status_word() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_words.find(dev);
    if (it != g_words.end()) return it->second;
    unsigned* w = nullptr;
    if (hipMalloc(&w, sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(w, 0, sizeof(unsigned)) != hipSuccess) return nullptr;
    g_words[dev] = w;
    return w;
}

int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}

inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

}  // namespace

// the same word for the training kernels (g2p_train.hip): one ttsc_g2p_status covers both
unsigned* g2p_status_word() { return status_word(); }

}  // namespace ttsc

using namespace ttsc;

extern "C" int32_t ttsc_g2p_status(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    unsigned* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_words.find(dev);
        if (it == g_words.end()) return 0;
        w = it->second;
    }
    unsigned v = 0;
    if (hipMemcpy(&v, w, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -1;   // synchronises
    if (v && hipMemset(w, 0, sizeof(unsigned)) != hipSuccess) return -1;
    return (int32_t)v;
}

extern "C" int ttsc_g2p_embed(const int32_t* ids_dev, const float* table_dev, int64_t R, int32_t G, int32_t Em, float* out_dev, void* stream) {
    TTSC_REQUIRE(ids_dev && table_dev && out_dev, "ttsc_g2p_embed: null argument");
    TTSC_REQUIRE(R > 0 && G > 0 && Em > 0, "ttsc_g2p_embed: bad sizes (R=%lld G=%d Em=%d)", (long long)R, G, Em);
    unsigned* st = status_word();
    TTSC_REQUIRE(st, "ttsc_g2p_embed: cannot allocate the status word");
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(R * Em, 256), 1024);
    hipLaunchKernelGGL(g2p_embed_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, ids_dev, table_dev, (long)R, G, Em, out_dev, st);
    return launched("g2p_embed_kernel");
}

extern "C" int ttsc_g2p_decode(const ttsc_g2p_args* args, void* stream) {
    TTSC_REQUIRE(args, "ttsc_g2p_decode: null argument");
    const ttsc_g2p_args& a = *args;
    TTSC_REQUIRE(a.enc_dev && a.pe_dev && a.w_aq && a.v && a.w_ic && a.tab && a.w_hh0 && a.b0 && a.w_ih1 && a.w_hh1 && a.b1 && a.w_out && a.b_out &&
                     a.scratch_dev,
                 "ttsc_g2p_decode: null tensor");
    TTSC_REQUIRE(a.B > 0 && a.Nmax > 0 && a.T > 0 && a.L > 0, "ttsc_g2p_decode: bad sizes (B=%d Nmax=%d T=%d L=%d)", a.B, a.Nmax, a.T, a.L);
    TTSC_REQUIRE(a.E > 0 && a.A > 0 && a.D > 0 && a.E % 4 == 0 && a.A % 4 == 0 && a.D % 4 == 0,
                 "ttsc_g2p_decode: encoder width, attention width and decoder size must be positive multiples of 4 (E=%d A=%d D=%d)", a.E, a.A, a.D);
    TTSC_REQUIRE(a.idx_dev || a.count_dev || a.logits_dev, "ttsc_g2p_decode: no output asked for");
    TTSC_REQUIRE((((uintptr_t)a.enc_dev | (uintptr_t)a.pe_dev | (uintptr_t)a.w_aq | (uintptr_t)a.w_ic | (uintptr_t)a.w_hh0 | (uintptr_t)a.w_ih1 |
                   (uintptr_t)a.w_hh1 | (uintptr_t)a.w_out) & 15) == 0,
                 "ttsc_g2p_decode: enc, pe and the packed matrices must be 16-byte aligned");
    const int64_t fixed = 6 * (int64_t)a.D + a.A + a.E + up4(a.L) + 4;             // floats; the + 4: the fed-back label's slot
    TTSC_REQUIRE(fixed * 4 <= G2P_MAX_LDS, "ttsc_g2p_decode: 6 D + A + E + L + 4 = %lld floats exceed the workgroup's LDS", (long long)fixed);
    // largest n whose rows fit next to the fixed part: n (E + A) + 2 * round4(n) floats
    const int64_t room = G2P_MAX_LDS / 4 - fixed;
    int64_t ncap = room / ((int64_t)a.E + a.A + 2);
    while (ncap > 0 && ncap * ((int64_t)a.E + a.A) + 2 * up4(ncap) > room) --ncap;
    ncap = std::min<int64_t>(ncap, a.Nmax);
    if (!a.n_dev && a.Nmax > ncap) ncap = 0;      // every word is Nmax long and none fits: ask for no resident rows (per-word n is known on the device only)
    const size_t lds = (size_t)(fixed + ncap * ((int64_t)a.E + a.A) + 2 * up4(ncap)) * sizeof(float);
    unsigned* st = status_word();
    TTSC_REQUIRE(st, "ttsc_g2p_decode: cannot allocate the status word");
    G2pLaunch p{a, st, (int)ncap};
    hipLaunchKernelGGL(g2p_decode_kernel, dim3((unsigned)a.B), dim3(G2P_THREADS), lds, (hipStream_t)stream, p);
    return launched("g2p_decode_kernel");
}
