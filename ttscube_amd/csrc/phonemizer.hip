// Kernels of the sentence phonemizer (cube/networks/phonemizer.py:12-103: CubenetPhonemizer, the character tagger in front of every synthesis
// call) — gfx950.  The tagger's middle runs on the existing convolution / LSTM / GEMM kernels; new here are its two ends and its training loss:
//
//   ttsc_char_features   x_char / x_case [B, N] -> [B, Ec + Es, N] in the channel-major layout the convolution kernels read: the two embedding
//                        gathers, the concat, the permute and the length mask of the reference's graph in ONE launch.  It only moves values.
//   ttsc_tag_argmax      rows [M, K] . W[P, K]^T + b -> the index of the first maximum per row (torch.argmax's rule), 0 for padding rows; the
//                        logits go to HBM only when asked for.
//   ttsc_masked_ce       mean cross-entropy over the rows whose target is not ignore_index, and dlogits / count (ce_loss.hpp, shared with
//                        ttsc_textcoder_loss); partial sums per workgroup are added in a fixed order by the last workgroup (ticket).
//
// Tagging head — where the weights live.  W is P x K floats (81 x 400 x 4 B = 130 KB for the reference's model).  Holding all of it in LDS would
// take most of a CU's 160 KiB, leave the CU one workgroup and still need a chunked walk for larger P; and a B = 1 sentence has 30-400 rows, so
// a handful of workgroups would each fill 130 KB of LDS to use it a few times.  Instead W streams from L2 (it is re-read by every workgroup and
// stays resident: 130 KB against 4 MB per XCD) and LDS holds what IS reused inside a workgroup: the TAG_ROWS x K tile of input rows, read by all
// lanes at the same address (broadcast), and the TAG_ROWS x P logits for the arg-max.  Thread p of a workgroup owns class p: it walks W[p, :] once
// in 16-byte loads and feeds TAG_ROWS accumulators, k = 0 .. K-1 in order, one fmaf each — the same chain for every (row, class) whatever M, B
// or the row's place in a tile, so a sentence gets the same bits alone and inside a batch.  P is a run-time value (classes beyond the
// workgroup's width take further passes).
//
// An id outside its table (ttsc_char_features) or a target outside [0, K) that is not ignore_index (ttsc_masked_ce) sets a bit of a sticky
// per-device status word, read and cleared by ttsc_phonemizer_status (the pattern of ttsc_gemm_split_status); there is no device assert.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>

#include "common.hpp"
#include "ce_loss.hpp"

namespace ttsc {

namespace {

constexpr int TAG_ROWS = 4;        // input rows per workgroup
constexpr int TAG_THREADS = 128;   // classes per pass
constexpr int TAG_MAX_LDS = 64 * 1024;

// out[b, c, n] = (c < Ec ? char_tab[x_char[b, n], c] : case_tab[x_case[b, n], c - Ec]) for n < len[b], else 0
__global__ __launch_bounds__(256) void char_features_kernel(const int* __restrict__ x_char, const int* __restrict__ x_case,
                                                            const float* __restrict__ char_tab, const float* __restrict__ case_tab,
                                                            const int* __restrict__ len, int N, int G, int Ec, int Gc, int Es,
                                                            float* __restrict__ out, unsigned* __restrict__ status) {
    const int b = blockIdx.y;
    const int C = Ec + Es;
    const int n_valid = len ? (len[b] < N ? len[b] : N) : N;
    const long total = (long)C * N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i / N), n = (int)(i - (long)c * N);
        float v = 0.f;
        if (n < n_valid) {
            const bool is_char = c < Ec;
            const int id = is_char ? x_char[(size_t)b * N + n] : x_case[(size_t)b * N + n];
            const int rows = is_char ? G : Gc;
            if (id >= 0 && id < rows)
                v = is_char ? char_tab[(size_t)id * Ec + c] : case_tab[(size_t)id * Es + (c - Ec)];
            else
                atomicOr(status, 1u);
        }
        out[(size_t)b * total + i] = v;
    }
}

struct TagArgs {
    const float* x;      // [M, K] rows at stride ldx
    const float* w;      // [P, K]
    const float* bias;   // [P] or null
    const int* len;      // [M / period] or null
    int* tags;           // [M]
    float* logits;       // [M, P] or null
    int M, P, K, ldx, period;
};

__global__ __launch_bounds__(TAG_THREADS) void tag_argmax_kernel(const TagArgs a) {
    extern __shared__ float lds[];
    float* xs = lds;                          // [TAG_ROWS][K]
    float* ls = lds + TAG_ROWS * a.K;         // [TAG_ROWS][P]
    __shared__ int valid[TAG_ROWS];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * TAG_ROWS;
    if (tid < TAG_ROWS) {
        const int r = r0 + tid;
        int ok = r < a.M;
        if (ok && a.len) ok = (r % a.period) < a.len[r / a.period];
        valid[tid] = ok;
    }
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int r = 0; r < TAG_ROWS; ++r) any = any || valid[r];
    if (any) {
        const int K4 = a.K >> 2;
        // padding rows hold whatever the recurrence left there (possibly nothing): they enter the tile as zeros
        for (int i = tid; i < TAG_ROWS * K4; i += TAG_THREADS) {
            const int r = i / K4, k4 = i - r * K4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[r]) v = *reinterpret_cast<const float4*>(a.x + (size_t)(r0 + r) * a.ldx + 4 * k4);
            reinterpret_cast<float4*>(xs)[i] = v;
        }
        __syncthreads();
        for (int p = tid; p < a.P; p += TAG_THREADS) {
            const float4* wp = reinterpret_cast<const float4*>(a.w + (size_t)p * a.K);
            const float b0 = a.bias ? a.bias[p] : 0.f;
            float acc[TAG_ROWS];
#pragma unroll
            for (int r = 0; r < TAG_ROWS; ++r) acc[r] = 0.f;
            for (int k4 = 0; k4 < K4; ++k4) {
                const float4 w = wp[k4];
#pragma unroll
                for (int r = 0; r < TAG_ROWS; ++r) {
                    const float4 x = reinterpret_cast<const float4*>(xs + r * a.K)[k4];
                    acc[r] = fmaf(x.x, w.x, acc[r]);
                    acc[r] = fmaf(x.y, w.y, acc[r]);
                    acc[r] = fmaf(x.z, w.z, acc[r]);
                    acc[r] = fmaf(x.w, w.w, acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < TAG_ROWS; ++r) ls[r * a.P + p] = acc[r] + b0;
        }
        __syncthreads();
    }
    // arg-max: wave w takes rows w, w + 2; a lane walks p = lane, lane + 64, .. upwards (strict >: its first maximum), the lanes then
    // merge pairwise — the larger value wins, equal values keep the lower index; NaN never wins (as ttsc_align_durations)
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < TAG_ROWS; r += TAG_THREADS / 64) {
        const int row = r0 + r;
        if (row >= a.M) continue;
        int best_i = 0;
        if (valid[r]) {
            float best = -INFINITY;
            best_i = a.P;
            for (int p = lane; p < a.P; p += 64) {
                const float v = ls[r * a.P + p];
                if (v > best) {
                    best = v;
                    best_i = p;
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
            if (best_i >= a.P) best_i = 0;      // (a row of NaNs: no class won)
        }
        if (lane == 0) a.tags[row] = best_i;
        if (a.logits) {
            float* dst = a.logits + (size_t)row * a.P;
            for (int p = lane; p < a.P; p += 64) dst[p] = valid[r] ? ls[r * a.P + p] : 0.f;
        }
    }
}

struct CeArgs {
    const float* logits;   // [R, K]
    const int64_t* target; // [R]
    float* grad;           // [R, K]
    int R, K, nb;
    long ignore;
    double* partial;       // [nb]
    unsigned* ticket;      // workspace word 0
    int* launch_status;    // workspace word 1: this launch's bad-target flag
    float* out;            // [1]
    int* status_out;       // [1] or null: 2 when a target was out of range, else 0
    unsigned* sticky;      // the device's status word
};

__global__ __launch_bounds__(TC_THREADS) void masked_ce_kernel(const CeArgs a) {
    __shared__ double red[TC_THREADS / 64];
    __shared__ bool last;
    const double cnt = count_valid(a.target, a.R, a.K, a.ignore, red);
    double v = ce_rows(a.logits, a.target, a.grad, a.R, a.K, a.ignore, blockIdx.x, a.nb, (float)(1.0 / cnt), a.launch_status, 2);
    v = tc_block_sum(v, red);
    if (threadIdx.x == 0) {
        a.partial[blockIdx.x] = v;
        __threadfence();
        last = atomicAdd(a.ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nb; i += TC_THREADS) s += __hip_atomic_load(a.partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double tot = tc_block_sum(s, red);
    if (threadIdx.x == 0) {
        a.out[0] = cnt > 0.0 ? (float)(tot / cnt) : 0.f;     // (torch's mean over no rows is NaN; the trainer wants a step without targets to be a no-op)
        const int bad = __hip_atomic_load(a.launch_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bad) atomicOr(a.sticky, 2u);
        if (a.status_out) *a.status_out = bad ? 2 : 0;
        *a.ticket = 0u;
    }
}

// sticky status word of these kernels, one per device
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

int ce_blocks(int32_t R) { return (int)std::max<int64_t>(std::min<int64_t>(ceil_div(R, 4), 512), 1); }

}  // namespace

}  // namespace ttsc

using namespace ttsc;

extern "C" int32_t ttsc_phonemizer_status(void) {
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

extern "C" int ttsc_char_features(const int32_t* x_char_dev, const int32_t* x_case_dev, const float* char_table_dev, const float* case_table_dev,
                                  const int32_t* len_dev, int32_t B, int32_t N, int32_t G, int32_t Ec, int32_t Gc, int32_t Es, float* out_dev,
                                  void* stream) {
    TTSC_REQUIRE(x_char_dev && x_case_dev && char_table_dev && case_table_dev && out_dev, "ttsc_char_features: null argument");
    TTSC_REQUIRE(B > 0 && B <= 65535 && N > 0 && G > 0 && Ec > 0 && Gc > 0 && Es > 0, "ttsc_char_features: bad sizes (B=%d N=%d G=%d Ec=%d Gc=%d Es=%d)", B,
                 N, G, Ec, Gc, Es);
    unsigned* st = status_word();
    TTSC_REQUIRE(st, "ttsc_char_features: cannot allocate the status word");
    const int64_t total = (int64_t)(Ec + Es) * N;
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div(total, 256), 1024);
    hipLaunchKernelGGL(char_features_kernel, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x_char_dev, x_case_dev, char_table_dev,
                       case_table_dev, len_dev, N, G, Ec, Gc, Es, out_dev, st);
    return launched("char_features_kernel");
}

extern "C" int ttsc_tag_argmax(const float* x_dev, const float* w_dev, const float* bias_dev, const int32_t* len_dev, int32_t period, int64_t M,
                               int32_t P, int32_t K, int64_t ldx, int32_t* tags_dev, float* logits_dev, void* stream) {
    TTSC_REQUIRE(x_dev && w_dev && tags_dev, "ttsc_tag_argmax: null argument");
    TTSC_REQUIRE(M > 0 && M < (1ll << 31) - TAG_ROWS && P > 0 && K > 0 && K % 4 == 0 && ldx >= K && ldx % 4 == 0 && ldx < (1ll << 31),
                 "ttsc_tag_argmax: bad shape M=%lld P=%d K=%d ldx=%lld (K and ldx must be multiples of 4, ldx >= K)", (long long)M, P, K, (long long)ldx);
    TTSC_REQUIRE(!len_dev || (period > 0 && M % period == 0), "ttsc_tag_argmax: rows must be [utterance][period] when lengths are given");
    TTSC_REQUIRE((((uintptr_t)x_dev | (uintptr_t)w_dev) & 15) == 0, "ttsc_tag_argmax: x and W must be 16-byte aligned");
    const size_t lds = (size_t)TAG_ROWS * ((size_t)K + (size_t)P) * sizeof(float);
    TTSC_REQUIRE(lds <= (size_t)TAG_MAX_LDS, "ttsc_tag_argmax: K + P = %d exceeds %d", K + P, TAG_MAX_LDS / (TAG_ROWS * 4));
    TagArgs a{x_dev, w_dev, bias_dev, len_dev, tags_dev, logits_dev, (int)M, P, K, (int)ldx, period};
    hipLaunchKernelGGL(tag_argmax_kernel, dim3((unsigned)ceil_div(M, TAG_ROWS)), dim3(TAG_THREADS), lds, (hipStream_t)stream, a);
    return launched("tag_argmax_kernel");
}

extern "C" size_t ttsc_masked_ce_workspace_bytes(int32_t R) { return 64 + (size_t)ce_blocks(R) * sizeof(double); }

extern "C" int ttsc_masked_ce(const float* logits_dev, const int64_t* target_dev, int32_t R, int32_t K, int64_t ignore_index, float* loss_dev,
                              float* dlogits_dev, int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    TTSC_REQUIRE(logits_dev && target_dev && loss_dev && dlogits_dev && ws_dev, "ttsc_masked_ce: null argument");
    TTSC_REQUIRE(R > 0 && K > 0, "ttsc_masked_ce: bad sizes (R %d, K %d)", R, K);
    TTSC_REQUIRE(ws_bytes >= ttsc_masked_ce_workspace_bytes(R), "ttsc_masked_ce: workspace too small");
    unsigned* st = status_word();
    TTSC_REQUIRE(st, "ttsc_masked_ce: cannot allocate the status word");
    CeArgs a{};
    a.logits = logits_dev; a.target = target_dev; a.grad = dlogits_dev; a.R = R; a.K = K; a.nb = ce_blocks(R); a.ignore = ignore_index;
    a.ticket = (unsigned*)ws_dev;
    a.launch_status = (int*)ws_dev + 1;
    a.partial = (double*)((char*)ws_dev + 64);
    a.out = loss_dev; a.status_out = status_dev; a.sticky = st;
    hipStream_t s = (hipStream_t)stream;
    TTSC_HIP_CHECK(hipMemsetAsync(ws_dev, 0, 64, s));
    hipLaunchKernelGGL(masked_ce_kernel, dim3((unsigned)a.nb), dim3(TC_THREADS), 0, s, a);
    return launched("masked_ce_kernel");
}
