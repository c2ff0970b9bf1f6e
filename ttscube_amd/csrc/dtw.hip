// Dynamic time warping of the dev-set evaluation (io_utils/evaluate.py): P ragged pairs of feature sequences in one launch; tests/dtw_reference.py
// is the float64 (and float32) statement of what is computed here.  Steps (1,1), (1,0), (0,1), unweighted; local cost sqrt(sum_k (a - b)^2) taken
// from the differences in ascending k; ties to the diagonal, then (i-1, j), then (i, j-1).  VALU + LDS work and one latency chain: nothing here
// belongs on the matrix pipe.
//
// One workgroup of eight waves per pair.  Columns j are taken in blocks of 64, lane = column.
//   waves 1..7  form the local costs of the block 32 rows at a time into a ring of 128 rows in LDS (lane = column, its b vector in LDS at an odd
//               stride; the row of a is wave-uniform).  No Na x Nb cost matrix exists anywhere: the ring is all there is.
//   wave 0      runs the recurrence as a skewed wavefront 32 steps behind them: at step s lane t holds row i = s - t.  D(i-1, j) is the lane's own
//               previous value, D(i, j-1) the left neighbour's (one DPP wave shift), D(i-1, j-1) what that shift gave one step earlier.  Lane 0's
//               left neighbour is the block's boundary column: lane 63 writes D(., j0 + 63) to the workspace, the next block reads it back 32 rows
//               at a time, one hand-over ahead of its use.
// One barrier per 32 steps hands a ring slot over.  Back-pointers go as bytes to the workspace in the skewed order [block][step][lane] (64
// contiguous bytes per step) and are walked back through LDS 512 steps at a time once the last block is done; the reversed path is parked in the
// workspace and turned round by the whole workgroup.
#include "common.hpp"

#include <cmath>

namespace ttsc {

constexpr int DTW_W = 64;                  // columns per block = lanes of the recurrence wave
constexpr int DTW_THREADS = 512;             // wave 0 runs the recurrence, waves 1..7 form local costs
constexpr int DTW_NPROD = DTW_THREADS / 64 - 1;
constexpr int DTW_RC = 32;                 // rows / steps per hand-over
constexpr int DTW_RPW = (DTW_RC + DTW_NPROD - 1) / DTW_NPROD;   // rows per producing wave and hand-over
constexpr int DTW_RING = 128;              // rows of local costs in LDS: the 32 being written + the 95 a skewed chunk of steps can touch
constexpr int DTW_KMAX = 80;
constexpr int DTW_KS = DTW_KMAX + 1;       // odd row stride of the b block in LDS: 32 lanes, 32 banks
constexpr int DTW_WALK = DTW_RING * DTW_W * 4 / DTW_W;   // steps of back-pointers per LDS refill of the walk back (the ring's bytes)

static inline size_t dtw_round16(size_t v) { return (v + 15) / 16 * 16; }
static inline size_t dtw_bp_bytes(int64_t Na, int64_t Nb) { return (size_t)ceil_div(Nb, DTW_W) * (size_t)(Na + DTW_W - 1) * DTW_W; }
static inline size_t dtw_bnd_bytes(int64_t Na) { return dtw_round16((size_t)Na * sizeof(float)); }
static inline size_t dtw_path_len(int64_t Na, int64_t Nb) { return Na + Nb > 0 ? (size_t)(Na + Nb - 1) : 0; }
static inline size_t dtw_pair_bytes(int64_t Na, int64_t Nb) {
    return dtw_bp_bytes(Na, Nb) + dtw_bnd_bytes(Na) + dtw_round16(2 * dtw_path_len(Na, Nb) * sizeof(int32_t));
}

// lane t <- lane t - 1, lane 0 <- edge (wave_shr:1; every lane of the wave must be executing)
__device__ __forceinline__ float dtw_shift_up(float v, float edge) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// the boundary column crosses from lane 63 of one block to the loads of the next: device-scope accesses, so no stale L1 line can serve them
__device__ __forceinline__ float dtw_bnd_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dtw_bnd_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(DTW_THREADS) void dtw_align_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const int* __restrict__ len_a, const int* __restrict__ len_b, long long Na,
                                                                long long Nb, int K, unsigned char* ws, long long pair_bytes, long long bp_bytes,
                                                                long long bnd_bytes, float* __restrict__ cost, int* __restrict__ plen,
                                                                int* __restrict__ path_a, int* __restrict__ path_b) {
    __shared__ float ring[DTW_RING * DTW_W];                  // 32 KiB; the walk back reuses it for back-pointers
    __shared__ float bst[DTW_W * DTW_KS];
    __shared__ long long wk_i, wk_j, wk_n;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long p = blockIdx.x;
    const long long Lp = Na + Nb > 0 ? Na + Nb - 1 : 0;
    long long la = len_a[p], lb = len_b[p];
    la = la < 0 ? 0 : (la > Na ? Na : la);
    lb = lb < 0 ? 0 : (lb > Nb ? Nb : lb);
    int* pa = path_a + p * Lp;
    int* pb = path_b + p * Lp;
    if (la == 0 || lb == 0) {                                 // (uniform over the workgroup)
        for (long long q = tid; q < Lp; q += DTW_THREADS) {
            pa[q] = -1;
            pb[q] = -1;
        }
        if (tid == 0) {
            cost[p] = 0.f;
            plen[p] = 0;
        }
        return;
    }
    const float* ap = a + p * Na * K;
    const float* bp = b + p * Nb * K;
    unsigned char* bpw = ws + p * pair_bytes;                  // back-pointers [block][step < Na + 63][lane]
    float* bnd = reinterpret_cast<float*>(bpw + bp_bytes);     // D(i, last column of the previous block)
    int* tmp = reinterpret_cast<int*>(bpw + bp_bytes + bnd_bytes);   // the path, last cell first: i at [n], j at [Lp + n]
    const long long nblk = (lb + DTW_W - 1) / DTW_W, srows = Na + DTW_W - 1;

    for (long long cb = 0; cb < nblk; ++cb) {
        const long long j0 = cb * DTW_W;
        const int ncol = lb - j0 < DTW_W ? (int)(lb - j0) : DTW_W;
        __syncthreads();                                      // the previous block is done with bst[] and ring[]
        for (int e = tid; e < ncol * K; e += DTW_THREADS) {
            const int c = e / K;
            bst[c * DTW_KS + (e - c * K)] = bp[j0 * K + e];
        }
        __syncthreads();
        const long long nsteps = la + ncol - 1, nsc = (nsteps + DTW_RC - 1) / DTW_RC;
        const bool col = lane < ncol, carry = cb > 0, hand_on = cb + 1 < nblk;
        float val = INFINITY;                                 // D of this lane's previous row; +inf above row 0
        float lprev = (cb == 0 && lane == 0) ? 0.f : INFINITY;   // what the shift gave one step ago: D(i-1, j-1); D(-1, -1) = 0 starts the path
        float bnext = INFINITY;                               // boundary rows of the next 32 steps, row s0 + lane in lanes 0..31
        if (wave == 0 && carry && lane < DTW_RC && lane < la) bnext = dtw_bnd_load(bnd + lane);
        for (long long n = 0; n <= nsc; ++n) {
            if (wave != 0) {
                // this wave's rows of the chunk: lanes 0..K-1 fetch a row with one coalesced load (two above K = 64), every k is then a lane read
                const long long r0 = n * DTW_RC + (wave - 1);
                float a0[DTW_RPW], a1[DTW_RPW], acc[DTW_RPW];
#pragma unroll
                for (int m = 0; m < DTW_RPW; ++m) {
                    const long long r = r0 + (long long)m * DTW_NPROD;
                    const bool row = (wave - 1) + m * DTW_NPROD < DTW_RC && r < la;
                    a0[m] = (row && lane < K) ? ap[r * K + lane] : 0.f;
                    a1[m] = (row && lane + 64 < K) ? ap[r * K + lane + 64] : 0.f;
                    acc[m] = 0.f;
                }
                const float* br = bst + lane * DTW_KS;
                const int K0 = K < 64 ? K : 64;
                for (int k = 0; k < K0; ++k) {
                    const float bk = br[k];
#pragma unroll
                    for (int m = 0; m < DTW_RPW; ++m) {
                        const float df = __fsub_rn(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(a0[m]), k)), bk);
                        acc[m] = __fadd_rn(acc[m], __fmul_rn(df, df));
                    }
                }
                for (int k = 64; k < K; ++k) {
                    const float bk = br[k];
#pragma unroll
                    for (int m = 0; m < DTW_RPW; ++m) {
                        const float df = __fsub_rn(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(a1[m]), k - 64)), bk);
                        acc[m] = __fadd_rn(acc[m], __fmul_rn(df, df));
                    }
                }
#pragma unroll
                for (int m = 0; m < DTW_RPW; ++m) {
                    const long long r = r0 + (long long)m * DTW_NPROD;
                    if (col && (wave - 1) + m * DTW_NPROD < DTW_RC && r < la) ring[(int)(r & (DTW_RING - 1)) * DTW_W + lane] = sqrtf(acc[m]);
                }
            } else if (n > 0) {
                const long long s0 = (n - 1) * DTW_RC;
                const int ns = nsteps - s0 < DTW_RC ? (int)(nsteps - s0) : DTW_RC;
                const float bcur = bnext;
                bnext = INFINITY;
                if (carry && lane < DTW_RC && s0 + DTW_RC + lane < la) bnext = dtw_bnd_load(bnd + s0 + DTW_RC + lane);
                // rows relative to s0: lane t holds row s0 + q - t at step q; rows [lo, hi) exist
                const int lo = s0 < DTW_W ? -(int)s0 : -DTW_W, hi = la - s0 < DTW_W ? (int)(la - s0) : DTW_W;
                const int s0m = (int)(s0 & (DTW_RING - 1));
                const int qend = (int)(la - 1 - s0) + lane;      // the step of this chunk at which this lane holds the last row (if any)
                const bool endcol = j0 + lane == lb - 1;
                int rel = -lane;
                float dn = (col && rel >= lo && rel < hi) ? ring[((s0m + rel) & (DTW_RING - 1)) * DTW_W + lane] : 0.f;
                unsigned char* bps = bpw + ((size_t)cb * (size_t)srows + (size_t)s0) * DTW_W + lane;
                for (int q = 0; q < ns; ++q, ++rel) {
                    const bool act = col && rel >= lo && rel < hi;
                    const float d = dn;
                    if (q + 1 < ns) dn = (col && rel + 1 >= lo && rel + 1 < hi) ? ring[((s0m + rel + 1) & (DTW_RING - 1)) * DTW_W + lane] : 0.f;
                    const float left = dtw_shift_up(val, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bcur), q)));
                    float best = lprev;                       // the diagonal first, then (i-1, j), then (i, j-1); strict <
                    int code = 0;
                    if (val < best) {
                        best = val;
                        code = 1;
                    }
                    if (left < best) {
                        best = left;
                        code = 2;
                    }
                    const float nv = __fadd_rn(d, best);
                    lprev = left;
                    val = act ? nv : INFINITY;
                    if (act) {
                        bps[(size_t)q * DTW_W] = (unsigned char)code;
                        if (hand_on && lane == DTW_W - 1) dtw_bnd_store(bnd + s0 + rel, nv);
                        if (endcol && q == qend) cost[p] = nv;
                    }
                }
            }
            __syncthreads();
        }
        __threadfence();                                      // the boundary column and the back-pointers are out before the next block reads
    }

    if (tid == 0) {
        wk_i = la - 1;
        wk_j = lb - 1;
        wk_n = 0;
    }
    __syncthreads();
    const unsigned char* chunk = reinterpret_cast<const unsigned char*>(ring);
    unsigned* chunk32 = reinterpret_cast<unsigned*>(ring);
    for (;;) {
        const long long ci = wk_i, cj = wk_j;
        if (ci < 0) break;                                    // (uniform: read behind a barrier)
        const long long cb = cj / DTW_W, shi = ci + (cj - cb * DTW_W), slo = shi >= DTW_WALK ? shi - (DTW_WALK - 1) : 0;
        const unsigned* src = reinterpret_cast<const unsigned*>(bpw + ((size_t)cb * (size_t)srows + (size_t)slo) * DTW_W);
        const int nw = (int)(shi - slo + 1) * (DTW_W / 4);
        for (int e = tid; e < nw; e += DTW_THREADS) chunk32[e] = src[e];
        __syncthreads();
        if (tid == 0) {
            long long i = ci, j = cj, n = wk_n;
            for (;;) {
                tmp[n] = (int)i;
                tmp[Lp + n] = (int)j;
                ++n;
                if (i == 0 && j == 0) {
                    i = -1;
                    break;
                }
                const long long t = j - cb * DTW_W;
                int code = chunk[(i + t - slo) * DTW_W + t];
                if (i == 0) code = 2;                         // (what the recurrence wrote there anyway; holds the walk inside the table whatever the data)
                else if (j == 0) code = 1;
                if (code != 2) --i;
                if (code != 1) --j;
                if (j < cb * DTW_W || i + (j - cb * DTW_W) < slo) break;
            }
            wk_i = i;
            wk_j = j;
            wk_n = n;
            __threadfence();
        }
        __syncthreads();
    }
    const long long n = wk_n;
    for (long long q = tid; q < Lp; q += DTW_THREADS) {
        pa[q] = q < n ? tmp[n - 1 - q] : -1;
        pb[q] = q < n ? tmp[Lp + n - 1 - q] : -1;
    }
    if (tid == 0) plen[p] = (int)n;
}

}  // namespace ttsc

using namespace ttsc;

extern "C" size_t ttsc_dtw_workspace_bytes(int32_t P, int64_t Na_max, int64_t Nb_max) {
    if (P <= 0 || Na_max <= 0 || Nb_max <= 0) return 0;
    return (size_t)P * dtw_pair_bytes(Na_max, Nb_max);
}

extern "C" int ttsc_dtw_align(const float* a_dev, const float* b_dev, const int32_t* len_a_dev, const int32_t* len_b_dev, int32_t P, int64_t Na_max,
                              int64_t Nb_max, int32_t K, void* workspace_dev, size_t workspace_bytes, float* cost_dev, int32_t* plen_dev,
                              int32_t* path_a_dev, int32_t* path_b_dev, void* stream) {
    TTSC_REQUIRE(P >= 0 && K >= 1 && K <= DTW_KMAX && Na_max >= 0 && Nb_max >= 0 && Na_max < (int64_t)1 << 30 && Nb_max < (int64_t)1 << 30,
                 "ttsc_dtw_align: bad sizes (P=%d Na_max=%lld Nb_max=%lld K=%d; K must be 1 .. %d)", P, (long long)Na_max, (long long)Nb_max, K,
                 DTW_KMAX);
    if (P == 0) return TTSC_OK;
    TTSC_REQUIRE(len_a_dev && len_b_dev && cost_dev && plen_dev, "ttsc_dtw_align: null lengths / cost / plen with P=%d", P);
    TTSC_REQUIRE((a_dev || Na_max == 0) && (b_dev || Nb_max == 0), "ttsc_dtw_align: null sequence pointer with a nonzero size");
    TTSC_REQUIRE((path_a_dev && path_b_dev) || dtw_path_len(Na_max, Nb_max) == 0, "ttsc_dtw_align: null path pointer with a nonzero size");
    const size_t need = ttsc_dtw_workspace_bytes(P, Na_max, Nb_max);
    TTSC_REQUIRE(workspace_bytes >= need && (workspace_dev || need == 0), "ttsc_dtw_align: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    TTSC_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "ttsc_dtw_align: the workspace must be 16-byte aligned");
    hipLaunchKernelGGL(dtw_align_kernel, dim3((unsigned)P), dim3(DTW_THREADS), 0, (hipStream_t)stream, a_dev, b_dev, len_a_dev, len_b_dev,
                       (long long)Na_max, (long long)Nb_max, (int)K, (unsigned char*)workspace_dev, (long long)dtw_pair_bytes(Na_max, Nb_max),
                       (long long)dtw_bp_bytes(Na_max, Nb_max), (long long)dtw_bnd_bytes(Na_max), cost_dev, plen_dev, path_a_dev, path_b_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("dtw_align_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
