// Forced aligner (io_utils/forced_align.py): text to audio, which the DTW of dtw.hip (audio to audio) is not.  tests/forced_align_reference.py is
// the float32 and float64 numpy statement of everything computed here.
//
// fa_viterbi_kernel     one workgroup of 256 threads per utterance, thread = lattice position (up to FA_PPT positions per thread).  The search
//                       is time-synchronous: a recurrence over frames with one barrier per frame, the shape of pitch.hip::pitch_track_kernel.
//                       The emissions (diagonal Gaussians) do not depend on the recurrence: they are formed FA_TILE frames at a time into LDS
//                       ahead of the dependent chain (a model row is loaded once per tile and used for its FA_TILE frames), so that the chain
//                       carries three LDS reads, three compares, one add and one byte store per position and frame.  Back-pointers go to the
//                       workspace as bytes [B][Tmax][Smax] (0 = stay, 1 = from j - 1, 2 = from skip[j]) and are walked back in the same launch
//                       through LDS, a chunk of frames at a time.
// fa_segment_kernel     per (utterance, position) the float64 sums of x and x * x over the position's frames, ascending t.
// fa_reduce_kernel      one wave per model state: the segment sums of its positions are added in ascending (b, position) and the batch total is
//                       added once to the running tables.  No atomics anywhere; the order of every sum is fixed by the definition, not by the
//                       launch geometry.
// VALU + LDS work and one latency chain: nothing here belongs on the matrix pipe.
#include "common.hpp"

#include <cmath>

namespace ttsc {

constexpr int FA_THREADS = 256;
constexpr int FA_PPT = 4;                                  // lattice positions per thread
constexpr int FA_SMAX = FA_THREADS * FA_PPT;               // 1024 positions per utterance
constexpr int FA_DMAX = 63;                                // feature dimensions (lane 63 of the reducing wave carries the count)
constexpr int FA_TILE = 8;                                 // frames of emissions formed ahead of the chain
// LDS of fa_viterbi_kernel: emissions FA_TILE * FA_SMAX floats (32 KiB; the walk back reuses them for back-pointers) + two rows of scores
// (8 KiB) + the tile's feature rows (2 KiB) = 42 KiB of the 64 KiB a workgroup gets without asking for more
constexpr int FA_EM_BYTES = FA_TILE * FA_SMAX * 4;

static inline size_t fa_round16(size_t v) { return (v + 15) / 16 * 16; }

__global__ __launch_bounds__(FA_THREADS) void fa_viterbi_kernel(const float* __restrict__ feat, const int* __restrict__ nframes,
                                                                const int* __restrict__ state, const int* __restrict__ skip,
                                                                const unsigned char* __restrict__ start, const unsigned char* __restrict__ fin,
                                                                const int* __restrict__ npos, const float* __restrict__ mean,
                                                                const float* __restrict__ ivar, const float* __restrict__ cst, long long Tmax,
                                                                int Smax, int D, int M, unsigned char* bp, int* __restrict__ align,
                                                                float* __restrict__ score, int* __restrict__ ok) {
    __shared__ float em[FA_TILE * FA_SMAX];
    __shared__ float v[2][FA_SMAX];
    __shared__ float xs[FA_TILE * FA_DMAX];
    __shared__ int end_pos;
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    long long T = nframes[b];
    T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
    int S = npos[b];
    S = S < 0 ? 0 : (S > Smax ? Smax : S);
    int* al = align + b * Tmax;
    for (long long t = T + tid; t < Tmax; t += FA_THREADS) al[t] = -1;
    if (T == 0 || S == 0) {                                   // (uniform over the workgroup)
        if (tid == 0) {
            score[b] = 0.f;
            ok[b] = 0;
        }
        return;
    }
    const float* x = feat + b * Tmax * D;
    unsigned char* bpb = bp + (size_t)b * (size_t)Tmax * (size_t)Smax;
    const int nper = (S + FA_THREADS - 1) / FA_THREADS;
    // this thread's positions: model row (-1: an id outside the model, the position is closed), extra predecessor, start flag
    int mrow[FA_PPT], sk[FA_PPT];
    bool st[FA_PPT];
    float cj[FA_PPT];
#pragma unroll
    for (int k = 0; k < FA_PPT; ++k) {
        const int j = tid + k * FA_THREADS;
        mrow[k] = -1;
        sk[k] = -1;
        st[k] = false;
        cj[k] = 0.f;
        if (j < S) {
            const int m = state[b * Smax + j], s = skip[b * Smax + j];
            mrow[k] = (m >= 0 && m < M) ? m : -1;
            sk[k] = (s >= 0 && s < j) ? s : -1;
            st[k] = start[b * Smax + j] != 0;
            if (mrow[k] >= 0) cj[k] = cst[mrow[k]];
        }
    }

    for (long long t0 = 0; t0 < T; t0 += FA_TILE) {
        const int nt = T - t0 < FA_TILE ? (int)(T - t0) : FA_TILE;
        for (int e = tid; e < FA_TILE * D; e += FA_THREADS) xs[e] = e < nt * D ? x[t0 * D + e] : 0.f;
        __syncthreads();
        // emissions of the tile: only the thread that owns a position reads them back, so no barrier stands between them and the chain
#pragma unroll
        for (int k = 0; k < FA_PPT; ++k) {
            const int j = tid + k * FA_THREADS;
            if (k < nper && j < S) {
                float acc[FA_TILE];
#pragma unroll
                for (int q = 0; q < FA_TILE; ++q) acc[q] = 0.f;
                if (mrow[k] >= 0) {
                    const float* mp = mean + (size_t)mrow[k] * D;
                    const float* ip = ivar + (size_t)mrow[k] * D;
                    for (int d = 0; d < D; ++d) {
                        const float mu = mp[d], iv = ip[d];
#pragma unroll
                        for (int q = 0; q < FA_TILE; ++q) {
                            const float df = __fsub_rn(xs[q * D + d], mu);
                            acc[q] = __fadd_rn(acc[q], __fmul_rn(__fmul_rn(df, df), iv));
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < FA_TILE; ++q)
                    em[q * FA_SMAX + j] = mrow[k] >= 0 ? __fsub_rn(cj[k], __fmul_rn(0.5f, acc[q])) : -INFINITY;
            }
        }
        for (int q = 0; q < nt; ++q) {
            const long long t = t0 + q;
            const int cur = (int)(t & 1), prv = cur ^ 1;
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < FA_PPT; ++k) {
                    const int j = tid + k * FA_THREADS;
                    if (k < nper && j < S) v[cur][j] = st[k] ? em[q * FA_SMAX + j] : -INFINITY;
                }
            } else {
                unsigned char* row = bpb + (size_t)t * (size_t)Smax;
#pragma unroll
                for (int k = 0; k < FA_PPT; ++k) {
                    const int j = tid + k * FA_THREADS;
                    if (k < nper && j < S) {
                        float best = v[prv][j];               // stay, then j - 1, then skip[j]; strict >: ties stay on the earlier candidate
                        int code = 0;
                        const float left = j > 0 ? v[prv][j - 1] : -INFINITY;
                        const float jump = sk[k] >= 0 ? v[prv][sk[k]] : -INFINITY;
                        if (left > best) {
                            best = left;
                            code = 1;
                        }
                        if (jump > best) {
                            best = jump;
                            code = 2;
                        }
                        v[cur][j] = __fadd_rn(em[q * FA_SMAX + j], best);
                        row[j] = (unsigned char)code;
                    }
                }
            }
            __syncthreads();
        }
    }

    if (tid == 0) {
        const float* vf = v[(int)((T - 1) & 1)];
        float best = -INFINITY;
        int bi = -1;
        for (int j = 0; j < S; ++j)
            if (fin[b * Smax + j] != 0 && vf[j] > best) {     // strict: ties go to the lowest position
                best = vf[j];
                bi = j;
            }
        if (!(best < INFINITY)) bi = -1;                      // (+inf can only come from non-finite input: no finite path)
        end_pos = bi;
        score[b] = bi >= 0 ? best : 0.f;
        ok[b] = bi >= 0 ? 1 : 0;
    }
    __threadfence();                                          // the back-pointers are out before the walk back reads them
    __syncthreads();
    if (end_pos < 0) {                                        // (uniform: read behind a barrier)
        for (long long t = tid; t < T; t += FA_THREADS) al[t] = -1;
        return;
    }
    unsigned char* chunk = reinterpret_cast<unsigned char*>(em);
    const long long CH = FA_EM_BYTES / S;                     // frames of back-pointers per refill, >= FA_TILE * 4
    for (long long c1 = T; c1 > 0; c1 -= CH) {
        const long long c0 = c1 > CH ? c1 - CH : 0;
        const long long r0 = c0 == 0 ? 1 : c0;                // frame 0 has no back-pointers
        for (long long r = r0; r < c1; ++r)
            for (int j = tid; j < S; j += FA_THREADS) chunk[(r - c0) * S + j] = bpb[(size_t)r * (size_t)Smax + j];
        __syncthreads();
        if (tid == 0) {
            int j = end_pos;
            for (long long t = c1 - 1; t >= c0; --t) {
                al[t] = j;
                if (t > 0) {
                    const int code = chunk[(t - c0) * S + j];
                    // (a code can only name a predecessor the recurrence read; the guards hold the walk inside the row whatever the bytes)
                    if (code == 1 && j > 0) j = j - 1;
                    else if (code == 2) {
                        const int s = skip[b * Smax + j];
                        if (s >= 0 && s < j) j = s;
                    }
                }
            }
            end_pos = j;
        }
        __syncthreads();
    }
}

// seg_cnt [B, Smax] int32, seg_sum / seg_sq [B, Smax, D] float64: written for the positions p < npos[b] of utterances with ok[b] != 0
__global__ __launch_bounds__(FA_THREADS) void fa_segment_kernel(const float* __restrict__ feat, const int* __restrict__ nframes,
                                                                const int* __restrict__ align, const int* __restrict__ ok,
                                                                const int* __restrict__ npos, long long Tmax, int Smax, int D,
                                                                double* __restrict__ seg_sum, double* __restrict__ seg_sq,
                                                                int* __restrict__ seg_cnt) {
    __shared__ int lo[FA_SMAX];
    __shared__ int hi[FA_SMAX];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    if (ok[b] == 0) return;
    long long T = nframes[b];
    T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
    int S = npos[b];
    S = S < 0 ? 0 : (S > Smax ? Smax : S);
    const int* al = align + b * Tmax;
    // first and last frame and the number of frames of every position: each thread scans the row for its own positions (the loads are uniform over
    // the wave), so any align row gives a defined result, not only a non-decreasing one
    for (int p = tid; p < S; p += FA_THREADS) {
        int first = 0, last = -1, n = 0;
        for (long long t = 0; t < T; ++t)
            if (al[t] == p) {
                if (n == 0) first = (int)t;
                last = (int)t;
                ++n;
            }
        lo[p] = first;
        hi[p] = last;
        seg_cnt[b * Smax + p] = n;
    }
    __syncthreads();
    const float* x = feat + b * Tmax * D;
    for (int e = tid; e < S * D; e += FA_THREADS) {
        const int p = e / D, d = e - p * D;
        double s = 0.0, q = 0.0;
        for (int t = lo[p]; t <= hi[p]; ++t)
            if (al[t] == p) {
                const double xv = (double)x[(size_t)t * D + d];
                s = __dadd_rn(s, xv);
                q = __dadd_rn(q, __dmul_rn(xv, xv));
            }
        seg_sum[((size_t)b * Smax + p) * D + d] = s;
        seg_sq[((size_t)b * Smax + p) * D + d] = q;
    }
}

// one wave per model state m: lanes scan 64 (b, position) slots at a time, the matches are taken in ascending order; lane d < D carries column d
// of sum and sumsq, lane 63 the count
__global__ __launch_bounds__(64) void fa_reduce_kernel(const int* __restrict__ state, const int* __restrict__ npos, const int* __restrict__ ok,
                                                       const double* __restrict__ seg_sum, const double* __restrict__ seg_sq,
                                                       const int* __restrict__ seg_cnt, int B, int Smax, int D, double* __restrict__ count,
                                                       double* __restrict__ sum, double* __restrict__ sumsq) {
    const int lane = threadIdx.x, m = blockIdx.x;
    const long long slots = (long long)B * Smax;
    double s = 0.0, q = 0.0, c = 0.0;
    for (long long base = 0; base < slots; base += 64) {
        const long long i = base + lane;
        bool hit = false;
        if (i < slots) {
            const long long b = i / Smax;
            const int p = (int)(i - b * Smax);
            int S = npos[b];
            S = S > Smax ? Smax : S;
            if (ok[b] != 0 && p < S && state[i] == m) hit = seg_cnt[i] > 0;
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int w = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const long long i2 = base + w;
            if (lane < D) {
                s = __dadd_rn(s, seg_sum[(size_t)i2 * D + lane]);
                q = __dadd_rn(q, seg_sq[(size_t)i2 * D + lane]);
            } else if (lane == 63) {
                c = __dadd_rn(c, (double)seg_cnt[i2]);
            }
        }
    }
    if (lane < D) {
        sum[(size_t)m * D + lane] = __dadd_rn(sum[(size_t)m * D + lane], s);
        sumsq[(size_t)m * D + lane] = __dadd_rn(sumsq[(size_t)m * D + lane], q);
    } else if (lane == 63) {
        count[m] = __dadd_rn(count[m], c);
    }
}

}  // namespace ttsc

using namespace ttsc;

extern "C" size_t ttsc_fa_workspace_bytes(int32_t B, int64_t Tmax, int32_t Smax) {
    if (B <= 0 || Tmax <= 0 || Smax <= 0) return 0;
    return fa_round16((size_t)B * (size_t)Tmax * (size_t)Smax);
}

extern "C" int ttsc_fa_check_lattice(const int32_t* state, const int32_t* skip, const uint8_t* start, const uint8_t* final_, const int32_t* npos,
                                     int32_t B, int32_t Smax, int32_t M) {
    TTSC_REQUIRE(B >= 0 && Smax >= 0 && Smax <= FA_SMAX && M >= 0, "ttsc_fa_check_lattice: bad sizes (B=%d Smax=%d M=%d; Smax must be 0 .. %d)", B,
                 Smax, M, FA_SMAX);
    if (B == 0) return TTSC_OK;
    TTSC_REQUIRE(npos && ((state && skip && start && final_) || Smax == 0), "ttsc_fa_check_lattice: null table with B=%d Smax=%d", B, Smax);
    for (int64_t b = 0; b < B; ++b) {
        TTSC_REQUIRE(npos[b] >= 0 && npos[b] <= Smax, "ttsc_fa_check_lattice: npos[%lld] = %d outside 0 .. %d", (long long)b, npos[b], Smax);
        for (int32_t j = 0; j < npos[b]; ++j) {
            const int64_t i = b * Smax + j;
            TTSC_REQUIRE(state[i] >= 0 && state[i] < M, "ttsc_fa_check_lattice: state[%lld, %d] = %d outside 0 .. %d", (long long)b, j, state[i],
                         M - 1);
            TTSC_REQUIRE(skip[i] >= -1 && skip[i] < j, "ttsc_fa_check_lattice: skip[%lld, %d] = %d is neither -1 nor an earlier position",
                         (long long)b, j, skip[i]);
            TTSC_REQUIRE(start[i] <= 1 && final_[i] <= 1, "ttsc_fa_check_lattice: start / final [%lld, %d] = %d / %d are not flags", (long long)b, j,
                         (int)start[i], (int)final_[i]);
        }
    }
    return TTSC_OK;
}

extern "C" int ttsc_fa_viterbi(const float* feat_dev, const int32_t* nframes_dev, const int32_t* state_dev, const int32_t* skip_dev,
                               const uint8_t* start_dev, const uint8_t* final_dev, const int32_t* npos_dev, const float* mean_dev,
                               const float* ivar_dev, const float* cst_dev, int32_t B, int64_t Tmax, int32_t Smax, int32_t D, int32_t M,
                               void* workspace_dev, size_t workspace_bytes, int32_t* align_dev, float* score_dev, int32_t* ok_dev, void* stream) {
    TTSC_REQUIRE(B >= 0 && Tmax >= 0 && Tmax < (int64_t)1 << 30 && Smax >= 0 && Smax <= FA_SMAX && D >= 1 && D <= FA_DMAX && M >= 0,
                 "ttsc_fa_viterbi: bad sizes (B=%d Tmax=%lld Smax=%d D=%d M=%d; Smax must be 0 .. %d, D 1 .. %d)", B, (long long)Tmax, Smax, D, M,
                 FA_SMAX, FA_DMAX);
    if (B == 0) return TTSC_OK;
    TTSC_REQUIRE(nframes_dev && npos_dev && score_dev && ok_dev, "ttsc_fa_viterbi: null nframes / npos / score / ok with B=%d", B);
    TTSC_REQUIRE((feat_dev && align_dev) || Tmax == 0, "ttsc_fa_viterbi: null feat / align with Tmax=%lld", (long long)Tmax);
    TTSC_REQUIRE((state_dev && skip_dev && start_dev && final_dev) || Smax == 0, "ttsc_fa_viterbi: null lattice table with Smax=%d", Smax);
    TTSC_REQUIRE((mean_dev && ivar_dev && cst_dev) || M == 0, "ttsc_fa_viterbi: null model table with M=%d", M);
    const size_t need = ttsc_fa_workspace_bytes(B, Tmax, Smax);
    TTSC_REQUIRE(workspace_bytes >= need && (workspace_dev || need == 0), "ttsc_fa_viterbi: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    TTSC_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "ttsc_fa_viterbi: the workspace must be 16-byte aligned");
    hipLaunchKernelGGL(fa_viterbi_kernel, dim3((unsigned)B), dim3(FA_THREADS), 0, (hipStream_t)stream, feat_dev, nframes_dev, state_dev, skip_dev,
                       start_dev, final_dev, npos_dev, mean_dev, ivar_dev, cst_dev, (long long)Tmax, (int)Smax, (int)D, (int)M,
                       (unsigned char*)workspace_dev, align_dev, score_dev, ok_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("fa_viterbi_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}

extern "C" size_t ttsc_fa_accumulate_workspace_bytes(int32_t B, int32_t Smax, int32_t D) {
    if (B <= 0 || Smax <= 0 || D <= 0) return 0;
    const size_t slots = (size_t)B * (size_t)Smax;
    return fa_round16(2 * slots * (size_t)D * sizeof(double) + slots * sizeof(int32_t));
}

extern "C" int ttsc_fa_accumulate(const float* feat_dev, const int32_t* nframes_dev, const int32_t* align_dev, const int32_t* ok_dev,
                                  const int32_t* state_dev, const int32_t* npos_dev, int32_t B, int64_t Tmax, int32_t Smax, int32_t D, int32_t M,
                                  void* workspace_dev, size_t workspace_bytes, double* count_dev, double* sum_dev, double* sumsq_dev,
                                  void* stream) {
    TTSC_REQUIRE(B >= 0 && Tmax >= 0 && Tmax < (int64_t)1 << 30 && Smax >= 0 && Smax <= FA_SMAX && D >= 1 && D <= FA_DMAX && M >= 0,
                 "ttsc_fa_accumulate: bad sizes (B=%d Tmax=%lld Smax=%d D=%d M=%d; Smax must be 0 .. %d, D 1 .. %d)", B, (long long)Tmax, Smax, D,
                 M, FA_SMAX, FA_DMAX);
    if (B == 0 || M == 0 || Smax == 0 || Tmax == 0) return TTSC_OK;
    TTSC_REQUIRE(feat_dev && nframes_dev && align_dev && ok_dev && state_dev && npos_dev && count_dev && sum_dev && sumsq_dev,
                 "ttsc_fa_accumulate: null argument");
    const size_t need = ttsc_fa_accumulate_workspace_bytes(B, Smax, D);
    TTSC_REQUIRE(workspace_bytes >= need && workspace_dev, "ttsc_fa_accumulate: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    TTSC_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "ttsc_fa_accumulate: the workspace must be 16-byte aligned");
    const size_t slots = (size_t)B * (size_t)Smax;
    double* seg_sum = reinterpret_cast<double*>(workspace_dev);
    double* seg_sq = seg_sum + slots * D;
    int* seg_cnt = reinterpret_cast<int*>(seg_sq + slots * D);
    hipLaunchKernelGGL(fa_segment_kernel, dim3((unsigned)B), dim3(FA_THREADS), 0, (hipStream_t)stream, feat_dev, nframes_dev, align_dev, ok_dev,
                       npos_dev, (long long)Tmax, (int)Smax, (int)D, seg_sum, seg_sq, seg_cnt);
    hipLaunchKernelGGL(fa_reduce_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, state_dev, npos_dev, ok_dev, seg_sum, seg_sq, seg_cnt,
                       (int)B, (int)Smax, (int)D, count_dev, sum_dev, sumsq_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("fa_segment_kernel / fa_reduce_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
