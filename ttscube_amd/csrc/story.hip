// Timeline mixer of StoryCube (ttscube_amd/story.py; io_utils/story_mix.py): the narrated track of cube/story.py:16-52 in one launch.  Timeline
// sample t is
//
//     s = trunc(fl32(w 32767))                      where t lies in a segment (w: the generator's float32 sample), else 0
//     out[t] = int16(trunc(fl32(fl32(fl32(music[t % M] gain) scale) + s)))
//
// which is what the reference's per-sample Python loop computes with np.float32 scalars (tests/story_reference.py::mix_literal): three float32
// operations, each rounded on its own, and a cast that truncates toward zero.  s is an integer of magnitude <= 32767, so keeping it as a float is
// exact.  The products and the sum use __fmul_rn / __fadd_rn: they are never contracted into a fused multiply-add, whatever -ffp-contract says
// (a fused second product changes about 1 sample in 6 500 after truncation).  Where the sum leaves the int16 range the reference's cast is
// undefined; here the sample saturates to [-32768, 32767] (a NaN gives -32768) and is counted.
//
// Memory-bound: per sample 4 B of music (the loop is re-read from cache), 4 B of speech inside a segment, 2 B written.  Each thread owns a run
// of STORY_RUN = 8 consecutive samples and writes it as one 16-byte store (sample by sample at the end of the range, or when `out` is not 16-byte
// aligned).  The segment table is sorted and non-overlapping, so the ends are non-decreasing too: a workgroup finds the first segment that ends
// behind its first sample and the first that ends behind its last sample (two uniform binary searches), a thread searches between the two
// only when they differ, and steps to the next segment where a boundary falls inside its run.  The music phase is one t % M per workgroup and
// one 32-bit (M < 2^31) or 64-bit remainder per thread, then increment-and-wrap: M may be smaller than the run.  All other index arithmetic is
// 64-bit.  The saturation count is an integer: wave shuffles, LDS across the waves, one 64-bit integer atomic per workgroup that saw any.
#include "common.hpp"

namespace ttsc {

constexpr int STORY_RUN = 8;              // samples per thread = one 16-byte store
constexpr int STORY_THREADS = 256;
constexpr int STORY_TILE = STORY_RUN * STORY_THREADS;

typedef short story_short8 __attribute__((ext_vector_type(8)));

// first p in [lo, P) with seg_dst[p] + seg_len[p] > t (P when there is none)
__device__ __forceinline__ int story_first_open(const long long* __restrict__ dst, const long long* __restrict__ len, int lo, int hi, long long t) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (dst[mid] + len[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

template <bool VEC>
__global__ __launch_bounds__(STORY_THREADS) void story_mix_kernel(const float* __restrict__ speech, const long long* __restrict__ seg_src,
                                                                  const long long* __restrict__ seg_len, const long long* __restrict__ seg_dst, int P,
                                                                  const float* __restrict__ music, long long M, float gain, float scale, long long t0,
                                                                  long long n, short* __restrict__ out, unsigned long long* __restrict__ clipped) {
    __shared__ unsigned wave_count[STORY_THREADS / 64];
    const int tid = threadIdx.x;
    const long long jb = (long long)blockIdx.x * STORY_TILE;           // this workgroup's first output sample (jb < n: the grid is ceil(n / TILE))
    const long long j0 = jb + (long long)tid * STORY_RUN;              // this thread's
    const long long tb = t0 + jb, t_first = t0 + j0;
    const long long left = n - j0;                                     // samples of the run inside the range (<= 0: none)
    const int cnt = left >= STORY_RUN ? STORY_RUN : (left > 0 ? (int)left : 0);

    // segment: p = first segment that ends behind t_first
    const long long tb_last = tb + (STORY_TILE - 1) < t0 + n - 1 ? tb + (STORY_TILE - 1) : t0 + n - 1;
    const int pb = story_first_open(seg_dst, seg_len, 0, P, tb);       // (uniform)
    const int pe = story_first_open(seg_dst, seg_len, pb, P, tb_last); // (uniform)
    int p = pb == pe ? pb : story_first_open(seg_dst, seg_len, pb, pe, t_first);
    long long d = 0, e = 0, sidx = 0;                                  // current segment: [d, e) on the timeline, sidx = seg_src - d
    if (p < P) {
        d = seg_dst[p];
        e = d + seg_len[p];
        sidx = seg_src[p] - d;
    }

    // music phase
    const unsigned long long mb = (unsigned long long)tb % (unsigned long long)M;      // (uniform) < M
    const unsigned long long ahead = mb + (unsigned long long)(tid * STORY_RUN);
    long long m = M < (1ll << 31) ? (long long)((unsigned)ahead % (unsigned)M)         // (mb + 2040 < 2^32)
                                  : (long long)(ahead % (unsigned long long)M);

    story_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned sat = 0;
#pragma unroll
    for (int i = 0; i < STORY_RUN; ++i) {
        if (i < cnt) {
            const long long t = t_first + i;
            while (p < P && e <= t) {                                  // a boundary inside the run (also skips empty segments)
                ++p;
                if (p < P) {
                    d = seg_dst[p];
                    e = d + seg_len[p];
                    sidx = seg_src[p] - d;
                }
            }
            float s = 0.f;
            if (p < P && t >= d) s = truncf(__fmul_rn(speech[sidx + t], 32767.f));
            const float bed = __fmul_rn(__fmul_rn(music[m], gain), scale);
            const float r = truncf(__fadd_rn(bed, s));
            const float c = fminf(fmaxf(r, -32768.f), 32767.f);        // (fmaxf(NaN, x) = x)
            sat += (c != r) ? 1u : 0u;
            v[i] = (short)(int)c;
            if (++m == M) m = 0;
        }
    }
    if (VEC && cnt == STORY_RUN) {
        *reinterpret_cast<story_short8*>(out + j0) = v;               // j0 is a multiple of 8 and `out` 16-byte aligned (host check)
    } else {
#pragma unroll
        for (int i = 0; i < STORY_RUN; ++i)
            if (i < cnt) out[j0 + i] = v[i];
    }

    if (clipped != nullptr) {                                          // (uniform)
        for (int off = 32; off > 0; off >>= 1) sat += __shfl_down(sat, off, 64);
        if ((tid & 63) == 0) wave_count[tid >> 6] = sat;
        __syncthreads();
        if (tid == 0) {
            unsigned total = 0;
            for (int w = 0; w < STORY_THREADS / 64; ++w) total += wave_count[w];
            if (total) atomicAdd(clipped, (unsigned long long)total);
        }
    }
}

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_story_mix(const float* speech_dev, const int64_t* seg_src_dev, const int64_t* seg_len_dev, const int64_t* seg_dst_dev, int32_t P,
                              const float* music_dev, int64_t M, float music_gain, float music_scale, int64_t t0, int64_t n, int16_t* out_dev,
                              int64_t* clipped_dev, void* stream) {
    TTSC_REQUIRE(M >= 1, "ttsc_story_mix: the music loop has M=%lld samples, at least 1 is needed", (long long)M);
    TTSC_REQUIRE(P >= 0 && n >= 0 && t0 >= 0, "ttsc_story_mix: negative size (P=%d n=%lld t0=%lld)", P, (long long)n, (long long)t0);
    TTSC_REQUIRE(t0 <= INT64_MAX - n - STORY_TILE, "ttsc_story_mix: t0=%lld + n=%lld does not fit 64 bits", (long long)t0, (long long)n);
    TTSC_REQUIRE(music_dev != nullptr, "ttsc_story_mix: music_dev is NULL");
    TTSC_REQUIRE(P == 0 || (speech_dev && seg_src_dev && seg_len_dev && seg_dst_dev), "ttsc_story_mix: P=%d segments, but a NULL speech or segment table", P);
    TTSC_REQUIRE(n == 0 || out_dev != nullptr, "ttsc_story_mix: out_dev is NULL for n=%lld", (long long)n);
    TTSC_REQUIRE(((uintptr_t)out_dev & 1) == 0 && ((uintptr_t)clipped_dev & 7) == 0, "ttsc_story_mix: out_dev / clipped_dev are not aligned to their type");
    if (n == 0) return TTSC_OK;
    const int64_t tiles = ceil_div(n, STORY_TILE);
    TTSC_REQUIRE(tiles < (int64_t)1 << 31, "ttsc_story_mix: n=%lld needs too many workgroups; mix the timeline in ranges (t0, n)", (long long)n);
    const dim3 grid((unsigned)tiles), block(STORY_THREADS);
    const bool vec = ((uintptr_t)out_dev & 15) == 0;
#define TTSC_STORY_LAUNCH(VEC)                                                                                                                       \
    hipLaunchKernelGGL((story_mix_kernel<VEC>), grid, block, 0, (hipStream_t)stream, speech_dev, (const long long*)seg_src_dev,                     \
                       (const long long*)seg_len_dev, (const long long*)seg_dst_dev, (int)P, music_dev, (long long)M, music_gain, music_scale,      \
                       (long long)t0, (long long)n, (short*)out_dev, (unsigned long long*)clipped_dev)
    if (vec)
        TTSC_STORY_LAUNCH(true);
    else
        TTSC_STORY_LAUNCH(false);
#undef TTSC_STORY_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("story_mix_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
