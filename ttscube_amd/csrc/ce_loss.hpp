// Cross-entropy with ignore_index over logits [R, K] — the stage shared by ttsc_textcoder_loss (textcoder_train.hip) and ttsc_masked_ce
// (phonemizer.hip): one wave per row, loss of the row in a double accumulator, gradient row (softmax - onehot) / count written in the same walk.
// A target outside [0, K) that is not `ignore` contributes nothing, gets a zero gradient row and ORs `bad_bit` into *status.  Workgroups of
// TC_THREADS threads; every reduction is a fixed shuffle / LDS tree.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace ttsc {

namespace {

constexpr int TC_THREADS = 256;

__device__ __forceinline__ double tc_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

__device__ double count_valid(const int64_t* t, int R, int K, long ignore, double* red) {
    double c = 0.0;
    for (int r = threadIdx.x; r < R; r += TC_THREADS) {
        const int64_t v = t[r];
        c += (v != ignore && v >= 0 && v < K) ? 1.0 : 0.0;
    }
    return tc_block_sum(c, red);
}

// one wave per row: loss of the row (lane 0's value) and the gradient row (softmax - onehot) / count
__device__ double ce_rows(const float* L, const int64_t* T, float* G, int R, int K, long ignore, int blk, int nblk, float inv_count,
                          int* status, int bad_bit) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int r = blk * 4 + wave; r < R; r += nblk * 4) {
        const int64_t t = T[r];
        const float* x = L + (size_t)r * K;
        float* g = G + (size_t)r * K;
        const bool valid = t != ignore && t >= 0 && t < K;
        if (!valid) {
            if (t != ignore && lane == 0) atomicOr(status, bad_bit);
            for (int k = lane; k < K; k += 64) g[k] = 0.f;
            continue;
        }
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, x[k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += expf(x[k] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float lse = m + logf(s);
        for (int k = lane; k < K; k += 64) g[k] = (expf(x[k] - lse) - (k == (int)t ? 1.f : 0.f)) * inv_count;
        if (lane == 0) acc += (double)(lse - x[t]);
    }
    return acc;   // (lane 0 of each wave holds its rows' sum; the other lanes 0)
}

}  // namespace

}  // namespace ttsc
