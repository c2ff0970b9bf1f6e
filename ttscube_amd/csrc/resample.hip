// Rational-rate polyphase FIR resampler of the audio readers (io_utils/resample.py): what scipy.signal.resample_poly(x, up, down) computes with its
// defaults, for a ragged batch in one launch.  tests/resample_reference.py is the float64 statement:
//
//     y[n] = sum_i x[i] h[n down - i up + half]   over |n down - i up| <= half,   half = 10 max(up, down),   n < ceil(L up / down)
//
// With c = n down + half, i_hi = c / up and p = c % up this is y[n] = sum_{j < K} x[i_hi - j] h[p + j up]: output n walks phase p of the filter
// backwards through the input.  The caller passes h padded with zeros to up * K4 floats, K4 = K rounded up to a multiple of 4, so every output sums
// exactly K4 terms: four running sums over j mod 4, j ascending, combined as (s0 + s1) + (s2 + s3).  That order depends on nothing but the position
// of the output: a row comes out with the same bits alone, in any batch and whatever the tile it falls into.  Samples outside [0, L) read as zero.
//
// One 256-thread workgroup per (row, RESAMPLE_TILE consecutive outputs), one output per thread.  The input span of the tile (at most
// ceil((TILE - 1) down / up) + K4 samples) is staged in LDS when it fits RESAMPLE_X_LDS floats, the padded filter when it fits RESAMPLE_H_LDS floats;
// whatever does not fit is read through L2 by the same loop (a long decimation such as 48 kHz -> 1 kHz: the span of one tile is megabytes).  In
// LDS, lanes of a wave read different phases p + j up at one j: consecutive p lie in consecutive banks.  VALU + LDS work, nothing for the matrix pipe.
// max |y| of a row: a workgroup maximum, then one vector atomic max on the bits of the non-negative float (a maximum does not depend on order).
#include "common.hpp"

namespace ttsc {

constexpr int RESAMPLE_TILE = 256;        // outputs per workgroup = threads (io_utils/resample.py::TILE restates it for the tests)
constexpr int RESAMPLE_X_LDS = 9216;      // floats of input span staged per workgroup (36 KiB)
constexpr int RESAMPLE_H_LDS = 4096;      // floats of filter staged per workgroup (16 KiB)
constexpr int RESAMPLE_MAX_RATE = 1024;

template <bool X_LDS, bool H_LDS>
__global__ __launch_bounds__(RESAMPLE_TILE) void resample_poly_kernel(const float* __restrict__ x, const int* __restrict__ len, long long Lmax, int up,
                                                                      int down, int K4, int span_cap, const float* __restrict__ h,
                                                                      float* __restrict__ y, long long Omax, unsigned* __restrict__ peak) {
    extern __shared__ float lds[];
    __shared__ float red[RESAMPLE_TILE];
    float* xs = lds;                                          // [span_cap] when X_LDS
    float* hs = lds + (X_LDS ? span_cap : 0);                 // [up * K4] when H_LDS
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long n0 = (long long)blockIdx.x * RESAMPLE_TILE, n = n0 + tid;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const long long O = (L * up + down - 1) / down;           // this row's output length (<= Omax: checked on the host for Lmax)
    float* yb = y + (size_t)b * (size_t)Omax;
    if (n0 >= O) {                                            // (uniform) a tile behind the row's end: zeros
        if (n < Omax) yb[n] = 0.f;
        return;
    }
    const float* xb = x + (size_t)b * (size_t)Lmax;
    const long long half = 10ll * (up > down ? up : down);
    const long long nl = (n0 + RESAMPLE_TILE < O ? n0 + RESAMPLE_TILE : O) - 1;      // last output of the tile
    const long long i0 = (n0 * down + half) / up - (K4 - 1);                           // first input sample any output of the tile reads (may be < 0)
    if (X_LDS) {
        long long S = (nl * down + half) / up - i0 + 1;
        S = S > span_cap ? span_cap : S;                      // (S <= span_cap by construction; the clamp keeps a wrong host value inside the buffer)
        for (int s = tid; s < (int)S; s += RESAMPLE_TILE) {
            const long long i = i0 + s;
            xs[s] = (i >= 0 && i < L) ? xb[i] : 0.f;
        }
    }
    if (H_LDS)
        for (int k = tid; k < up * K4; k += RESAMPLE_TILE) hs[k] = h[k];
    if (X_LDS || H_LDS) __syncthreads();

    float v = 0.f;
    if (n < O) {
        const long long c = n * down + half;
        const long long ihi = c / up;
        const int p = (int)(c - ihi * up);
        const float* hp = (H_LDS ? hs : h) + p;
        const float* xl = xs + (ihi - i0);                    // X_LDS: xl[-j] = x[ihi - j]; ihi - i0 in [K4 - 1, span_cap)
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int j = 0; j < K4; j += 4) {
            float a0, a1, a2, a3;
            if (X_LDS) {
                a0 = xl[-j];
                a1 = xl[-j - 1];
                a2 = xl[-j - 2];
                a3 = xl[-j - 3];
            } else {
                const long long i = ihi - j;
                a0 = (i >= 0 && i < L) ? xb[i] : 0.f;
                a1 = (i - 1 >= 0 && i - 1 < L) ? xb[i - 1] : 0.f;
                a2 = (i - 2 >= 0 && i - 2 < L) ? xb[i - 2] : 0.f;
                a3 = (i - 3 >= 0 && i - 3 < L) ? xb[i - 3] : 0.f;
            }
            const float* hj = hp + (size_t)j * up;
            s0 = fmaf(a0, hj[0], s0);
            s1 = fmaf(a1, hj[up], s1);
            s2 = fmaf(a2, hj[2 * up], s2);
            s3 = fmaf(a3, hj[3 * up], s3);
        }
        v = (s0 + s1) + (s2 + s3);
    }
    if (n < Omax) yb[n] = v;

    red[tid] = fabsf(v);
    __syncthreads();
    for (int off = RESAMPLE_TILE / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmaxf(red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) atomicMax(peak + b, __float_as_uint(red[0]));   // bits of non-negative floats order as unsigned integers
}

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_resample_poly(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t up, int32_t down, const float* taps_dev,
                                  int64_t ntaps, float* y_dev, int64_t Omax, float* peak_dev, void* stream) {
    TTSC_REQUIRE(up > 0 && down > 0 && up <= RESAMPLE_MAX_RATE && down <= RESAMPLE_MAX_RATE,
                 "ttsc_resample_poly: rates up=%d down=%d: both must lie in [1, %d] after reduction (no sample rates with a small common divisor)", up,
                 down, RESAMPLE_MAX_RATE);
    TTSC_REQUIRE(B > 0 && B <= 65535 && Lmax > 0 && Omax > 0, "ttsc_resample_poly: bad sizes (B=%d Lmax=%lld Omax=%lld, up=%d down=%d)", B,
                 (long long)Lmax, (long long)Omax, up, down);
    TTSC_REQUIRE(x_dev && len_dev && taps_dev && y_dev && peak_dev, "ttsc_resample_poly: null argument");
    TTSC_REQUIRE(Lmax < (int64_t)1 << 40, "ttsc_resample_poly: rows of %lld samples are too long", (long long)Lmax);
    const int64_t half = 10 * (int64_t)(up > down ? up : down);
    const int64_t K = ceil_div(2 * half + 1, up), K4 = round_up(K, 4);
    TTSC_REQUIRE(ntaps == (int64_t)up * K4, "ttsc_resample_poly: %lld filter taps for up=%d down=%d, %lld expected (the filter padded to up * K4)",
                 (long long)ntaps, up, down, (long long)((int64_t)up * K4));
    const int64_t need = ceil_div(Lmax * up, down);
    TTSC_REQUIRE(Omax >= need, "ttsc_resample_poly: Omax=%lld is shorter than the %lld outputs of a row of Lmax=%lld samples at up=%d down=%d",
                 (long long)Omax, (long long)need, (long long)Lmax, up, down);
    const int64_t tiles = ceil_div(Omax, RESAMPLE_TILE);
    TTSC_REQUIRE(tiles < (int64_t)1 << 31, "ttsc_resample_poly: Omax=%lld needs too many tiles", (long long)Omax);
    const int64_t span = ceil_div((int64_t)(RESAMPLE_TILE - 1) * down, up) + K4;
    const bool x_lds = span <= RESAMPLE_X_LDS, h_lds = ntaps <= RESAMPLE_H_LDS;
    const size_t lds = ((x_lds ? span : 0) + (h_lds ? ntaps : 0)) * sizeof(float);
    TTSC_HIP_CHECK(hipMemsetAsync(peak_dev, 0, (size_t)B * sizeof(float), (hipStream_t)stream));
    const dim3 grid((unsigned)tiles, (unsigned)B), block(RESAMPLE_TILE);
#define TTSC_RESAMPLE_LAUNCH(XL, HL)                                                                                                                 \
    hipLaunchKernelGGL((resample_poly_kernel<XL, HL>), grid, block, lds, (hipStream_t)stream, x_dev, len_dev, (long long)Lmax, up, down, (int)K4, \
                       (int)span, taps_dev, y_dev, (long long)Omax, reinterpret_cast<unsigned*>(peak_dev))
    if (x_lds && h_lds)
        TTSC_RESAMPLE_LAUNCH(true, true);
    else if (x_lds)
        TTSC_RESAMPLE_LAUNCH(true, false);
    else if (h_lds)
        TTSC_RESAMPLE_LAUNCH(false, true);
    else
        TTSC_RESAMPLE_LAUNCH(false, false);
#undef TTSC_RESAMPLE_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("resample_poly_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
