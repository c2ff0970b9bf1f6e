// Device pieces shared by every split-precision (f16x3) convolution kernel: conv_f16x3_kernel (conv_kernels.hpp) and the wide / tall kernels
// (conv_f16x3_widetall.hpp).  The bits of a layer depend on the operation ORDER of each of them, and a layer may run on either kernel (the
// machine-fill rule decides per launch), so each piece has exactly one definition, here.
#pragma once
#include "conv_internal.hpp"

namespace ttsc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
struct half8x2 {
    half8 hi, lo;
};

// The three product terms of one tap: lo_w * hi_x, hi_w * lo_x, hi_w * hi_x (smallest first), each a sweep over the wave's MI x NJ tiles so that
// consecutive MFMAs go to DIFFERENT accumulators (no back-to-back dependency).  acc: f32x16 [MI][NJ]; ah, al: half8 [MI]; bh, bl: half8 [NJ].
// A macro, not a function: a call that takes the accumulators by reference keeps them in memory until it is inlined, after the first
// round of scalar replacement, and conv_f16x3_kernel then compiles to other code (57 more VALU instructions in its <2, 1, *, FOLD> variants).
#define TTSC_MFMA3_F16X3(MI, NJ, acc, ah, al, bh, bl)                                                                                          \
    do {                                                                                                                                       \
        _Pragma("unroll") for (int i_ = 0; i_ < (MI); ++i_)                                                                                    \
            _Pragma("unroll") for (int n_ = 0; n_ < (NJ); ++n_) acc[i_][n_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i_], bh[n_], acc[i_][n_], 0, 0, 0); \
        _Pragma("unroll") for (int i_ = 0; i_ < (MI); ++i_)                                                                                    \
            _Pragma("unroll") for (int n_ = 0; n_ < (NJ); ++n_) acc[i_][n_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i_], bl[n_], acc[i_][n_], 0, 0, 0); \
        _Pragma("unroll") for (int i_ = 0; i_ < (MI); ++i_)                                                                                    \
            _Pragma("unroll") for (int n_ = 0; n_ < (NJ); ++n_) acc[i_][n_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i_], bh[n_], acc[i_][n_], 0, 0, 0); \
    } while (0)

// One staging item: 8 fp32 channels of one position -> lrelu(in_scale * x) (slopes in [0, 1]; 1 = identity) -> (hi, lo) fp16 items.  `ok(ch)`
// says whether channel ch of the item is data; padding becomes +0.  Pairwise: cvt_pk + two fma_mix + cvt_pk per pair (split2_f16: same bits as
// the scalar convert / convert back / subtract / convert sequence, two instructions fewer per pair).
template <class OK>
__device__ __forceinline__ half8x2 lrelu_split8(const float (&x)[8], float in_scale, float in_slope, OK ok) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 uh, ul;
#pragma unroll
    for (int ch = 0; ch < 8; ch += 2) {
        float v0 = ok(ch) ? x[ch] * in_scale : 0.f, v1 = ok(ch + 1) ? x[ch + 1] * in_scale : 0.f;
        v0 = fmaxf(v0, v0 * in_slope);
        v1 = fmaxf(v1, v1 * in_slope);
        unsigned h, l;
        split2_f16(v0, v1, h, l);
        uh[ch >> 1] = h;
        ul[ch >> 1] = l;
    }
    return {__builtin_bit_cast(half8, uh), __builtin_bit_cast(half8, ul)};
}

// `acc_init` layers (ConvArgs::acc_init): the sums START at (first [+ second] + bias) / w_unscale and the epilogue is the store of
// acc * w_unscale (w_unscale is a power of two: both exact).  One lane's 16 values of a 32 x 32 tile start as `first` (the residual or the
// running sum, zero without either) and take these steps in this order: acc_init_add(second) when both operands are present,
// acc_init_add(bias), acc_init_scale(1 / w_unscale).  The general kernel takes them tile by tile, the wide kernel operand by operand across
// its tiles (the loads of an operand leave together).  Without a bias the general kernel adds a vector of zeros and the wide kernel skips the
// step, as both always did: the same bits unless the sum so far is -0.
__device__ __forceinline__ void acc_init_add(f32x16& v, const float (&x)[16]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] += x[r];
}
__device__ __forceinline__ void acc_init_scale(f32x16& v, float inv) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] *= inv;
}
// yp = the lane's first row (channel 4 * (lane >> 5) of the tile) at its column; rows follow the C/D layout of v_mfma_*_32x32
__device__ __forceinline__ void acc_init_store(const f32x16& acc, float w_unscale, float* yp, int Lout) {
#pragma unroll
    for (int r = 0; r < 16; ++r) yp[(size_t)((r & 3) + 8 * (r >> 2)) * Lout] = acc[r] * w_unscale;
}

}  // namespace ttsc
