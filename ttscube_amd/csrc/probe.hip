// Measurement helper (bench.py, tools/): what the f16 matrix pipe of THIS device sustains, by operand data.
//
// MI355X clocks to its power budget (MI355X_MICROARCH.md, "DVFS give-back"): a register-only loop of v_mfma_f32_32x32x16_f16 reaches ~0.95 of the
// nominal 2.5 PFLOP/s on all-zero operands and ~0.66 - 0.68 on random fp16 operands (round-4 measurement, tools/probes/mfma_power_probe.hip:
// 2363 / 1655 / 1706 TFLOP/s).  Every MFMA-bound kernel of the generator runs on real data, so `roofline.peak` (nominal, as the contract asks)
// overstates what is reachable by that factor; bench.py reports both.
#include "common.hpp"

namespace ttsc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// 4 independent accumulators per wave, the three products of the split-precision scheme per step (lo x hi, hi x lo, hi x hi)
__global__ __launch_bounds__(512) void mfma_sustained_kernel(const half8* ops, int iters, float* sink) {
    const int lane = threadIdx.x & 63;
    const half8 a0 = ops[lane], a1 = ops[64 + lane], b0 = ops[128 + lane], b1 = ops[192 + lane];   // a0 / b0: "hi", a1 / b1: "lo"
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[i], 0, 0, 0);
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[i], 0, 0, 0);
        }
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) t += acc[i][0] + acc[i][7];
    if (t == 123.456f) sink[0] = t;   // keeps the accumulators alive
}

}  // namespace ttsc

using namespace ttsc;

// mode 0: all-zero operands; 1: random fp16 operands of unit scale; 2: the split-precision mix (hi operands unit scale, lo operands 2^-11 scale).
// Runs the loop for ~ms_target milliseconds on every CU (8 waves per CU) on `stream`, returns executed dense f16 MFMA TFLOP/s in *tflops_out.
extern "C" int ttsc_probe_mfma_tflops(int32_t mode, double ms_target, double* tflops_out, void* stream) {
    TTSC_REQUIRE(tflops_out && mode >= 0 && mode <= 2 && ms_target > 0 && ms_target <= 2000, "ttsc_probe_mfma_tflops: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int cus = device_cus();
    std::vector<_Float16> h(256 * 8);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < h.size(); ++i) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const float u = (float)((st >> 40) & 0xffffff) / 8388608.f - 1.f;   // [-1, 1)
        const bool lo = (i / (64 * 8)) & 1;
        h[i] = (_Float16)(mode == 0 ? 0.f : (mode == 2 && lo ? u * 4.8828125e-4f : u));
    }
    half8* d = nullptr;
    float* sink = nullptr;
    TTSC_HIP_CHECK(hipMalloc((void**)&d, h.size() * sizeof(_Float16)));
    if (hipMalloc((void**)&sink, sizeof(float)) != hipSuccess) {
        (void)hipFree(d);
        set_error("ttsc_probe_mfma_tflops: allocation failed");
        return TTSC_ENOMEM;
    }
    int rc = TTSC_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMemcpy(d, h.data(), h.size() * sizeof(_Float16), hipMemcpyHostToDevice) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
        hipEventCreate(&e1) != hipSuccess)
        rc = TTSC_EHIP;
    if (!rc) {
        // 12 MFMAs of 32 nominal cycles per iteration and wave, two waves per SIMD: ~0.32 us per iteration at 2.4 GHz
        const int iters = (int)(ms_target * 1e3 / 0.32);
        hipLaunchKernelGGL(mfma_sustained_kernel, dim3(cus), dim3(512), 0, s, d, iters / 10 + 1, sink);   // warm-up: clocks settle
        (void)hipEventRecord(e0, s);
        hipLaunchKernelGGL(mfma_sustained_kernel, dim3(cus), dim3(512), 0, s, d, iters, sink);
        (void)hipEventRecord(e1, s);
        float ms = 0.f;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || !(ms > 0.f)) {
            set_error("ttsc_probe_mfma_tflops: timing failed");
            rc = TTSC_EHIP;
        } else {
            *tflops_out = (double)cus * 8 * iters * 12 * (2.0 * 32 * 32 * 16) / ms / 1e9;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d);
    (void)hipFree(sink);
    return rc;
}

// ---- test-only probes of include/ttscube_math.h (tests/test_shared_math_gpu.py) ------------------------------------------------------------
// This file is compiled with the library's ordinary CXXFLAGS (csrc/Makefile: -O3 -ffp-contract=off, hipcc's default division / square-root
// rounding and denormal handling), so what these kernels evaluate is what the decode kernels evaluate: the header's functions, one element or
// one row per thread, and wr_sample_continuous (wavernn_sampler.hpp) one row per wave with all 64 lanes calling, as the decode kernels do.
// The host counterparts are the *_array entries of oracle/wavernn_ref.c; the tests hold the two equal bit for bit.
#include "wavernn_sampler.hpp"

namespace ttsc {

__global__ __launch_bounds__(256) void probe_math_kernel(int fn, const void* in, float* out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = ((const float*)in)[i];
    const uint32_t r = ((const uint32_t*)in)[i];
    float y = 0.f;
    switch (fn) {
        case TTSC_PROBE_EXPF: y = ttsc_expf(x); break;
        case TTSC_PROBE_LOGF: y = ttsc_logf(x); break;
        case TTSC_PROBE_SIGMOIDF: y = ttsc_sigmoidf(x); break;
        case TTSC_PROBE_TANHF: y = ttsc_tanhf(x); break;
        case TTSC_PROBE_NORMAL_ICDF: y = ttsc_normal_icdf(x); break;
        case TTSC_PROBE_LOGISTIC: y = ttsc_logistic(x); break;
        case TTSC_PROBE_U01: y = ttsc_u01(r); break;
        case TTSC_PROBE_U01_CLIP: y = ttsc_u01_clip(r); break;
        default: y = ttsc_gumbel(r); break;
    }
    out[i] = y;
}

__global__ __launch_bounds__(256) void probe_philox_kernel(const uint32_t* ctr, const uint32_t* key, uint32_t* out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t r4[4];
    ttsc_philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], r4);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = r4[j];
}

__device__ __forceinline__ int probe_noise_width(int out_kind) {
    return out_kind == TTSC_WR_OUT_MOL ? TTSC_MOL_NOISE : out_kind == TTSC_WR_OUT_GM ? TTSC_GM_NOISE : TTSC_BETA_NOISE;
}

__global__ __launch_bounds__(256) void probe_noise_kernel(int kind, const uint32_t* t, const uint32_t* b, const unsigned long long* seed, float* out,
                                                          long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float nz[TTSC_BETA_NOISE];
    if (kind == TTSC_WR_OUT_MOL)
        ttsc_noise_mol(t[i], b[i], seed[i], nz);
    else if (kind == TTSC_WR_OUT_GM)
        ttsc_noise_gm(t[i], b[i], seed[i], nz);
    else
        ttsc_noise_beta(t[i], b[i], seed[i], nz);
    const int w = probe_noise_width(kind);
    for (int j = 0; j < w; ++j) out[i * w + j] = nz[j];
}

// impl 0: the header's samplers, one thread per row — the statement sequence of the oracle's wr_decode_at (oracle/wavernn_ref.c)
__global__ __launch_bounds__(256) void probe_sample_header_kernel(int out_kind, int mode, int S, const float* y, const float* noise, const uint32_t* t,
                                                                  const uint32_t* b, const unsigned long long* seed, float* wv, int32_t* k,
                                                                  long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int w = probe_noise_width(out_kind);
    float yr[3 * TTSC_MOL_NMIX], nz[TTSC_BETA_NOISE];
    for (int j = 0; j < S; ++j) yr[j] = y[i * S + j];
    for (int j = 0; j < TTSC_BETA_NOISE; ++j) nz[j] = 0.f;
    if (mode == TTSC_WR_MODE_NOISE) {
        for (int j = 0; j < w; ++j) nz[j] = noise[i * w + j];
    } else if (mode == TTSC_WR_MODE_PHILOX) {
        if (out_kind == TTSC_WR_OUT_MOL)
            ttsc_noise_mol(t[i], b[i], seed[i], nz);
        else if (out_kind == TTSC_WR_OUT_GM)
            ttsc_noise_gm(t[i], b[i], seed[i], nz);
        else
            ttsc_noise_beta(t[i], b[i], seed[i], nz);
    } else if (out_kind == TTSC_WR_OUT_BETA) {
        for (int v = 0; v < 2; ++v) nz[v * (1 + 2 * TTSC_BETA_TRIES)] = 0.5f, nz[v * (1 + 2 * TTSC_BETA_TRIES) + 2] = 0.5f;
    }
    int best = 0;
    float x;
    if (out_kind == TTSC_WR_OUT_MOL)
        x = ttsc_sample_mol(yr, nz, nz[TTSC_MOL_NMIX], &best);
    else if (out_kind == TTSC_WR_OUT_GM)
        x = ttsc_sample_gm(yr, nz[0]);
    else
        x = ttsc_sample_beta(yr, nz);
    wv[i] = x;
    k[i] = best;
}

// impl 1: wr_sample_continuous, one wave per row (4 rows per workgroup), the row staged in LDS as in the decode kernels
__global__ __launch_bounds__(256) void probe_sample_wave_kernel(int out_kind, int mode, int S, const float* y, const float* noise, const uint32_t* t,
                                                                const uint32_t* b, const unsigned long long* seed, float* wv, int32_t* k,
                                                                long long n) {
    __shared__ float ys[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + wave;
    const bool live = i < n;
    if (live && lane < S) ys[wave][lane] = y[i * S + lane];
    __syncthreads();
    if (!live) return;   // whole waves leave together: every shuffle below has its 64 lanes
    const bool px = mode == TTSC_WR_MODE_PHILOX;
    float x;
    int best;
    wr_sample_continuous(out_kind, mode, ys[wave], noise, (size_t)i, px ? (int)t[i] : 0, px ? (int)b[i] : 0, px ? seed[i] : 0ull, lane, x, best);
    if (lane == 0) {
        wv[i] = x;
        k[i] = best;
    }
}

}  // namespace ttsc

extern "C" int ttsc_probe_math(int32_t fn, const void* in_dev, float* out_dev, int64_t n, void* stream) {
    TTSC_REQUIRE(fn >= TTSC_PROBE_EXPF && fn <= TTSC_PROBE_GUMBEL, "ttsc_probe_math: fn %d is not a TTSC_PROBE_* function", (int)fn);
    TTSC_REQUIRE(in_dev && out_dev && n > 0 && n <= (int64_t)1 << 31, "ttsc_probe_math: null pointer or n outside [1, 2^31]");
    hipLaunchKernelGGL(probe_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)fn, in_dev, out_dev, (long long)n);
    return launch_checked("probe_math_kernel");
}

extern "C" int ttsc_probe_philox(const uint32_t* ctr_dev, const uint32_t* key_dev, uint32_t* out_dev, int64_t n, void* stream) {
    TTSC_REQUIRE(ctr_dev && key_dev && out_dev && n > 0 && n <= (int64_t)1 << 28, "ttsc_probe_philox: null pointer or n outside [1, 2^28]");
    hipLaunchKernelGGL(probe_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctr_dev, key_dev, out_dev, (long long)n);
    return launch_checked("probe_philox_kernel");
}

extern "C" int ttsc_probe_noise(int32_t kind, const uint32_t* t_dev, const uint32_t* b_dev, const uint64_t* seed_dev, float* out_dev, int64_t n,
                                void* stream) {
    TTSC_REQUIRE(kind == TTSC_WR_OUT_MOL || kind == TTSC_WR_OUT_GM || kind == TTSC_WR_OUT_BETA, "ttsc_probe_noise: kind %d is not MOL / GM / BETA", (int)kind);
    TTSC_REQUIRE(t_dev && b_dev && seed_dev && out_dev && n > 0 && n <= (int64_t)1 << 26, "ttsc_probe_noise: null pointer or n outside [1, 2^26]");
    hipLaunchKernelGGL(probe_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)kind, t_dev, b_dev,
                       (const unsigned long long*)seed_dev, out_dev, (long long)n);
    return launch_checked("probe_noise_kernel");
}

extern "C" int ttsc_probe_sample(int32_t out_kind, int32_t mode, int32_t impl, const float* y_dev, const float* noise_dev, const uint32_t* t_dev,
                                 const uint32_t* b_dev, const uint64_t* seed_dev, float* wv_dev, int32_t* k_dev, int64_t n, void* stream) {
    TTSC_REQUIRE(out_kind == TTSC_WR_OUT_MOL || out_kind == TTSC_WR_OUT_GM || out_kind == TTSC_WR_OUT_BETA,
                 "ttsc_probe_sample: out_kind %d is not MOL / GM / BETA", (int)out_kind);
    TTSC_REQUIRE(mode >= TTSC_WR_MODE_ARGMAX && mode <= TTSC_WR_MODE_PHILOX && (impl == 0 || impl == 1), "ttsc_probe_sample: bad mode %d or impl %d",
                 (int)mode, (int)impl);
    TTSC_REQUIRE(y_dev && wv_dev && k_dev && n > 0 && n <= (int64_t)1 << 26, "ttsc_probe_sample: null pointer or n outside [1, 2^26]");
    TTSC_REQUIRE(mode != TTSC_WR_MODE_NOISE || noise_dev, "ttsc_probe_sample: MODE_NOISE needs noise_dev");
    TTSC_REQUIRE(mode != TTSC_WR_MODE_PHILOX || (t_dev && b_dev && seed_dev), "ttsc_probe_sample: MODE_PHILOX needs t_dev, b_dev and seed_dev");
    const int S = out_kind == TTSC_WR_OUT_MOL ? 3 * TTSC_MOL_NMIX : 2;
    const unsigned long long* sd = (const unsigned long long*)seed_dev;
    if (impl == 0) {
        hipLaunchKernelGGL(probe_sample_header_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)out_kind, (int)mode, S,
                           y_dev, noise_dev, t_dev, b_dev, sd, wv_dev, k_dev, (long long)n);
        return launch_checked("probe_sample_header_kernel");
    }
    hipLaunchKernelGGL(probe_sample_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (int)out_kind, (int)mode, S, y_dev,
                       noise_dev, t_dev, b_dev, sd, wv_dev, k_dev, (long long)n);
    return launch_checked("probe_sample_wave_kernel");
}
