// Complex STFT, inverse STFT and the Griffin-Lim projection step on a radix-4 Stockham FFT held in LDS, for the rest of
// MelVocoder (cube/io_utils/vocoder.py:42-52,69-75,100-124: fft / ifft / griffinlim through librosa.stft / librosa.istft).
// The float64 statement is tests/griffinlim_reference.py; the Python side is io_utils/stft.py.
//
// Conventions (librosa's, as melspectrogram_log10 already uses them): periodic Hann of length n_fft, centred frames over
// n_fft/2 samples of reflect padding, NB = n_fft/2 + 1 bins, F = 1 + L // hop frames, the inverse returns hop (F - 1) samples.
//
// One workgroup of 256 threads transforms FRAMES_PER_WG consecutive frames of ONE row, one after the other, each as one
// n_fft-point complex transform: a frame's bits depend on that frame's samples alone, so a row has the same bits alone, in
// any batch and at any position in it.  The transform is the auto-sort (Stockham) schedule between two LDS buffers, radix 4
// with one closing radix-2 stage for 512 and 2048: stage Ns = 1, 4, 16 .. reads in[j + r n_fft/4], r < 4 (contiguous in the
// thread index: conflict-free) and writes out[j0 + r Ns], j0 = 4 (j - j % Ns) + j % Ns (contiguous runs of Ns).  The
// twiddles exp(-2 pi i k / (2 M)), k < M, sit at table[M + k] for every M = 1, 2, 4 .. n_fft/2: each stage reads contiguous
// runs (a single exp(-2 pi i m / n_fft) table is read at stride n_fft / (4 Ns): 16-way conflicts in the middle stages).
// Table and window come from the host, built in float64 and rounded once; no sincosf in here.  No atomics, every sum in a fixed order, 64-bit offsets.
#include <cfloat>

#include "common.hpp"

namespace ttsc {

constexpr int FFT_THREADS = 256;
constexpr int FRAMES_PER_WG = 4;          // frames one workgroup transforms with one load of the tables

template <int N>
struct FftShared {
    float2 buf[2][N];
    float2 tw[N];                          // tw[Ns + k] = exp(-2 pi i k / (2 Ns)), k < Ns; tw[0] unused
};

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// N-point transform of s.buf[cur] (fully written and barrier-ed by the caller) -> s.buf[returned index], visible to every thread.
// Radix-4 stages Ns = 1, 4, 16 .. while 4 Ns <= N, then one radix-2 stage if log2 N is odd.  INV: conjugated twiddles (the unscaled inverse).
// The powers of a radix-4 stage's twiddle w = exp(-2 pi i k / (4 Ns)) all come from the table, none from a product:
//   w = tw[2 Ns + k],  w^2 = tw[Ns + k],  w^3 = tw[2 Ns + 3k] for 3k < 2 Ns and -tw[3k] beyond (half a turn further).
template <int N, bool INV>
__device__ __forceinline__ int fft_run(FftShared<N>& s, int cur) {
    const int tid = threadIdx.x;
    int Ns = 1;
    for (; 4 * Ns <= N; Ns <<= 2) {
        const float2* in = s.buf[cur];
        float2* out = s.buf[cur ^ 1];
#pragma unroll
        for (int j = tid; j < N / 4; j += FFT_THREADS) {
            const int k = j & (Ns - 1);
            float2 w1 = s.tw[2 * Ns + k], w2 = s.tw[Ns + k], w3;
            if (3 * k < 2 * Ns) {
                w3 = s.tw[2 * Ns + 3 * k];
            } else {
                w3 = s.tw[3 * k];
                w3 = make_float2(-w3.x, -w3.y);
            }
            if (INV) w1.y = -w1.y, w2.y = -w2.y, w3.y = -w3.y;
            const float2 v0 = in[j], v1 = cmul(in[j + N / 4], w1), v2 = cmul(in[j + N / 2], w2), v3 = cmul(in[j + 3 * (N / 4)], w3);
            const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
            const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y);
            const float2 d = make_float2(v1.x - v3.x, v1.y - v3.y);
            const float2 a3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);      // (v1 - v3) times +i (inverse) or -i (forward)
            const int j0 = ((j - k) << 2) + k;
            out[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
            out[j0 + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
            out[j0 + 2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
            out[j0 + 3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (Ns < N) {                                                 // Ns = N/2: the last, radix-2 stage of 512 and 2048
        const float2* in = s.buf[cur];
        float2* out = s.buf[cur ^ 1];
#pragma unroll
        for (int j = tid; j < N / 2; j += FFT_THREADS) {
            float2 w = s.tw[N / 2 + j];
            if (INV) w.y = -w.y;
            const float2 u = in[j], v = cmul(in[j + N / 2], w);
            out[j] = make_float2(u.x + v.x, u.y + v.y);
            out[j + N / 2] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// exp(1j * angle(z)) without forming re^2 + im^2 at z's own scale (it underflows below ~1e-19 and overflows above ~1e19): z is divided by
// max(|re|, |im|) first, which leaves a vector of length 1 .. sqrt(2).  (0, 0) -> (1, 0), numpy's angle(0) = 0.
__device__ __forceinline__ float2 unit_phase(float2 z) {
    const float m = fmaxf(fabsf(z.x), fabsf(z.y));
    if (!(m > 0.f)) return make_float2(1.f, 0.f);
    const float r = z.x / m, i = z.y / m;
    const float h = sqrtf(r * r + i * i);
    return make_float2(r / h, i / h);
}

// frames of row b that the kernels touch: frames[b] clamped to [0, Fmax]; a row too short for its reflect padding counts as empty (the
// host refuses it before the launch; this only keeps a stale table from turning into an out-of-bounds read)
__device__ __forceinline__ int row_frames(const int* __restrict__ frames, int b, int Fmax, int n_fft, int hop) {
    int Fb = frames ? frames[b] : Fmax;
    if (Fb > Fmax) Fb = Fmax;
    if (Fb < 1 || (long)hop * (Fb - 1) < n_fft / 2 + 1) Fb = 0;
    return Fb;
}

enum { MODE_ANALYZE = 0, MODE_SYNTHESIZE = 1, MODE_PROJECT = 2 };

// MODE_ANALYZE     sig [B, Lpad] -> out = spectrum [B, Fmax, NB] (re, im)
// MODE_SYNTHESIZE  in = spectrum [B, Fmax, NB] (re, im) -> out = windowed frames [B, Fmax, N]
// MODE_PROJECT     sig [B, Lpad], in = magnitude [B, Fmax, NB] -> out = windowed frames of |mag| . phase(STFT(sig))
// grid (ceil(Fmax / FRAMES_PER_WG), B).  Rows of `out` at or beyond row_frames are written as zeros; nothing of them is read.
template <int N, int MODE>
__global__ __launch_bounds__(FFT_THREADS) void stft_fft_kernel(const float* __restrict__ sig, long Lpad, const float* __restrict__ in,
                                                               const int* __restrict__ frames, int Fmax, int hop,
                                                               const float* __restrict__ tables, float* __restrict__ out) {
    constexpr int NB = N / 2 + 1;
    constexpr int PT = (N + FFT_THREADS - 1) / FFT_THREADS;      // samples per thread
    __shared__ FftShared<N> s;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Fb = row_frames(frames, b, Fmax, N, hop);
    for (int i = tid; i < N; i += FFT_THREADS) s.tw[i] = reinterpret_cast<const float2*>(tables)[i];
    float win[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) win[i] = tables[2 * N + tid + FFT_THREADS * i];
    __syncthreads();
    const int f0 = blockIdx.x * FRAMES_PER_WG;
    for (int f = f0; f < f0 + FRAMES_PER_WG && f < Fmax; ++f) {
        const size_t row = (size_t)b * Fmax + f;
        if (f >= Fb) {                                            // the same for every thread of the workgroup
            if (MODE == MODE_ANALYZE) {
                for (int k = tid; k < NB; k += FFT_THREADS) reinterpret_cast<float2*>(out)[row * NB + k] = make_float2(0.f, 0.f);
            } else {
#pragma unroll
                for (int i = 0; i < PT; ++i) out[row * N + tid + FFT_THREADS * i] = 0.f;
            }
            continue;
        }
        int cur = 0;
        if (MODE != MODE_SYNTHESIZE) {
            const float* x = sig + (size_t)b * Lpad + (size_t)f * hop;
#pragma unroll
            for (int i = 0; i < PT; ++i) s.buf[0][tid + FFT_THREADS * i] = make_float2(x[tid + FFT_THREADS * i] * win[i], 0.f);
            __syncthreads();
            cur = fft_run<N, false>(s, 0);
        }
        if (MODE == MODE_ANALYZE) {
            for (int k = tid; k < NB; k += FFT_THREADS) {
                float2 z = s.buf[cur][k];
                if (k == 0 || k == N / 2) z.y = 0.f;              // a real signal's bins 0 and N/2 are real (rfft returns them so)
                reinterpret_cast<float2*>(out)[row * NB + k] = z;
            }
        } else {
            // the Hermitian spectrum of the real inverse, in place: bin k <= N/2 is read by its own thread only, bins above N/2 by nobody
            float2* X = s.buf[cur];
            for (int k = tid; k < NB; k += FFT_THREADS) {
                float2 v;
                if (MODE == MODE_SYNTHESIZE) {
                    v = reinterpret_cast<const float2*>(in)[row * NB + k];
                    if (k == 0 || k == N / 2) v.y = 0.f;          // ignored, as irfft ignores them
                } else {
                    float2 z = X[k];
                    if (k == 0 || k == N / 2) z.y = 0.f;
                    const float2 p = unit_phase(z);
                    const float m = fabsf(in[row * NB + k]);
                    v = make_float2(m * p.x, m * p.y);
                }
                X[k] = v;
                if (k > 0 && k < N / 2) X[N - k] = make_float2(v.x, -v.y);
            }
            __syncthreads();
            cur = fft_run<N, true>(s, cur);
#pragma unroll
            for (int i = 0; i < PT; ++i) out[row * N + tid + FFT_THREADS * i] = (s.buf[cur][tid + FFT_THREADS * i].x * (1.f / N)) * win[i];
        }
        __syncthreads();                                          // the next frame overwrites the buffers read above
    }
}

// One output sample of librosa.istft before the trim: q counts from the start of the first frame.
//   s = sum over frames f < Fb with f hop <= q < f hop + n of frames[f, q - f hop],  e = the same sum of window[q - f hop]^2
// ascending f, at most ceil(n / hop) terms; s / e where e > FLT_MIN (window_sumsquare's `> tiny` rule), s elsewhere.
__device__ __forceinline__ float ola_sample(const float* __restrict__ fr, const float* __restrict__ win, long q, int Fb, int n, int hop) {
    long f_hi = q / hop;
    if (f_hi > Fb - 1) f_hi = Fb - 1;
    const long f_lo = q < n ? 0 : (q - n) / hop + 1;
    float s = 0.f, e = 0.f;
    for (long f = f_lo; f <= f_hi; ++f) {
        const long i = q - f * hop;
        const float w = win[i];
        s += fr[(size_t)f * n + i];
        e += w * w;
    }
    return e > FLT_MIN ? s / e : s;
}

// windowed frames [B, Fmax, n] -> out [B, ldo]; row b has Lb = hop (Fb - 1) samples.
//   padded == 0: out[b, t] = audio sample t (t < Lb), zeros behind; ldo = hop (Fmax - 1)
//   padded != 0: out[b, p] = audio sample reflect(p - n/2) (p < Lb + n), zeros behind: the signal the next analysis reads, pad samples from
//                the same formula at their mirror positions; ldo = hop (Fmax - 1) + n
// grid (., B), one thread per output sample
__global__ __launch_bounds__(256) void stft_ola_kernel(const float* __restrict__ fr, const int* __restrict__ frames, int Fmax, int n, int hop,
                                                       const float* __restrict__ win, int padded, float* __restrict__ out, long ldo) {
    const int b = blockIdx.y;
    const int Fb = row_frames(frames, b, Fmax, n, hop);
    const long Lb = Fb > 0 ? (long)hop * (Fb - 1) : 0;
    const float* frb = fr + (size_t)b * Fmax * n;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < ldo; t += (long)gridDim.x * blockDim.x) {
        long i = t;
        bool live = t < Lb;
        if (padded) {
            live = Fb > 0 && t < Lb + n;
            i = t - n / 2;
            if (i < 0) i = -i;
            else if (i >= Lb) i = 2 * (Lb - 1) - i;
        }
        out[(size_t)b * ldo + t] = live ? ola_sample(frb, win, i + n / 2, Fb, n, hop) : 0.f;
    }
}

// y [B, Lmax] with len[b] samples each -> out [B, Lpad]: out[b, p] = y[b, reflect(p - n/2)] for p < len[b] + n, zeros behind (numpy's
// pad(mode='reflect') by n/2 on both sides).  A row shorter than n/2 + 1 is written as zeros.
__global__ __launch_bounds__(256) void stft_reflect_pad_kernel(const float* __restrict__ y, const int* __restrict__ len, long Lmax, int n,
                                                               float* __restrict__ out, long Lpad) {
    const int b = blockIdx.y;
    long Lb = len ? len[b] : Lmax;
    if (Lb > Lmax) Lb = Lmax;
    if (Lb < n / 2 + 1) Lb = 0;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < Lpad; p += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (Lb > 0 && p < Lb + n) {
            long i = p - n / 2;
            if (i < 0) i = -i;
            else if (i >= Lb) i = 2 * (Lb - 1) - i;
            v = y[(size_t)b * Lmax + i];
        }
        out[(size_t)b * Lpad + p] = v;
    }
}

static inline int ola_grid(long n) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

static bool size_supported(int n_fft) { return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048; }

// the checks every entry point shares; frames_host (the caller's host copy of frames_dev, or both NULL: every row has Fmax frames)
static int check_common(const char* who, int32_t B, int32_t Fmax, int32_t n_fft, int32_t hop, const int32_t* frames_host, const int32_t* frames_dev) {
    TTSC_REQUIRE(size_supported(n_fft), "%s: n_fft=%d is not supported (256, 512, 1024, 2048)", who, n_fft);
    TTSC_REQUIRE(hop >= 1 && hop <= n_fft, "%s: hop=%d outside [1, n_fft=%d]", who, hop, n_fft);
    TTSC_REQUIRE(B >= 1 && B <= 65535 && Fmax >= 1, "%s: B=%d (1 .. 65535) / Fmax=%d", who, B, Fmax);
    TTSC_REQUIRE((frames_host == nullptr) == (frames_dev == nullptr), "%s: frames_host and frames_dev go together", who);
    for (int32_t b = 0; b < B; ++b) {
        const int64_t Fb = frames_host ? frames_host[b] : Fmax;
        TTSC_REQUIRE(Fb >= 1 && Fb <= Fmax, "%s: frames[%d]=%lld outside [1, Fmax=%d]", who, b, (long long)Fb, Fmax);
        TTSC_REQUIRE((int64_t)hop * (Fb - 1) >= n_fft / 2 + 1,
                     "%s: row %d has %lld frames = %lld samples at hop %d; reflect padding of n_fft/2 = %d needs at least %d samples", who, b,
                     (long long)Fb, (long long)((int64_t)hop * (Fb - 1)), hop, n_fft / 2, n_fft / 2 + 1);
        if (!frames_host) break;
    }
    return TTSC_OK;
}

template <int MODE>
static void launch_fft(int n_fft, dim3 grid, hipStream_t st, const float* sig, long Lpad, const float* in, const int* frames, int Fmax, int hop,
                       const float* tables, float* out) {
    switch (n_fft) {
        case 256: hipLaunchKernelGGL((stft_fft_kernel<256, MODE>), grid, dim3(FFT_THREADS), 0, st, sig, Lpad, in, frames, Fmax, hop, tables, out); break;
        case 512: hipLaunchKernelGGL((stft_fft_kernel<512, MODE>), grid, dim3(FFT_THREADS), 0, st, sig, Lpad, in, frames, Fmax, hop, tables, out); break;
        case 1024: hipLaunchKernelGGL((stft_fft_kernel<1024, MODE>), grid, dim3(FFT_THREADS), 0, st, sig, Lpad, in, frames, Fmax, hop, tables, out); break;
        default: hipLaunchKernelGGL((stft_fft_kernel<2048, MODE>), grid, dim3(FFT_THREADS), 0, st, sig, Lpad, in, frames, Fmax, hop, tables, out); break;
    }
}

}  // namespace ttsc

using namespace ttsc;

#define TTSC_LAUNCH_CHECK(name)                                              \
    do {                                                                     \
        hipError_t _e = hipGetLastError();                                   \
        if (_e != hipSuccess) {                                              \
            set_error(name " launch failed: %s", hipGetErrorString(_e));     \
            return TTSC_EHIP;                                                \
        }                                                                    \
    } while (0)

static dim3 fft_grid(int32_t B, int32_t Fmax) { return dim3((unsigned)((Fmax + FRAMES_PER_WG - 1) / FRAMES_PER_WG), (unsigned)B); }

extern "C" int ttsc_stft_reflect_pad(const float* y_dev, const int32_t* len_host, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t n_fft,
                                     float* out_dev, int64_t Lpad, void* stream) {
    TTSC_REQUIRE(y_dev && out_dev, "ttsc_stft_reflect_pad: null pointer");
    TTSC_REQUIRE(size_supported(n_fft), "ttsc_stft_reflect_pad: n_fft=%d is not supported (256, 512, 1024, 2048)", n_fft);
    TTSC_REQUIRE(B >= 1 && B <= 65535 && Lmax >= 1 && Lmax < ((int64_t)1 << 31) && Lpad >= Lmax + n_fft, "ttsc_stft_reflect_pad: B=%d Lmax=%lld Lpad=%lld",
                 B, (long long)Lmax, (long long)Lpad);
    TTSC_REQUIRE((len_host == nullptr) == (len_dev == nullptr), "ttsc_stft_reflect_pad: len_host and len_dev go together");
    for (int32_t b = 0; b < B; ++b) {
        const int64_t Lb = len_host ? len_host[b] : Lmax;
        TTSC_REQUIRE(Lb <= Lmax && Lb >= n_fft / 2 + 1, "ttsc_stft_reflect_pad: row %d has %lld samples; reflect padding of n_fft/2 = %d needs %d .. Lmax=%lld",
                     b, (long long)Lb, n_fft / 2, n_fft / 2 + 1, (long long)Lmax);
        if (!len_host) break;
    }
    hipLaunchKernelGGL(stft_reflect_pad_kernel, dim3(ola_grid(Lpad), (unsigned)B), dim3(256), 0, (hipStream_t)stream, y_dev, len_dev, (long)Lmax, n_fft,
                       out_dev, (long)Lpad);
    TTSC_LAUNCH_CHECK("stft_reflect_pad_kernel");
    return TTSC_OK;
}

extern "C" int ttsc_stft_analyze(const float* sig_dev, int64_t Lpad, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax,
                                 int32_t n_fft, int32_t hop, const float* tables_dev, float* spec_dev, void* stream) {
    TTSC_REQUIRE(sig_dev && tables_dev && spec_dev, "ttsc_stft_analyze: null pointer");
    if (int rc = check_common("ttsc_stft_analyze", B, Fmax, n_fft, hop, frames_host, frames_dev)) return rc;
    TTSC_REQUIRE(Lpad >= (int64_t)hop * (Fmax - 1) + n_fft, "ttsc_stft_analyze: Lpad=%lld < hop (Fmax - 1) + n_fft", (long long)Lpad);
    launch_fft<MODE_ANALYZE>(n_fft, fft_grid(B, Fmax), (hipStream_t)stream, sig_dev, (long)Lpad, nullptr, frames_dev, Fmax, hop, tables_dev, spec_dev);
    TTSC_LAUNCH_CHECK("stft_fft_kernel<analyze>");
    return TTSC_OK;
}

extern "C" int ttsc_stft_synthesize(const float* spec_dev, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax, int32_t n_fft,
                                    int32_t hop, const float* tables_dev, float* frames_out_dev, void* stream) {
    TTSC_REQUIRE(spec_dev && tables_dev && frames_out_dev, "ttsc_stft_synthesize: null pointer");
    if (int rc = check_common("ttsc_stft_synthesize", B, Fmax, n_fft, hop, frames_host, frames_dev)) return rc;
    launch_fft<MODE_SYNTHESIZE>(n_fft, fft_grid(B, Fmax), (hipStream_t)stream, nullptr, 0, spec_dev, frames_dev, Fmax, hop, tables_dev, frames_out_dev);
    TTSC_LAUNCH_CHECK("stft_fft_kernel<synthesize>");
    return TTSC_OK;
}

extern "C" int ttsc_stft_project(const float* sig_dev, int64_t Lpad, const float* mag_dev, const int32_t* frames_host, const int32_t* frames_dev,
                                 int32_t B, int32_t Fmax, int32_t n_fft, int32_t hop, const float* tables_dev, float* frames_out_dev, void* stream) {
    TTSC_REQUIRE(sig_dev && mag_dev && tables_dev && frames_out_dev, "ttsc_stft_project: null pointer");
    if (int rc = check_common("ttsc_stft_project", B, Fmax, n_fft, hop, frames_host, frames_dev)) return rc;
    TTSC_REQUIRE(Lpad >= (int64_t)hop * (Fmax - 1) + n_fft, "ttsc_stft_project: Lpad=%lld < hop (Fmax - 1) + n_fft", (long long)Lpad);
    launch_fft<MODE_PROJECT>(n_fft, fft_grid(B, Fmax), (hipStream_t)stream, sig_dev, (long)Lpad, mag_dev, frames_dev, Fmax, hop, tables_dev, frames_out_dev);
    TTSC_LAUNCH_CHECK("stft_fft_kernel<project>");
    return TTSC_OK;
}

extern "C" int ttsc_stft_overlap_add(const float* frames_in_dev, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax,
                                     int32_t n_fft, int32_t hop, const float* tables_dev, int32_t padded, float* out_dev, int64_t ldo, void* stream) {
    TTSC_REQUIRE(frames_in_dev && tables_dev && out_dev, "ttsc_stft_overlap_add: null pointer");
    if (int rc = check_common("ttsc_stft_overlap_add", B, Fmax, n_fft, hop, frames_host, frames_dev)) return rc;
    const int64_t want = (int64_t)hop * (Fmax - 1) + (padded ? n_fft : 0);
    TTSC_REQUIRE(ldo == want, "ttsc_stft_overlap_add: ldo=%lld, the %s form has %lld samples per row", (long long)ldo, padded ? "padded" : "trimmed",
                 (long long)want);
    hipLaunchKernelGGL(stft_ola_kernel, dim3(ola_grid(ldo), (unsigned)B), dim3(256), 0, (hipStream_t)stream, frames_in_dev, frames_dev, Fmax, n_fft, hop,
                       tables_dev + 2 * n_fft, padded, out_dev, (long)ldo);
    TTSC_LAUNCH_CHECK("stft_ola_kernel");
    return TTSC_OK;
}
