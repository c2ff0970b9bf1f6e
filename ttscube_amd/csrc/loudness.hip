// Loudness meter of io_utils/loudness.py: ITU-R BS.1770-4 K-weighted sub-block energies, sample peak and 4x true peak of a ragged batch, the two
// gates with the static gain, and the gain stage.  tests/loudness_reference.py is the float64 statement.
//
// The K-weighting is a cascade of two transposed direct-form-II biquads, a linear system with a 4-vector state s kept in float64:
//
//     u = b0 x + s1;   s1 = (b1 x - a1 u) + s2;   s2 = b2 x - a2 u          (shelf, then the same on u for the high-pass -> y)
//
// Its high-pass poles sit at 0.99 at 24 kHz, so a row cannot be cut into pieces with a warm-up; it is cut exactly.  A thread owns LOUD_CHUNK = 64
// consecutive samples, a 256-thread workgroup a tile of LOUD_TILE = 16384, tiles counted from the row's own first sample.  With A the 4x4 matrix
// of one step at x = 0, the state behind a chunk entered with s is A^64 s + f, f being the state the chunk leaves when entered with zero:
//
//   loud_tile_state   every thread runs its chunk from zero; a Hillis-Steele scan over the workgroup (level k: F_i = A^(64 2^k) F_(i - 2^k) + F_i,
//                     the matrix powers made on the host in float64) leaves in F_255 what the tile adds to the state: f_t, one 4-vector per tile
//   loud_row_scan     one thread per row: S_0 = 0, S_(t+1) = A^TILE S_t + f_t, written over f_t.  Exact, linear in the number of tiles
//   loud_energy       thread 0 enters its chunk with S_t, the others with zero; the same scan now leaves the TRUE state behind every chunk; each
//                     thread filters its chunk again from the state of its left neighbour and sums y^2 on either side of the one sub-block
//                     boundary (sub-blocks are sr / 10 >= 64 samples) its chunk can hold.  Per sub-block the partial sums of the tile are added
//                     in thread order
//   loud_combine      per sub-block, the tile partials in tile order
//
// No floating-point atomics; every sum has one fixed order that depends on the position inside the row alone, so a row has the same bits alone,
// anywhere in any batch, and behind any padding.  Samples behind a row's length are never read (they filter as zeros and are not summed).
// The build has -ffp-contract=off and the recursion is written with separate products and sums: each operation rounds once, as in numpy.
//
// loud_peak is a launch of its own: one input sample per lane (coalesced, the 20-sample halo in LDS), the four phases of the project's 4x
// polyphase filter (resample.design_filter(4, 1) as float32, 21 taps per phase, zeros outside the row) as float32 FMAs in one fixed order, |.|
// maxima through a workgroup reduction and one integer atomic max on the bits of the non-negative float.  The recurrence launches map 64 samples
// to a lane and run a dependent float64 chain at 4 waves per workgroup; the FIR wants the opposite mapping.  The five launches of a measure call
// run one after the other on the caller's stream.  The 4x signal is never stored.
#include "common.hpp"

#include <cmath>

namespace ttsc {

constexpr int LOUD_CHUNK = 64;                          // samples per thread (io_utils/loudness.py::CHUNK)
constexpr int LOUD_THREADS = 256;
constexpr int LOUD_TILE = LOUD_CHUNK * LOUD_THREADS;    // samples per workgroup (io_utils/loudness.py::TILE)
constexpr int LOUD_LEVELS = 8;                          // log2(LOUD_THREADS)
constexpr int LOUD_PEAK_TILE = 1024;                    // samples per workgroup of loud_peak
constexpr int LOUD_TP_HALF = 10;                        // the 4x filter reaches 10 input samples to either side
constexpr int LOUD_TP_TAPS = 2 * LOUD_TP_HALF + 1;

struct LoudCoef {                                       // by value in the kernel arguments
    double sos[2][5];                                   // b0 b1 b2 a1 a2 of the shelf and of the high-pass
    double P[LOUD_LEVELS + 1][16];                      // A^(CHUNK 2^k) row-major, k = 0 .. 8 (k = 8: A^TILE)
};
struct LoudTaps {
    float h[4][LOUD_TP_TAPS];                           // h[p][d + 10] = fl32(design_filter(4, 1)[4 d + p + 40]), 0 where that index is outside
};

struct LoudState {
    double v[4];
};

__device__ __forceinline__ double loud_step(const LoudCoef& c, LoudState& s, double x) {
    const double u = c.sos[0][0] * x + s.v[0];
    s.v[0] = (c.sos[0][1] * x - c.sos[0][3] * u) + s.v[1];
    s.v[1] = c.sos[0][2] * x - c.sos[0][4] * u;
    const double y = c.sos[1][0] * u + s.v[2];
    s.v[2] = (c.sos[1][1] * u - c.sos[1][3] * y) + s.v[3];
    s.v[3] = c.sos[1][2] * u - c.sos[1][4] * y;
    return y;
}

// r = M v + w, each row ((m0 v0 + m1 v1) + m2 v2) + m3 v3, then + w
__device__ __forceinline__ LoudState loud_affine(const double* M, const LoudState& v, const LoudState& w) {
    LoudState r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r.v[i] = (((M[4 * i] * v.v[0] + M[4 * i + 1] * v.v[1]) + M[4 * i + 2] * v.v[2]) + M[4 * i + 3] * v.v[3]) + w.v[i];
    return r;
}

// the thread's 64 samples, zeros from the row's end on: 16-byte loads when the chunk lies inside the row and its address allows
__device__ __forceinline__ void loud_load_chunk(const float* __restrict__ xb, long long c0, long long L, float (&xv)[LOUD_CHUNK]) {
    const float* p = xb + c0;
    if (c0 + LOUD_CHUNK <= L && (reinterpret_cast<size_t>(p) & 15) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int j = 0; j < LOUD_CHUNK / 4; ++j) {
            const float4 q = p4[j];
            xv[4 * j] = q.x;
            xv[4 * j + 1] = q.y;
            xv[4 * j + 2] = q.z;
            xv[4 * j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LOUD_CHUNK; ++j) xv[j] = c0 + j < L ? p[j] : 0.f;
    }
}

// inclusive scan of the chunk states over the workgroup: on return F[tid] is the state behind chunk tid given the state thread 0 entered with
__device__ __forceinline__ LoudState loud_scan(const LoudCoef& c, LoudState f, LoudState (*buf)[LOUD_THREADS]) {
    const int tid = threadIdx.x;
    int cur = 0;
    buf[0][tid] = f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LOUD_LEVELS; ++k) {
        const int off = 1 << k;
        if (tid >= off) f = loud_affine(c.P[k], buf[cur][tid - off], f);
        buf[cur ^ 1][tid] = f;
        cur ^= 1;
        __syncthreads();
    }
    return f;                                            // (buf[cur] holds every thread's F)
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_tile_state(const float* __restrict__ x, const int* __restrict__ len, long long Lmax,
                                                                long long tiles, LoudCoef c, double* __restrict__ states) {
    __shared__ LoudState buf[2][LOUD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long t = blockIdx.x, t0 = t * LOUD_TILE;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    if (t0 + LOUD_TILE >= L) return;                     // (uniform) no tile follows this one inside the row: nobody reads its f_t
    const float* xb = x + (size_t)b * (size_t)Lmax;
    float xv[LOUD_CHUNK];
    loud_load_chunk(xb, t0 + (long long)tid * LOUD_CHUNK, L, xv);
    LoudState s = {{0., 0., 0., 0.}};
#pragma unroll
    for (int j = 0; j < LOUD_CHUNK; ++j) loud_step(c, s, (double)xv[j]);
    s = loud_scan(c, s, buf);
    if (tid == LOUD_THREADS - 1) {
        double* o = states + ((size_t)b * (size_t)tiles + (size_t)t) * 4;
        o[0] = s.v[0], o[1] = s.v[1], o[2] = s.v[2], o[3] = s.v[3];
    }
}

__global__ __launch_bounds__(64) void loud_row_scan(const int* __restrict__ len, int B, long long Lmax, long long tiles, LoudCoef c,
                                                    double* __restrict__ states) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const long long nt = (L + LOUD_TILE - 1) / LOUD_TILE;
    double* o = states + (size_t)b * (size_t)tiles * 4;
    LoudState S = {{0., 0., 0., 0.}};
    for (long long t = 0; t < nt; ++t, o += 4) {
        LoudState f = {{0., 0., 0., 0.}};
        const bool more = t + 1 < nt;
        if (more) f.v[0] = o[0], f.v[1] = o[1], f.v[2] = o[2], f.v[3] = o[3];
        o[0] = S.v[0], o[1] = S.v[1], o[2] = S.v[2], o[3] = S.v[3];
        if (more) S = loud_affine(c.P[LOUD_LEVELS], S, f);
    }
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_energy(const float* __restrict__ x, const int* __restrict__ len, long long Lmax,
                                                            long long tiles, int S, int spt, LoudCoef c, const double* __restrict__ states,
                                                            double* __restrict__ part) {
    __shared__ LoudState buf[2][LOUD_THREADS];
    __shared__ double e[LOUD_THREADS][2];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long t = blockIdx.x, t0 = t * LOUD_TILE;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    if (t0 >= L) return;                                  // (uniform) a tile behind the row's end
    const float* xb = x + (size_t)b * (size_t)Lmax;
    const long long c0 = t0 + (long long)tid * LOUD_CHUNK;
    float xv[LOUD_CHUNK];
    loud_load_chunk(xb, c0, L, xv);
    LoudState s = {{0., 0., 0., 0.}};
    if (tid == 0) {
        const double* in = states + ((size_t)b * (size_t)tiles + (size_t)t) * 4;
        s.v[0] = in[0], s.v[1] = in[1], s.v[2] = in[2], s.v[3] = in[3];
    }
    const LoudState s_in0 = s;
#pragma unroll
    for (int j = 0; j < LOUD_CHUNK; ++j) loud_step(c, s, (double)xv[j]);
    loud_scan(c, s, buf);
    // LOUD_LEVELS is even: the scan's last write went to buf[0]
    s = tid == 0 ? s_in0 : buf[LOUD_LEVELS & 1][tid - 1];

    const long long k0 = c0 / S;                          // sub-block of the chunk's first sample
    const long long nb = (k0 + 1) * (long long)S - c0;    // samples of the chunk before the boundary (>= 64: none inside)
    const long long nv = L - c0;                          // samples of the chunk inside the row (may be <= 0)
    double lo = 0., hi = 0.;
#pragma unroll
    for (int j = 0; j < LOUD_CHUNK; ++j) {
        const double y = loud_step(c, s, (double)xv[j]);
        const double q = y * y;
        if (j < nv) {
            if (j < nb)
                lo = lo + q;
            else
                hi = hi + q;
        }
    }
    e[tid][0] = lo;
    e[tid][1] = hi;
    __syncthreads();

    const long long tend = t0 + LOUD_TILE < L ? t0 + LOUD_TILE : L;   // end of the tile inside the row
    const long long kf = t0 / S, kl = (tend - 1) / S;
    double* pb = part + ((size_t)b * (size_t)tiles + (size_t)t) * (size_t)spt;
    for (long long j = tid; j <= kl - kf && j < spt; j += LOUD_THREADS) {
        const long long k = kf + j;
        const long long a0 = k * S > t0 ? k * S : t0, a1 = (k + 1) * S < tend ? (k + 1) * S : tend;
        const int i0 = (int)((a0 - t0) / LOUD_CHUNK), i1 = (int)((a1 - 1 - t0) / LOUD_CHUNK);
        double acc = 0.;
        for (int i = i0; i <= i1; ++i) {
            const long long ki = (t0 + (long long)i * LOUD_CHUNK) / S;
            acc = acc + e[i][k == ki ? 0 : 1];
        }
        pb[j] = acc;
    }
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_combine(const int* __restrict__ len, long long Lmax, long long tiles, int S, int spt,
                                                             const double* __restrict__ part, double* __restrict__ sub, long long nsub_max) {
    const int b = blockIdx.y;
    const long long k = (long long)blockIdx.x * LOUD_THREADS + threadIdx.x;
    if (k >= nsub_max) return;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    double acc = 0.;
    if (k * S < L) {
        const long long a1 = (k + 1) * S < L ? (k + 1) * S : L;
        const long long tf = k * S / LOUD_TILE, tl = (a1 - 1) / LOUD_TILE;
        for (long long t = tf; t <= tl; ++t) {
            const long long j = k - t * LOUD_TILE / S;
            acc = acc + part[((size_t)b * (size_t)tiles + (size_t)t) * (size_t)spt + (size_t)j];
        }
    }
    sub[(size_t)b * (size_t)nsub_max + (size_t)k] = acc;
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_peak(const float* __restrict__ x, const int* __restrict__ len, long long Lmax, LoudTaps taps,
                                                          unsigned* __restrict__ sample_peak, unsigned* __restrict__ true_peak) {
    __shared__ float xs[LOUD_PEAK_TILE + 2 * LOUD_TP_HALF];
    __shared__ float red[2][LOUD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * LOUD_PEAK_TILE;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    if (m0 >= L) return;
    const float* xb = x + (size_t)b * (size_t)Lmax;
    for (int s = tid; s < LOUD_PEAK_TILE + 2 * LOUD_TP_HALF; s += LOUD_THREADS) {
        const long long i = m0 - LOUD_TP_HALF + s;
        xs[s] = (i >= 0 && i < L) ? xb[i] : 0.f;
    }
    __syncthreads();
    float sp = 0.f, tp = 0.f;
    for (int r = 0; r < LOUD_PEAK_TILE / LOUD_THREADS; ++r) {
        const int ml = r * LOUD_THREADS + tid;            // sample m0 + ml; xs[ml + 10 - d] = x[m - d]
        if (m0 + ml >= L) break;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int d = -LOUD_TP_HALF; d <= LOUD_TP_HALF; ++d) {
            const float v = xs[ml + LOUD_TP_HALF - d];
            a0 = fmaf(v, taps.h[0][d + LOUD_TP_HALF], a0);
            a1 = fmaf(v, taps.h[1][d + LOUD_TP_HALF], a1);
            a2 = fmaf(v, taps.h[2][d + LOUD_TP_HALF], a2);
            a3 = fmaf(v, taps.h[3][d + LOUD_TP_HALF], a3);
        }
        sp = fmaxf(sp, fabsf(xs[ml + LOUD_TP_HALF]));
        tp = fmaxf(tp, fmaxf(fmaxf(fabsf(a0), fabsf(a1)), fmaxf(fabsf(a2), fabsf(a3))));
    }
    red[0][tid] = sp;
    red[1][tid] = tp;
    __syncthreads();
    for (int off = LOUD_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] = fmaxf(red[0][tid], red[0][tid + off]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + off]);
        }
        __syncthreads();
    }
    if (tid == 0) {                                       // bits of non-negative floats order as unsigned integers
        atomicMax(sample_peak + b, __float_as_uint(red[0][0]));
        atomicMax(true_peak + b, __float_as_uint(red[1][0]));
    }
}

// g = sqrt(target / zbar), held under peak_lin / max(sample peak, true peak) and under max_gain (when > 0); 1 for a silent row
__device__ __forceinline__ void loud_gain(double zbar, float sp, float tp, bool silent, double target_e, double peak_lin, double max_gain,
                                          float* gain, int* limited) {
    double g = 1.;
    int lim = 0;
    if (!silent) {
        g = sqrt(target_e / zbar);
        const double pk = (double)(sp > tp ? sp : tp);
        if (pk > 0.) {
            const double ceil_g = peak_lin / pk;
            if (ceil_g < g) g = ceil_g, lim = 1;
        }
        if (max_gain > 0. && max_gain < g) g = max_gain;
    }
    *gain = (float)g;
    if (limited) *limited = lim;
}

// z_j of row with nsub sub-blocks e[]: 400 ms blocks at a 100 ms step, or the one short block
__device__ __forceinline__ double loud_block(const double* __restrict__ e, long long j, long long L, int S, bool shortrow, long long nsub) {
    if (shortrow) {
        double a = 0.;
        for (long long k = 0; k < nsub; ++k) a = a + e[k];
        return a / (double)L;
    }
    return (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / (4. * (double)S);
}

// fixed-order workgroup sum of (value, count): strided per-thread partials, then a halving tree
__device__ __forceinline__ void loud_reduce(double& v, long long& n, double* rv, long long* rn) {
    const int tid = threadIdx.x;
    rv[tid] = v;
    rn[tid] = n;
    __syncthreads();
    for (int off = LOUD_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) rv[tid] = rv[tid] + rv[tid + off], rn[tid] += rn[tid + off];
        __syncthreads();
    }
    v = rv[0];
    n = rn[0];
    __syncthreads();
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_finish(const double* __restrict__ sub, const int* __restrict__ len, long long Lmax,
                                                            long long nsub_max, int S, const float* __restrict__ sample_peak,
                                                            const float* __restrict__ true_peak, double abs_gate,
                                                            const double* __restrict__ target_e, const double* __restrict__ peak_lin,
                                                            double max_gain, double* __restrict__ zbar, int* __restrict__ blocks,
                                                            int* __restrict__ gated, int* __restrict__ silent, float* __restrict__ gain,
                                                            int* __restrict__ limited) {
    __shared__ double rv[LOUD_THREADS];
    __shared__ long long rn[LOUD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const double* e = sub + (size_t)b * (size_t)nsub_max;
    const long long nsub = (L + S - 1) / S;
    const bool shortrow = L > 0 && L < 4ll * S;
    const long long nblk = L == 0 ? 0 : (shortrow ? 1 : L / S - 3);

    double v = 0.;
    long long n = 0;
    for (long long j = tid; j < nblk; j += LOUD_THREADS) {
        const double z = loud_block(e, j, L, S, shortrow, nsub);
        if (z > abs_gate) v = v + z, ++n;
    }
    loud_reduce(v, n, rv, rn);
    double zb = 0.;
    long long ng = 0;
    if (n > 0) {
        const double rel = 0.1 * (v / (double)n);
        v = 0., n = 0;
        for (long long j = tid; j < nblk; j += LOUD_THREADS) {
            const double z = loud_block(e, j, L, S, shortrow, nsub);
            if (z > abs_gate && z > rel) v = v + z, ++n;
        }
        loud_reduce(v, n, rv, rn);
        ng = n;
        if (ng > 0) zb = v / (double)ng;
    }
    if (tid == 0) {
        const bool sil = ng == 0;
        zbar[b] = zb;
        blocks[b] = (int)nblk;
        gated[b] = (int)ng;
        silent[b] = sil ? 1 : 0;
        if (gain) loud_gain(zb, sample_peak[b], true_peak[b], sil, target_e[b], peak_lin[b], max_gain, gain + b, limited ? limited + b : nullptr);
    }
}

__global__ __launch_bounds__(LOUD_THREADS) void loud_gain_kernel(const double* __restrict__ zbar, const float* __restrict__ sample_peak,
                                                                 const float* __restrict__ true_peak, const int* __restrict__ silent,
                                                                 const double* __restrict__ target_e, const double* __restrict__ peak_lin,
                                                                 double max_gain, int B, float* __restrict__ gain, int* __restrict__ limited) {
    const int b = blockIdx.x * LOUD_THREADS + threadIdx.x;
    if (b >= B) return;
    loud_gain(zbar[b], sample_peak[b], true_peak[b], silent[b] != 0, target_e[b], peak_lin[b], max_gain, gain + b, limited ? limited + b : nullptr);
}

// y = fl32(g x) on [0, len): four elements per thread, as one 16-byte load and store where both rows allow it at that position
__global__ __launch_bounds__(LOUD_THREADS) void loud_apply(const float* x, const int* __restrict__ len, const float* __restrict__ gain,
                                                           long long Lmax, float* y) {
    const int b = blockIdx.y;
    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const float* xb = x + (size_t)b * (size_t)Lmax;
    float* yb = y + (size_t)b * (size_t)Lmax;
    const int mis = (int)((reinterpret_cast<size_t>(xb) >> 2) & 3);        // floats past a 16-byte boundary
    const bool vec = ((reinterpret_cast<size_t>(xb) ^ reinterpret_cast<size_t>(yb)) & 15) == 0;
    const long long n0 = ((long long)blockIdx.x * LOUD_THREADS + threadIdx.x) * 4 - mis;
    if (n0 >= L) return;
    const float g = gain[b];
    if (vec && n0 >= 0 && n0 + 4 <= L) {
        float4 q = *reinterpret_cast<const float4*>(xb + n0);
        q.x = __fmul_rn(g, q.x);
        q.y = __fmul_rn(g, q.y);
        q.z = __fmul_rn(g, q.z);
        q.w = __fmul_rn(g, q.w);
        *reinterpret_cast<float4*>(yb + n0) = q;
    } else {
        for (int j = 0; j < 4; ++j) {
            const long long n = n0 + j;
            if (n >= 0 && n < L) yb[n] = __fmul_rn(g, xb[n]);
        }
    }
}

static bool loud_rate_ok(int32_t sr) { return sr > 0 && sr % 10 == 0 && sr / 10 >= LOUD_CHUNK; }

}  // namespace ttsc

using namespace ttsc;

extern "C" size_t ttsc_loudness_workspace_bytes(int32_t B, int64_t Lmax, int32_t sr) {
    if (B <= 0 || Lmax <= 0 || !loud_rate_ok(sr)) return 0;
    const int64_t tiles = ceil_div(Lmax, LOUD_TILE), spt = LOUD_TILE / (sr / 10) + 2;
    return (size_t)B * (size_t)tiles * (size_t)(4 + spt) * sizeof(double);
}

extern "C" int ttsc_loudness_measure(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t sr, const double* kweight_host,
                                     const float* taps_host, double* sub_dev, int64_t nsub_max, float* sample_peak_dev, float* true_peak_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
    TTSC_REQUIRE(loud_rate_ok(sr), "ttsc_loudness_measure: sr=%d: the rate must be a positive multiple of 10 with sr / 10 >= %d (100 ms sub-blocks of "
                 "whole samples, no shorter than a chunk)", sr, LOUD_CHUNK);
    TTSC_REQUIRE(B > 0 && B <= 65535 && Lmax > 0 && Lmax < (int64_t)1 << 31, "ttsc_loudness_measure: bad sizes (B=%d Lmax=%lld)", B, (long long)Lmax);
    TTSC_REQUIRE(x_dev && len_dev && kweight_host && taps_host && sub_dev && sample_peak_dev && true_peak_dev && workspace_dev,
                 "ttsc_loudness_measure: null argument");
    const int S = sr / 10;
    const int64_t need = ceil_div(Lmax, S);
    TTSC_REQUIRE(nsub_max >= need, "ttsc_loudness_measure: nsub_max=%lld is fewer than the %lld sub-blocks of a row of Lmax=%lld samples at sr=%d",
                 (long long)nsub_max, (long long)need, (long long)Lmax, sr);
    TTSC_REQUIRE(workspace_bytes >= ttsc_loudness_workspace_bytes(B, Lmax, sr), "ttsc_loudness_measure: workspace of %zu bytes, %zu needed",
                 workspace_bytes, ttsc_loudness_workspace_bytes(B, Lmax, sr));
    TTSC_REQUIRE((reinterpret_cast<size_t>(workspace_dev) & 7) == 0 && (reinterpret_cast<size_t>(sub_dev) & 7) == 0,
                 "ttsc_loudness_measure: misaligned float64 buffer");
    LoudCoef c;
    LoudTaps taps;
    memcpy(&c, kweight_host, sizeof(c));
    memcpy(&taps, taps_host, sizeof(taps));
    for (size_t i = 0; i < sizeof(c) / sizeof(double); ++i)
        TTSC_REQUIRE(std::isfinite(reinterpret_cast<const double*>(&c)[i]), "ttsc_loudness_measure: non-finite filter constant %zu", i);
    const int64_t tiles = ceil_div(Lmax, LOUD_TILE), spt = LOUD_TILE / S + 2;
    double* states = static_cast<double*>(workspace_dev);
    double* part = states + (size_t)B * (size_t)tiles * 4;
    hipStream_t st = (hipStream_t)stream;
    TTSC_HIP_CHECK(hipMemsetAsync(sample_peak_dev, 0, (size_t)B * sizeof(float), st));
    TTSC_HIP_CHECK(hipMemsetAsync(true_peak_dev, 0, (size_t)B * sizeof(float), st));
    const dim3 grid((unsigned)tiles, (unsigned)B), block(LOUD_THREADS);
    int rc;
    if (tiles > 1) {
        hipLaunchKernelGGL(loud_tile_state, grid, block, 0, st, x_dev, len_dev, (long long)Lmax, (long long)tiles, c, states);
        if ((rc = launch_checked("loud_tile_state")) != TTSC_OK) return rc;
    }
    hipLaunchKernelGGL(loud_row_scan, dim3((unsigned)ceil_div(B, 64)), dim3(64), 0, st, len_dev, B, (long long)Lmax, (long long)tiles, c, states);
    if ((rc = launch_checked("loud_row_scan")) != TTSC_OK) return rc;
    hipLaunchKernelGGL(loud_energy, grid, block, 0, st, x_dev, len_dev, (long long)Lmax, (long long)tiles, S, (int)spt, c, states, part);
    if ((rc = launch_checked("loud_energy")) != TTSC_OK) return rc;
    hipLaunchKernelGGL(loud_combine, dim3((unsigned)ceil_div(nsub_max, LOUD_THREADS), (unsigned)B), block, 0, st, len_dev, (long long)Lmax,
                       (long long)tiles, S, (int)spt, part, sub_dev, (long long)nsub_max);
    if ((rc = launch_checked("loud_combine")) != TTSC_OK) return rc;
    hipLaunchKernelGGL(loud_peak, dim3((unsigned)ceil_div(Lmax, LOUD_PEAK_TILE), (unsigned)B), block, 0, st, x_dev, len_dev, (long long)Lmax, taps,
                       reinterpret_cast<unsigned*>(sample_peak_dev), reinterpret_cast<unsigned*>(true_peak_dev));
    return launch_checked("loud_peak");
}

extern "C" int ttsc_loudness_finish(const double* sub_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int64_t nsub_max, int32_t sr,
                                    const float* sample_peak_dev, const float* true_peak_dev, double abs_gate, const double* target_energy_dev,
                                    const double* peak_lin_dev, double max_gain_lin, double* zbar_dev, int32_t* blocks_dev, int32_t* gated_dev,
                                    int32_t* silent_dev, float* gain_dev, int32_t* limited_dev, void* stream) {
    TTSC_REQUIRE(loud_rate_ok(sr), "ttsc_loudness_finish: sr=%d: the rate must be a positive multiple of 10 with sr / 10 >= %d", sr, LOUD_CHUNK);
    TTSC_REQUIRE(B > 0 && B <= 65535 && Lmax > 0 && Lmax < (int64_t)1 << 31, "ttsc_loudness_finish: bad sizes (B=%d Lmax=%lld)", B, (long long)Lmax);
    TTSC_REQUIRE(nsub_max >= ceil_div(Lmax, sr / 10), "ttsc_loudness_finish: nsub_max=%lld is fewer than the sub-blocks of Lmax=%lld samples",
                 (long long)nsub_max, (long long)Lmax);
    TTSC_REQUIRE(sub_dev && len_dev && zbar_dev && blocks_dev && gated_dev && silent_dev, "ttsc_loudness_finish: null argument");
    TTSC_REQUIRE(abs_gate >= 0. && std::isfinite(abs_gate), "ttsc_loudness_finish: the absolute gate must be a finite energy >= 0");
    if (gain_dev) {
        TTSC_REQUIRE(sample_peak_dev && true_peak_dev && target_energy_dev && peak_lin_dev,
                     "ttsc_loudness_finish: a gain needs the peaks, the target energies and the peak ceilings");
        TTSC_REQUIRE(!std::isnan(max_gain_lin), "ttsc_loudness_finish: max_gain_lin is NaN (<= 0 means none)");
    } else {
        TTSC_REQUIRE(!limited_dev, "ttsc_loudness_finish: limited_dev without gain_dev");
    }
    hipLaunchKernelGGL(loud_finish, dim3((unsigned)B), dim3(LOUD_THREADS), 0, (hipStream_t)stream, sub_dev, len_dev, (long long)Lmax,
                       (long long)nsub_max, sr / 10, sample_peak_dev, true_peak_dev, abs_gate, target_energy_dev, peak_lin_dev, max_gain_lin, zbar_dev,
                       blocks_dev, gated_dev, silent_dev, gain_dev, limited_dev);
    return launch_checked("loud_finish");
}

extern "C" int ttsc_loudness_gain(const double* zbar_dev, const float* sample_peak_dev, const float* true_peak_dev, const int32_t* silent_dev,
                                  const double* target_energy_dev, const double* peak_lin_dev, double max_gain_lin, int32_t B, float* gain_dev,
                                  int32_t* limited_dev, void* stream) {
    TTSC_REQUIRE(B > 0, "ttsc_loudness_gain: B=%d", B);
    TTSC_REQUIRE(zbar_dev && sample_peak_dev && true_peak_dev && silent_dev && target_energy_dev && peak_lin_dev && gain_dev,
                 "ttsc_loudness_gain: null argument");
    TTSC_REQUIRE(!std::isnan(max_gain_lin), "ttsc_loudness_gain: max_gain_lin is NaN (<= 0 means none)");
    hipLaunchKernelGGL(loud_gain_kernel, dim3((unsigned)ceil_div(B, LOUD_THREADS)), dim3(LOUD_THREADS), 0, (hipStream_t)stream, zbar_dev,
                       sample_peak_dev, true_peak_dev, silent_dev, target_energy_dev, peak_lin_dev, max_gain_lin, B, gain_dev, limited_dev);
    return launch_checked("loud_gain_kernel");
}

extern "C" int ttsc_loudness_apply(const float* x_dev, const int32_t* len_dev, const float* gain_dev, int32_t B, int64_t Lmax, float* y_dev,
                                   void* stream) {
    TTSC_REQUIRE(B > 0 && B <= 65535 && Lmax > 0 && Lmax < (int64_t)1 << 31, "ttsc_loudness_apply: bad sizes (B=%d Lmax=%lld)", B, (long long)Lmax);
    TTSC_REQUIRE(x_dev && len_dev && gain_dev && y_dev, "ttsc_loudness_apply: null argument");
    TTSC_REQUIRE((reinterpret_cast<size_t>(x_dev) & 3) == 0 && (reinterpret_cast<size_t>(y_dev) & 3) == 0, "ttsc_loudness_apply: misaligned float buffer");
    const int64_t groups = ceil_div(Lmax + 3, 4);
    hipLaunchKernelGGL(loud_apply, dim3((unsigned)ceil_div(groups, LOUD_THREADS), (unsigned)B), dim3(LOUD_THREADS), 0, (hipStream_t)stream, x_dev,
                       len_dev, gain_dev, (long long)Lmax, y_dev);
    return launch_checked("loud_apply");
}
