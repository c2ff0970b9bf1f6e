// Pitch tracker of the corpus importer (io_utils/pitch.py): a single-rate RAPT (Talkin 1995) in two launches for a whole batch of ragged utterances.
// The reference's importer calls pysptk.rapt per utterance on the host (scripts/import_textgrid.py:178); tests/pitch_reference.py is the float64
// statement of what is computed here.  VALU + LDS work and one latency chain: nothing here belongs on the matrix pipe.
//
//   ttsc_pitch_nccf    one workgroup per (utterance, group of PITCH_G consecutive frames).  The samples the group needs are staged once in LDS (frames
//                      of a group overlap: (G-1)*hop + n + kmax floats instead of G*(n + kmax)), then per frame: mean over n + kmax samples, the
//                      mean-removed frame, phi[k] = sum_j s[j] s[j+k] / sqrt(e_0 e_k + A) for every lag (threads stride over the lags; both sums
//                      are taken directly — a running prefix sum of squares cancels in float32), the frame's maximum, its peaks, and the 20 largest
//                      peaks by rank, refined by a parabola.  All from phi in LDS; phi goes to global memory only when the caller asks for it.
//   ttsc_pitch_track   one wave per utterance.  21 states (20 voiced candidates + unvoiced); lane 3j + s takes 7 of the 21 predecessors of state j,
//                      three lanes combine by shuffles.  Back-pointers go as bytes to a global workspace and are walked back in LDS-sized chunks.
#include "common.hpp"

namespace ttsc {

constexpr int PITCH_G = 8;            // frames per workgroup of the NCCF kernel
constexpr int PITCH_THREADS = 256;
constexpr int PITCH_NC = 20;          // voiced candidates per frame
constexpr int PITCH_NS = PITCH_NC + 1;
constexpr int PITCH_CHUNK = 128;      // frames of back-pointers walked per LDS refill
constexpr float PITCH_A = 10000.0f / (32768.0f * 32768.0f * 32768.0f * 32768.0f);
constexpr float PITCH_CAND_TR = 0.3f;
constexpr float PITCH_LAG_WT = 0.3f;
constexpr float PITCH_VOICE_BIAS = 0.0f;
constexpr float PITCH_FREQ_WT = 0.02f;
constexpr float PITCH_DOUBL_C = 0.35f;
constexpr float PITCH_TRANS_C = 0.005f;
constexpr float PITCH_TRANS_A = 0.5f;
constexpr float PITCH_RMS_EPS = 1e-6f;
constexpr float PITCH_LN2 = 0.69314718055994530942f;

// sum / max over the workgroup through red[PITCH_THREADS]; a fixed tree: the same bits every run
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int off = PITCH_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_max(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int off = PITCH_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmaxf(red[tid], red[tid + off]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// dynamic LDS: raw[(G-1)*hop + n + kmax] | s[n + kmax] | phi[K] | pk[K/2 + 1] (int) | red[PITCH_THREADS]
__global__ __launch_bounds__(PITCH_THREADS) void pitch_nccf_kernel(const float* __restrict__ x, const int* __restrict__ len, long long Lmax, int Fmax,
                                                                   int hop, int n, int kmin, int kmax, float* __restrict__ cand_lag,
                                                                   float* __restrict__ cand_val, int* __restrict__ ncand, float* __restrict__ maxphi,
                                                                   float* __restrict__ rms, float* __restrict__ phi_out) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * PITCH_G;
    const int K = kmax - kmin + 1, span = n + kmax, S = (PITCH_G - 1) * hop + span;
    float* raw = lds;
    float* s = raw + S;
    float* phi = s + span;
    int* pk = reinterpret_cast<int*>(phi + K);
    float* red = reinterpret_cast<float*>(pk + (K / 2 + 1));
    __shared__ int npk;

    long long L = len[b];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
    const int F = (int)(L / hop);
    const float* xb = x + (size_t)b * (size_t)Lmax;
    const long long g0 = (long long)t0 * hop;
    if (t0 < F)
        for (int j = tid; j < S; j += PITCH_THREADS) raw[j] = (g0 + j < L) ? xb[g0 + j] : 0.f;   // samples at or past L_b read as zero
    __syncthreads();

    for (int g = 0; g < PITCH_G; ++g) {
        const int t = t0 + g;
        if (t >= Fmax) break;                                 // (uniform over the workgroup)
        const size_t ft = (size_t)b * Fmax + t;
        if (t >= F) {                                         // a frame behind this utterance's end: defined, empty
            for (int c = tid; c < PITCH_NC; c += PITCH_THREADS) {
                cand_lag[ft * PITCH_NC + c] = 0.f;
                cand_val[ft * PITCH_NC + c] = 0.f;
            }
            if (phi_out)
                for (int i = tid; i < K; i += PITCH_THREADS) phi_out[ft * K + i] = 0.f;
            if (tid == 0) {
                ncand[ft] = 0;
                maxphi[ft] = 0.f;
                rms[ft] = 0.f;
            }
            continue;
        }
        const float* fr = raw + g * hop;
        float acc = 0.f;
        for (int j = tid; j < span; j += PITCH_THREADS) acc += fr[j];
        const float mean = block_sum(acc, red, tid) / (float)span;
        acc = 0.f;
        for (int j = tid; j < span; j += PITCH_THREADS) {
            const float v = fr[j] - mean;
            s[j] = v;
            if (j < n) acc = fmaf(v, v, acc);
        }
        const float e0 = block_sum(acc, red, tid);            // (its barriers also publish s[])

        float pmax = -INFINITY;
        for (int i = tid; i < K; i += PITCH_THREADS) {
            const float* sk = s + kmin + i;
            // eight partial sums per quantity: the rounding error of a sum of n terms stays near that of a pairwise sum, and the FMAs are independent
            float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, e[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int j = 0;
            for (; j + 8 <= n; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float a = s[j + u], c = sk[j + u];
                    d[u] = fmaf(a, c, d[u]);
                    e[u] = fmaf(c, c, e[u]);
                }
            }
            for (int u = 0; j < n; ++j, ++u) {
                const float a = s[j], c = sk[j];
                d[u] = fmaf(a, c, d[u]);
                e[u] = fmaf(c, c, e[u]);
            }
            const float num = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
            const float ek = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
            const float p = num / sqrtf(e0 * ek + PITCH_A);
            phi[i] = p;
            if (phi_out) phi_out[ft * K + i] = p;
            pmax = fmaxf(pmax, p);
        }
        if (tid == 0) npk = 0;
        pmax = block_max(pmax, red, tid);                     // (its barriers also publish phi[] and npk)

        const float thr = PITCH_CAND_TR * pmax;
        for (int i = 1 + tid; i < K - 1; i += PITCH_THREADS) {
            const float p = phi[i];
            if (p > phi[i - 1] && p >= phi[i + 1] && p >= thr) pk[atomicAdd(&npk, 1)] = i;   // at most K/2 peaks; their order in pk[] does not matter
        }
        __syncthreads();
        const int P = npk;
        for (int q = tid; q < P; q += PITCH_THREADS) {
            const int i = pk[q];
            const float p = phi[i];
            int rank = 0;                                     // peaks that come before this one: larger, or equal at a smaller lag
            for (int r = 0; r < P; ++r) {
                const int ir = pk[r];
                const float pr = phi[ir];
                rank += (pr > p || (pr == p && ir < i)) ? 1 : 0;
            }
            if (rank < PITCH_NC) {
                const float y0 = phi[i - 1], y2 = phi[i + 1];
                const float den = (y0 - p) + (y2 - p);        // < 0: p > y0 and p >= y2
                const float off = 0.5f * (y0 - y2) / den;
                cand_lag[ft * PITCH_NC + rank] = (float)(kmin + i) + off;
                cand_val[ft * PITCH_NC + rank] = p - 0.25f * (y0 - y2) * off;
            }
        }
        const int nc = P < PITCH_NC ? P : PITCH_NC;
        for (int c = nc + tid; c < PITCH_NC; c += PITCH_THREADS) {
            cand_lag[ft * PITCH_NC + c] = 0.f;
            cand_val[ft * PITCH_NC + c] = 0.f;
        }
        if (tid == 0) {
            ncand[ft] = nc;
            maxphi[ft] = pmax;
            rms[ft] = sqrtf(e0 / (float)n);
        }
        __syncthreads();                                      // s[], phi[], pk[] and npk are rewritten by the next frame
    }
}

// one wave per utterance; bp: [B, Fmax, 21] bytes
__global__ __launch_bounds__(64) void pitch_track_kernel(const float* __restrict__ cand_lag, const float* __restrict__ cand_val,
                                                         const int* __restrict__ ncand, const float* __restrict__ maxphi, const float* __restrict__ rms,
                                                         const int* __restrict__ nframes, int Fmax, float kmaxf, float sr, unsigned char* bp,
                                                         float* __restrict__ f0) {
    __shared__ float D[2][PITCH_NS];
    __shared__ float ll[2][PITCH_NS];
    __shared__ float loc[PITCH_NS];
    __shared__ unsigned char chunk[PITCH_CHUNK * PITCH_NS];
    __shared__ unsigned char st[PITCH_CHUNK];
    __shared__ int last_state;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int j = lane / 3, sub = lane - 3 * j;               // lane 63 (j = 21) only takes part in the shuffles
    int F = nframes[b];
    F = F < 0 ? 0 : (F > Fmax ? Fmax : F);
    const size_t fb = (size_t)b * Fmax;
    for (int t = F + lane; t < Fmax; t += 64) f0[fb + t] = 0.f;
    if (F == 0) return;
    unsigned char* bpb = bp + fb * PITCH_NS;

    // the tables of frame t + 1 are loaded while frame t is worked on
    float n_lag = 0.f, n_val = 0.f, n_mp, n_rms;
    int n_nc;
    if (lane < PITCH_NC) {
        n_lag = cand_lag[fb * PITCH_NC + lane];
        n_val = cand_val[fb * PITCH_NC + lane];
    }
    n_nc = ncand[fb];
    n_mp = maxphi[fb];
    n_rms = rms[fb];
    float rms_prev = 0.f;
    for (int t = 0; t < F; ++t) {
        const int cur = t & 1, prv = cur ^ 1;
        const float lag = n_lag, val = n_val, mp = n_mp, r = n_rms;
        int nc = n_nc;
        nc = nc < 0 ? 0 : (nc > PITCH_NC ? PITCH_NC : nc);
        if (t + 1 < F) {
            if (lane < PITCH_NC) {
                n_lag = cand_lag[(fb + t + 1) * PITCH_NC + lane];
                n_val = cand_val[(fb + t + 1) * PITCH_NC + lane];
            }
            n_nc = ncand[fb + t + 1];
            n_mp = maxphi[fb + t + 1];
            n_rms = rms[fb + t + 1];
        }
        if (lane < PITCH_NC) {
            const bool valid = lane < nc;
            ll[cur][lane] = valid ? logf(lag) : 0.f;          // accurate logf and divisions throughout: the test's bound leaves no room for fast ones
            loc[lane] = valid ? 1.0f - val * (1.0f - PITCH_LAG_WT * lag / kmaxf) : INFINITY;
        } else if (lane == PITCH_NC) {
            ll[cur][lane] = 0.f;
            loc[lane] = PITCH_VOICE_BIAS + mp;
        }
        __syncthreads();
        if (t == 0) {
            if (lane < PITCH_NS) D[cur][lane] = loc[lane];
        } else {
            const float rr = (r + PITCH_RMS_EPS) / (rms_prev + PITCH_RMS_EPS);
            const float uv = PITCH_TRANS_C + PITCH_TRANS_A / rr;   // unvoiced -> voiced
            const float vu = PITCH_TRANS_C + PITCH_TRANS_A * rr;   // voiced -> unvoiced
            float best = INFINITY;
            int bi = 0;
            if (j < PITCH_NS) {
                const float lj = ll[cur][j];
                for (int i = sub * 7; i < sub * 7 + 7; ++i) {
                    float tc;
                    if (j < PITCH_NC && i < PITCH_NC) {
                        const float d = lj - ll[prv][i];
                        tc = PITCH_FREQ_WT * fminf(fabsf(d), fminf(PITCH_DOUBL_C + fabsf(d - PITCH_LN2), PITCH_DOUBL_C + fabsf(d + PITCH_LN2)));
                    } else if (j < PITCH_NC) {
                        tc = uv;
                    } else if (i < PITCH_NC) {
                        tc = vu;
                    } else {
                        tc = 0.f;
                    }
                    const float c = D[prv][i] + tc;           // a state that does not exist carries +inf
                    if (c < best) {                           // strict: ties go to the lowest state
                        best = c;
                        bi = i;
                    }
                }
            }
            const float b1 = __shfl(best, (lane + 1) & 63), b2 = __shfl(best, (lane + 2) & 63);
            const int i1 = __shfl(bi, (lane + 1) & 63), i2 = __shfl(bi, (lane + 2) & 63);
            if (sub == 0 && j < PITCH_NS) {
                if (b1 < best) {
                    best = b1;
                    bi = i1;
                }
                if (b2 < best) {
                    best = b2;
                    bi = i2;
                }
                D[cur][j] = loc[j] + best;
                bpb[(size_t)t * PITCH_NS + j] = (unsigned char)bi;
            }
        }
        rms_prev = r;
        __syncthreads();
    }

    if (lane == 0) {
        const float* Df = D[(F - 1) & 1];
        float best = Df[0];
        int bi = 0;
        for (int i = 1; i < PITCH_NS; ++i)
            if (Df[i] < best) {
                best = Df[i];
                bi = i;
            }
        last_state = bi;
    }
    __threadfence();
    __syncthreads();
    for (int c1 = F; c1 > 0; c1 -= PITCH_CHUNK) {
        const int c0 = c1 > PITCH_CHUNK ? c1 - PITCH_CHUNK : 0;
        const int nb = (c1 - c0) * PITCH_NS;
        const int skip = c0 == 0 ? PITCH_NS : 0;              // frame 0 has no back-pointers
        for (int i = skip + lane; i < nb; i += 64) chunk[i] = bpb[(size_t)c0 * PITCH_NS + i];
        __syncthreads();
        if (lane == 0) {
            int state = last_state;
            for (int t = c1 - 1; t >= c0; --t) {
                st[t - c0] = (unsigned char)state;
                if (t > 0) state = chunk[(t - c0) * PITCH_NS + state];
            }
            last_state = state;
        }
        __syncthreads();
        for (int t = c0 + lane; t < c1; t += 64) {
            const int state = st[t - c0];
            f0[fb + t] = state < PITCH_NC ? sr / cand_lag[(fb + t) * PITCH_NC + state] : 0.f;
        }
        __syncthreads();
    }
}

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_pitch_nccf(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t hop, int32_t n, int32_t kmin, int32_t kmax,
                               float* cand_lag_dev, float* cand_val_dev, int32_t* ncand_dev, float* maxphi_dev, float* rms_dev, float* phi_dev,
                               void* stream) {
    TTSC_REQUIRE(x_dev && len_dev && cand_lag_dev && cand_val_dev && ncand_dev && maxphi_dev && rms_dev, "ttsc_pitch_nccf: null argument");
    TTSC_REQUIRE(B > 0 && B <= 65535 && Lmax > 0 && hop > 0 && n > 0 && kmin >= 1 && kmax >= kmin + 2,
                 "ttsc_pitch_nccf: bad sizes (B=%d Lmax=%lld hop=%d n=%d kmin=%d kmax=%d)", B, (long long)Lmax, hop, n, kmin, kmax);
    const int64_t Fmax = Lmax / hop;
    if (Fmax == 0) return TTSC_OK;                            // no frame in any utterance: nothing to write
    TTSC_REQUIRE(Fmax < (int64_t)1 << 30, "ttsc_pitch_nccf: too many frames (%lld)", (long long)Fmax);
    const int64_t K = kmax - kmin + 1, span = (int64_t)n + kmax, S = (int64_t)(PITCH_G - 1) * hop + span;
    const size_t lds = (size_t)(S + span + K + (K / 2 + 1) + PITCH_THREADS) * sizeof(float);
    TTSC_REQUIRE(lds <= 60 * 1024, "ttsc_pitch_nccf: hop / window / lag range need %zu bytes of LDS (limit 61440)", lds);
    hipLaunchKernelGGL(pitch_nccf_kernel, dim3((unsigned)ceil_div(Fmax, PITCH_G), (unsigned)B), dim3(PITCH_THREADS), lds, (hipStream_t)stream, x_dev,
                       len_dev, (long long)Lmax, (int)Fmax, hop, n, kmin, kmax, cand_lag_dev, cand_val_dev, ncand_dev, maxphi_dev, rms_dev, phi_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("pitch_nccf_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}

extern "C" size_t ttsc_pitch_track_workspace_bytes(int32_t B, int64_t Fmax) {
    if (B <= 0 || Fmax <= 0) return 0;
    return (size_t)B * (size_t)Fmax * PITCH_NS;
}

extern "C" int ttsc_pitch_track(const float* cand_lag_dev, const float* cand_val_dev, const int32_t* ncand_dev, const float* maxphi_dev,
                                const float* rms_dev, const int32_t* nframes_dev, int32_t B, int64_t Fmax, int32_t kmax, float sample_rate,
                                void* workspace_dev, size_t workspace_bytes, float* f0_dev, void* stream) {
    TTSC_REQUIRE(B > 0 && Fmax >= 0 && Fmax < (int64_t)1 << 30 && kmax > 0 && sample_rate > 0.f, "ttsc_pitch_track: bad sizes (B=%d Fmax=%lld kmax=%d)",
                 B, (long long)Fmax, kmax);
    if (Fmax == 0) return TTSC_OK;
    TTSC_REQUIRE(cand_lag_dev && cand_val_dev && ncand_dev && maxphi_dev && rms_dev && nframes_dev && f0_dev && workspace_dev,
                 "ttsc_pitch_track: null argument");
    TTSC_REQUIRE(workspace_bytes >= ttsc_pitch_track_workspace_bytes(B, Fmax), "ttsc_pitch_track: workspace of %zu bytes, %zu needed", workspace_bytes,
                 ttsc_pitch_track_workspace_bytes(B, Fmax));
    hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cand_lag_dev, cand_val_dev, ncand_dev, maxphi_dev, rms_dev,
                       nframes_dev, (int)Fmax, (float)kmax, sample_rate, (unsigned char*)workspace_dev, f0_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("pitch_track_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
