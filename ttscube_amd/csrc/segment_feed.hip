// Segment feed of the HiFi-GAN trainer (ttscube_amd/hifigan/train.py; io_utils/segment_feed.py): one training batch of random crops gathered from
// a device-resident corpus in ONE launch — instead of 2 B slices and two `cat`s, a permute and a scale.  Row b of the batch is utterance
// u = utt[b] from frame s = start_frame[b]:
//
//     y_out[b, 0, i]   = fl32(fl32(wav[wav_off[u] + s hop + i]) gain[u])           i < frames hop; 0 at and beyond wav_off[u + 1]
//     mel_out[b, c, t] = fl32(mel[(mel_off[u] + s + t) n_mels + c] mel_scale)      t < frames; mel_pad where s + t >= mel_off[u + 1] - mel_off[u]
//
// (tests/segment_feed_reference.py restates both in numpy.)  One float32 product per element: the int16 -> float conversion is exact and the
// 1/32768 of the int16 scale lives in gain[u], so a sample is rounded once.  Nothing is accumulated and there are no atomics: a row's bits do not
// depend on the batch around it.
//
// Memory-bound, and small: 2 B read + 4 B written per sample, 4 B + 4 B per mel element.  Workgroups (x, b) with x < audio_tiles convert audio,
// the others transpose mel (a uniform branch on blockIdx).
//   audio  a thread owns SEG_RUN = 8 consecutive samples.  Where the run lies inside the utterance and its first source sample sits on a 16-byte
//          boundary it is ONE 16-byte load of eight int16 (hop = 240 keeps s hop a multiple of 8, SegmentCorpus starts every utterance on a
//          multiple of 8: the usual case); otherwise eight bounds-checked 2-byte loads.  Where y_out's rows are 16-byte aligned (frames hop a
//          multiple of 4) the run leaves as two 16-byte stores, else sample by sample.
//   mel    the source is frame-major (the .mgc / GTA rows as they sit on disk), the generator wants channel-major.  A workgroup takes SEG_TF = 64
//          frames: they are ONE contiguous span of the arena, read in linear order (16 bytes per lane where n_mels is a multiple of 4) into an LDS
//          tile [64][n_mels | 1], then written in the linear order of the output, (c, t) -> c tf + t, which for frames <= 64 is the output row
//          itself.  The odd row pitch (81 words for n_mels = 80; banks are word address mod 32 for the 4-byte accesses used here) puts the 32
//          lanes of a group that read one channel's consecutive frames on 32 different banks; lanes that straddle two channels can meet 2-way.
//          The tile's stores are 4-byte too: consecutive lanes, consecutive words but for one skipped pad word per row — at most 2-way, which a
//          ds_write_b32 absorbs.
// All arena indexing is 64-bit.
#include "common.hpp"

namespace ttsc {

constexpr int SEG_RUN = 8;
constexpr int SEG_THREADS = 256;
constexpr int SEG_TILE = SEG_RUN * SEG_THREADS;     // audio samples per workgroup
constexpr int SEG_TF = 64;                          // mel frames per workgroup
constexpr int SEG_MAX_MELS = 255;                   // 64 x 255 words = 65 280 B of LDS

typedef short seg_short8 __attribute__((ext_vector_type(8)));

template <bool VEC_ST, bool VEC_MEL>
__global__ __launch_bounds__(SEG_THREADS) void segment_gather_kernel(const short* __restrict__ wav, const long long* __restrict__ wav_off,
                                                                     const float* __restrict__ gain, const float* __restrict__ mel,
                                                                     const long long* __restrict__ mel_off, const int* __restrict__ utt,
                                                                     const int* __restrict__ start_frame, int n_mels, int frames, int hop,
                                                                     float mel_scale, float mel_pad, int audio_tiles, float* __restrict__ y_out,
                                                                     float* __restrict__ mel_out) {
    extern __shared__ __attribute__((aligned(16))) float seg_tile[];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int u = utt[b];
    const long long s = start_frame[b];

    if ((int)blockIdx.x < audio_tiles) {                               // ---- audio (uniform) ----
        const long long n = (long long)frames * hop;                   // samples of a row
        const long long i0 = ((long long)blockIdx.x * SEG_THREADS + tid) * SEG_RUN;
        if (i0 >= n) return;
        const long long end = wav_off[u + 1];
        const long long src = wav_off[u] + s * hop + i0;
        const float g = gain[u];
        const int cnt = n - i0 >= SEG_RUN ? SEG_RUN : (int)(n - i0);
        float v[SEG_RUN];
        if (src + SEG_RUN <= end && (((uintptr_t)(wav + src)) & 15) == 0) {
            const seg_short8 w = *reinterpret_cast<const seg_short8*>(wav + src);
#pragma unroll
            for (int i = 0; i < SEG_RUN; ++i) v[i] = __fmul_rn((float)w[i], g);
        } else {
#pragma unroll
            for (int i = 0; i < SEG_RUN; ++i) v[i] = (i < cnt && src + i < end) ? __fmul_rn((float)wav[src + i], g) : 0.f;
        }
        float* dst = y_out + (long long)b * n + i0;
        if (VEC_ST && cnt == SEG_RUN) {                                // (n % 4 == 0, y_out 16-byte aligned, i0 % 8 == 0)
            reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
            reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
            for (int i = 0; i < SEG_RUN; ++i)
                if (i < cnt) dst[i] = v[i];
        }
        return;
    }

    // ---- mel: frames [t0, t0 + tf) of the row through the tile ----
    const int t0 = ((int)blockIdx.x - audio_tiles) * SEG_TF;
    const int tf = frames - t0 < SEG_TF ? frames - t0 : SEG_TF;
    const int pitch = n_mels | 1;
    const long long F = mel_off[u + 1] - mel_off[u];
    long long have = F - (s + t0);                                     // source frames this tile can take (the rest is mel_pad)
    have = have < 0 ? 0 : (have > tf ? tf : have);
    const float* span = mel + (mel_off[u] + s + t0) * (long long)n_mels;   // (only span[0 .. have n_mels) is read)
    const int total = tf * n_mels, valid = (int)have * n_mels;
    if (VEC_MEL) {                                                     // (n_mels % 4 == 0, the arena 16-byte aligned: so is every frame)
        for (int i = tid * 4; i < total; i += SEG_THREADS * 4) {
            const int t = i / n_mels, c = i - t * n_mels;
            float4 x = make_float4(mel_pad, mel_pad, mel_pad, mel_pad);
            if (i < valid) {
                x = *reinterpret_cast<const float4*>(span + i);
                x.x = __fmul_rn(x.x, mel_scale);
                x.y = __fmul_rn(x.y, mel_scale);
                x.z = __fmul_rn(x.z, mel_scale);
                x.w = __fmul_rn(x.w, mel_scale);
            }
            float* row = seg_tile + t * pitch + c;
            row[0] = x.x;
            row[1] = x.y;
            row[2] = x.z;
            row[3] = x.w;
        }
    } else {
        for (int i = tid; i < total; i += SEG_THREADS) {
            const int t = i / n_mels, c = i - t * n_mels;
            seg_tile[t * pitch + c] = i < valid ? __fmul_rn(span[i], mel_scale) : mel_pad;
        }
    }
    __syncthreads();
    float* out = mel_out + (long long)b * n_mels * frames + t0;
    for (int j = tid; j < total; j += SEG_THREADS) {
        const int c = j / tf, t = j - c * tf;
        out[(long long)c * frames + t] = seg_tile[t * pitch + c];
    }
}

}  // namespace ttsc

using namespace ttsc;

extern "C" int ttsc_segment_gather(const int16_t* wav_arena_dev, const int64_t* wav_off_dev, const float* gain_dev, const float* mel_arena_dev,
                                   const int64_t* mel_off_dev, const int32_t* utt_dev, const int32_t* start_frame_dev, int32_t B, int32_t n_mels,
                                   int32_t frames, int32_t hop, float mel_scale, float mel_pad, float* y_out_dev, float* mel_out_dev,
                                   void* stream) {
    TTSC_REQUIRE(B >= 1 && B <= 65535, "ttsc_segment_gather: B=%d is not in [1, 65535]", B);
    TTSC_REQUIRE(frames >= 1 && hop >= 1 && (int64_t)frames * hop < (int64_t)1 << 31, "ttsc_segment_gather: bad segment (frames=%d hop=%d)", frames, hop);
    TTSC_REQUIRE(wav_arena_dev && wav_off_dev && gain_dev && utt_dev && start_frame_dev && y_out_dev, "ttsc_segment_gather: null argument");
    TTSC_REQUIRE(((uintptr_t)wav_arena_dev & 1) == 0 && ((uintptr_t)y_out_dev & 3) == 0 && ((uintptr_t)mel_arena_dev & 3) == 0 &&
                     ((uintptr_t)mel_out_dev & 3) == 0,
                 "ttsc_segment_gather: a buffer is not aligned to its type");
    const bool with_mel = mel_arena_dev != nullptr;
    if (with_mel) {
        TTSC_REQUIRE(mel_off_dev && mel_out_dev, "ttsc_segment_gather: a mel arena without its offset table or its output");
        TTSC_REQUIRE(n_mels >= 1 && n_mels <= SEG_MAX_MELS, "ttsc_segment_gather: n_mels=%d is not in [1, %d]", n_mels, SEG_MAX_MELS);
        TTSC_REQUIRE((int64_t)n_mels * frames < (int64_t)1 << 31, "ttsc_segment_gather: n_mels=%d x frames=%d is too large", n_mels, frames);
    }
    const int64_t n = (int64_t)frames * hop;
    const int audio_tiles = (int)ceil_div(n, SEG_TILE);
    const int mel_tiles = with_mel ? (int)ceil_div(frames, SEG_TF) : 0;
    const size_t lds = with_mel ? (size_t)SEG_TF * (n_mels | 1) * sizeof(float) : 0;
    const dim3 grid((unsigned)(audio_tiles + mel_tiles), (unsigned)B), block(SEG_THREADS);
    const bool vec_st = n % 4 == 0 && ((uintptr_t)y_out_dev & 15) == 0;
    const bool vec_mel = with_mel && n_mels % 4 == 0 && ((uintptr_t)mel_arena_dev & 15) == 0;
#define TTSC_SEG_LAUNCH(VS, VM)                                                                                                                   \
    hipLaunchKernelGGL((segment_gather_kernel<VS, VM>), grid, block, lds, (hipStream_t)stream, (const short*)wav_arena_dev,                       \
                       (const long long*)wav_off_dev, gain_dev, mel_arena_dev, (const long long*)mel_off_dev, (const int*)utt_dev,               \
                       (const int*)start_frame_dev, (int)n_mels, (int)frames, (int)hop, mel_scale, mel_pad, audio_tiles, y_out_dev, mel_out_dev)
    if (vec_st && vec_mel)
        TTSC_SEG_LAUNCH(true, true);
    else if (vec_st)
        TTSC_SEG_LAUNCH(true, false);
    else if (vec_mel)
        TTSC_SEG_LAUNCH(false, true);
    else
        TTSC_SEG_LAUNCH(false, false);
#undef TTSC_SEG_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("segment_gather_kernel launch failed: %s", hipGetErrorString(e));
        return TTSC_EHIP;
    }
    return TTSC_OK;
}
