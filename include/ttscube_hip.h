/*
 * ttscube_hip.h — C ABI of libttscube_hip.so: the MI355X (gfx950) waveform-synthesis hot path of
 * TTS-Cube, hand-written HIP behind plain pointers and sizes (no torch types).
 *
 * The reference (tiberiu44/TTS-Cube) is 100 % Python and has no FFI; the boundary it exposes for this
 * path is `nn.Module.forward/inference` + the `state_dict` key layout.  Each entry point
 * below names the reference interface it replaces; `ttscube_amd/` (Python, ctypes) mirrors the
 * reference classes on top of these symbols and INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every function returns TTSC_OK (0) or a negative TTSC_E* code; ttsc_last_error() returns a
 *     thread-local, human-readable message for the last failure on the calling thread.
 *   - `*_dev` pointers are device (HBM) pointers owned by the caller and valid for the call;
 *     host pointers are copied before the function returns.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it, nothing synchronises the device unless stated.
 *   - handles are not thread-safe; distinct handles are independent.
 *   - activations are fp32, channel-major `[B, C, L]` contiguous (torch NCL), exactly what the
 *     reference modules exchange.
 */
#ifndef TTSCUBE_HIP_H
#define TTSCUBE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTSC_OK 0
#define TTSC_EINVAL (-1)   /* bad argument / shape / name */
#define TTSC_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define TTSC_ESTATE (-3)   /* weights missing / handle not ready */
#define TTSC_ENOMEM (-4)   /* workspace too small */
#define TTSC_ERANGE (-5)   /* split-precision generator: non-finite output even after re-calibration (non-finite input / weights) */

const char* ttsc_version(void);
const char* ttsc_last_error(void);
/* number of visible HIP devices, or negative error (used by the loader to fail loudly) */
int ttsc_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * Conv1d / ConvTranspose1d layer (fp32 MFMA implicit GEMM).
 * Replaces torch.nn.Conv1d / ConvTranspose1d as used by cube/networks/modules.py:37-55 (ConvNorm),
 * modules.py:117-145 (PostNet), modules.py:416-420 (WaveRNN low-res convs), textcoder.py:44-53 /
 * modules.py:850-871 (char CNN) and the [EXTERNAL] hifigan Generator convs (cubegan.py:43).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ttsc_conv1d ttsc_conv1d;

typedef struct {
    int32_t in_channels;
    int32_t out_channels;
    int32_t kernel_size;
    int32_t stride;      /* Conv1d: must be 1.  ConvTranspose1d: upsample factor */
    int32_t padding;
    int32_t dilation;    /* ConvTranspose1d: must be 1 */
    int32_t transposed;  /* 0 = Conv1d (weight [Cout,Cin,K]), 1 = ConvTranspose1d (weight [Cin,Cout,K]) */
    int32_t groups;      /* Conv1d only: torch's `groups` (weight [Cout, Cin/groups, K]); 0 or 1 = dense.  TTSC_PREC_FP32 only — the
                          * grouped k=41 layers of the multi-scale discriminator (training, row f1) */
} ttsc_conv1d_cfg;

enum { TTSC_ACT_NONE = 0, TTSC_ACT_TANH = 1, TTSC_ACT_RELU = 2, TTSC_ACT_SIGMOID = 3 };
/* arithmetic of the implicit GEMM: exact fp32 MFMA (k-ordered fmaf chain), or split precision — every fp32 value as
 * fp16 hi + lo halves, three fp16 MFMAs per product with fp32 accumulation (~2^-21 relative, 5.3x the MFMA rate;
 * activations must stay inside fp16 range |x| < 65504). */
enum { TTSC_PREC_FP32 = 0, TTSC_PREC_F16X3 = 1 };

typedef struct {
    float in_scale;      /* x is staged as leaky_relu(x * in_scale, in_slope); 1 / 1 = identity */
    float in_slope;
    float out_scale;     /* y = act((conv + bias + resid) * out_scale)  */
    int32_t out_act;     /* TTSC_ACT_* */
    int32_t accumulate;  /* 1: y += result (running sum of residual blocks) */
    /* data-gradient launches (training, row a9): gate_dev = the pre-activation [B,Cout,Lout] the forward layer read through its
     * leaky-relu prologue; then y = ((conv + bias) * (gate > 0 ? 1 : gate_slope) + resid) * out_scale.  NULL = off. */
    const float* gate_dev;
    float gate_slope;
} ttsc_conv1d_epilogue;

int ttsc_conv1d_create(const ttsc_conv1d_cfg* cfg, ttsc_conv1d** out);
/* weight: host fp32 in torch layout (already weight-norm folded); bias: host [Cout] or NULL */
int ttsc_conv1d_set_weight(ttsc_conv1d* c, const float* weight_host, const float* bias_host);
/* training: (re)pack the weights from DEVICE memory (torch parameter layout, fp32) on `stream`, no host round trip;
 * TTSC_PREC_FP32 handles only.  bias_dev NULL = no bias. */
int ttsc_conv1d_set_weight_device(ttsc_conv1d* c, const float* weight_dev, const float* bias_dev, void* stream);
/* same, reading the weight of the FORWARD layer this handle is the data gradient of: a Conv1d(Ci -> Co, K) forward weight
 * [Co,Ci,K] is packed as the flipped, transposed Conv1d(Co -> Ci, K) weight  W'[ci,co,k] = W[co,ci,K-1-k]. */
int ttsc_conv1d_set_weight_device_dgrad(ttsc_conv1d* c, const float* fwd_weight_dev, void* stream);
/* switch the arithmetic (TTSC_PREC_*); weights are re-packed from the host copy kept by set_weight */
int ttsc_conv1d_set_precision(ttsc_conv1d* c, int32_t precision);
int64_t ttsc_conv1d_out_len(const ttsc_conv1d* c, int64_t Lin);
int32_t ttsc_conv1d_in_channels(const ttsc_conv1d* c);
/* TTSC_PREC_F16X3 carries activations as fp16 (hi, lo) pairs: below |x| ~ 2^-3 the low half goes subnormal (accuracy decays
 * towards fp16's), above 65504 the high half overflows.  `scale` (a power of two) multiplies this layer's INPUT while it is
 * staged and is divided out of the accumulator in the epilogue — both exact; 1 = off.  Ignored by TTSC_PREC_FP32. */
int ttsc_conv1d_set_activation_scale(ttsc_conv1d* c, float scale);
float ttsc_conv1d_get_activation_scale(const ttsc_conv1d* c);
/* out_channels == 1 layers (conv_post): `flag_dev` (device, 4 bytes, or NULL = off) is OR-ed with 1 by the forward kernel when it emits a
 * non-finite sample — the range guard of the split-precision generator (ttsc_hifigan_forward). */
int ttsc_conv1d_set_nonfinite_flag(ttsc_conv1d* c, uint32_t* flag_dev);
/* out_dev[0] = max(out_dev[0], max_i |x_i|) over n device floats (out_dev zeroed by the caller); feeds the calibration below */
int ttsc_absmax(const float* x_dev, int64_t n, float* out_dev, void* stream);
/* x_dev [B,Cin,Lin] -> y_dev [B,Cout,Lout]; resid_dev NULL or [B,Cout,Lout]; ep NULL = plain conv */
int ttsc_conv1d_forward(const ttsc_conv1d* c, const float* x_dev, int32_t B, int64_t Lin, float* y_dev,
                        const float* resid_dev, const ttsc_conv1d_epilogue* ep, void* stream);
/* ragged batch: in_len_dev / out_len_dev int32 [B] (device) give each utterance's valid input / output length inside
 * the padded [B,C,L] tensors; input beyond in_len[b] reads as zero (== the utterance run alone), tiles wholly beyond
 * out_len[b] are skipped (their output is unspecified).  NULL = dense.
 * What the kernels do with the tail today (held by tests/test_conv_infer_f64_gpu.py and tests/test_conv1d_gpu.py): the column tile that
 * holds an utterance's last valid position is stored whole — its positions at or beyond out_len[b] receive the layer's result on the
 * zero-extended input, the bits of the dense call — and skipped tiles keep what the buffer held.  The tile is the launch's: 128 .. 512
 * columns in the general kernels, 256 in the wide kernel, 1024 in the Cout = 1 kernel.  The ResBlock chain kernels (ttsc_rbchain_forward)
 * store nothing at or beyond an utterance's length. */
int ttsc_conv1d_forward_ragged(const ttsc_conv1d* c, const float* x_dev, int32_t B, int64_t Lin, float* y_dev,
                               const float* resid_dev, const ttsc_conv1d_epilogue* ep, const int32_t* in_len_dev,
                               const int32_t* out_len_dev, void* stream);
/* The same with an explicit ROW PITCH of the output tensors: y_dev / resid_dev are [B,Cout,Lout_pitch] (Lout_pitch = 0: the natural
 * output length of Lin).  With per-utterance lengths in in_len_dev / out_len_dev, Lin and Lout_pitch are pitches only — that is how
 * ttsc_hifigan_forward keeps the rows of its intermediate tensors on 128-byte boundaries (4001 / 12004 samples per row otherwise: every
 * 128-byte store of the 256- and 128-channel stages straddled two lines).  Lout_pitch must cover every utterance's real output length. 
 * Rounding note (TTSC_PREC_F16X3, square 128- / 256-channel layers on the wide-tile kernel, out_scale == 1, no activation): by default the
 * residual, the running sum and the bias are the accumulators' INITIAL value (TTSC_CONV_ACC_INIT=1), so the K * Cin / 16 accumulation steps
 * round at the magnitude of the whole sum rather than of the convolution alone (self-check RMS against the fp32 oracle 6.4e-7 instead of 4.3e-7
 * for the whole generator; per-layer tolerance in tests 3e-6 relative).  TTSC_CONV_ACC_INIT=0 adds them after the sum (prefetched epilogue; the
 * bias still starts the sum there, so the bits differ from the general kernel's, which adds the bias last).  A layer's bits therefore depend on
 * which kernel the machine-fill rule selects; results are deterministic for a given (shape, batch, environment). */
int ttsc_conv1d_forward_pitched(const ttsc_conv1d* c, const float* x_dev, int32_t B, int64_t Lin, float* y_dev,
                                const float* resid_dev, const ttsc_conv1d_epilogue* ep, const int32_t* in_len_dev,
                                const int32_t* out_len_dev, int64_t Lout_pitch, void* stream);
/* Which kernel ttsc_conv1d_forward* launches for phase `phase` of the layer (0 unless the layer is a ConvTranspose1d that runs phase by phase) on a
 * batch of B utterances of Lin positions with epilogue `ep` (NULL = none), under the environment's TTSC_CONV_* switches; the launcher calls the
 * same selection.  No device is touched and no weights are needed: a handle from ttsc_conv1d_create + ttsc_conv1d_set_precision will do.
 * Returns a path id, < 0 (and ttsc_last_error) for what the launch would refuse, and fills info[10] = {tile rows, tile columns, tap bucket
 * (TTSC_CONV_PATH_F16X3: the TMAX of the instantiation, else 0), grid x, y, z, dynamic LDS bytes, lean, acc_init, short_from}:
 *   TTSC_CONV_PATH_NONE    nothing: the phase has no output position inside the output
 *   TTSC_CONV_PATH_COUT1   conv_cout1_kernel              one output channel (conv_post)
 *   TTSC_CONV_PATH_TALL    conv_f16x3_tall_kernel         the first two upsamplers of HiFi-GAN V1
 *   TTSC_CONV_PATH_WIDE    conv_f16x3_wide_kernel         square 128- / 256-channel ResBlock layers
 *   TTSC_CONV_PATH_F16X3   conv_f16x3_kernel              the general split-precision kernel
 *   TTSC_CONV_PATH_FP32    conv_mfma_kernel               the exact fp32 kernel */
#define TTSC_CONV_PATH_NONE 0
#define TTSC_CONV_PATH_COUT1 1
#define TTSC_CONV_PATH_TALL 2
#define TTSC_CONV_PATH_WIDE 3
#define TTSC_CONV_PATH_F16X3 4
#define TTSC_CONV_PATH_FP32 5
int32_t ttsc_conv1d_plan(const ttsc_conv1d* c, int32_t B, int64_t Lin, const ttsc_conv1d_epilogue* ep, int32_t phase, int32_t* info);
/* Fused residual pair y = x + conv2(lrelu(conv1(lrelu(x), 0.1), 0.1)) [+ y if accumulate]  of a HiFi-GAN ResBlock1
 * (both layers 32 -> 32 channels, odd kernel 3/7/11, conv2 undilated, both in TTSC_PREC_F16X3): the inner activation
 * stays in LDS, which removes two of the five HBM passes of the unfused pair.  `supported` returns 1 when the fused
 * kernel applies to the two layers; y must not alias x. */
int ttsc_respair_supported(const ttsc_conv1d* conv1, const ttsc_conv1d* conv2);
int ttsc_respair_forward(const ttsc_conv1d* conv1, const ttsc_conv1d* conv2, const float* x_dev, int32_t B, int64_t L,
                         float* y_dev, int32_t accumulate, const int32_t* len_dev, void* stream);
/* Fused ResBlock1 chain  x <- x + conv2_p(lrelu(conv1_p(lrelu(x), 0.1), 0.1)),  p = 0..npairs-1 (npairs <= 3), y (+)= x:
 * hifigan.models.ResBlock1.forward [EXTERNAL; call sites cube/networks/cubegan.py:72,83 via Generator.forward] for the 32- and
 * 64-channel stages, where every single convolution is HBM-bound.  The residual stream of a time tile stays in registers and
 * the activations in LDS for the whole chain; HBM sees one read of x and one write (read-modify-write when `accumulate`) of y.
 * All layers C -> C with C in {32, 64}, one odd kernel size K in {3, 7, 11}, conv1 dilation <= 5, conv2 undilated, "same"
 * padding, TTSC_PREC_F16X3, host-set weights with bias.  `supported` returns 1 when the fused kernel applies.
 * tile_shape: -1 = pick by halo, 0 = small tile (512 columns at C=32 / 256 at C=64; two workgroups per CU), 1 = large tile
 * (1024 / 512 columns, one 8-wave workgroup per CU); 0 and 1 run with interleaved columns (a lane's column tiles are consecutive
 * samples: the tile moves as dwordx4 / dwordx2 accesses; bit-identical results) when the dilations are in {1, 3, 5} unless the
 * environment says TTSC_CHAIN_IL=0; 10 / 11 ask for the interleaved kernels explicitly, 12 = 11 with 6-step weight groups (C = 32),
 * 2 .. 4 = measurement variants (longer weight groups, 768-column tiles).  y must not alias x. */
int ttsc_rbchain_supported(const ttsc_conv1d* const* convs1, const ttsc_conv1d* const* convs2, int32_t npairs);
int ttsc_rbchain_forward(const ttsc_conv1d* const* convs1, const ttsc_conv1d* const* convs2, int32_t npairs, const float* x_dev,
                         int32_t B, int64_t L, float* y_dev, int32_t accumulate, const int32_t* len_dev, int32_t tile_shape,
                         void* stream);
/* The last ResBlock1 chain of the generator with conv_post + activation in its epilogue:
 *     wav = act((conv_post(lrelu((ysum + chain(x)) * in_scale, in_slope)) + bias) * out_scale)         (scales / activation of post_ep)
 * — `xs += resblocks[-1](x); x = xs / nk; x = conv_post(lrelu(x)); tanh` of hifigan.models.Generator.forward [EXTERNAL; call sites
 * cube/networks/cubegan.py:72,83,131, cube/io_utils/runtime.py:78] in one launch: ysum_dev [B,32,L] (the sum of the blocks before this one, or NULL)
 * is only read, wav_dev [B,1,L] is the only tensor written, conv_post's range-guard word is honoured; bit-identical to
 * ttsc_rbchain_forward(accumulate) + ttsc_conv1d_forward.  32 channels, dilations in {1, 3, 5}, conv_post 32 -> 1 with k = 7 and padding 3;
 * L and every entry of len_dev multiples of 4, x / ysum 16-byte aligned.  ttsc_hifigan_forward uses it unless TTSC_HIFIGAN_FUSE_POST=0. */
int ttsc_rbchain_post_supported(const ttsc_conv1d* const* convs1, const ttsc_conv1d* const* convs2, int32_t npairs, const ttsc_conv1d* post);
int ttsc_rbchain_post_forward(const ttsc_conv1d* const* convs1, const ttsc_conv1d* const* convs2, int32_t npairs, const float* x_dev, int32_t B,
                              int64_t L, const float* ysum_dev, const ttsc_conv1d* post, const ttsc_conv1d_epilogue* post_ep, float* wav_dev,
                              const int32_t* len_dev, void* stream);
void ttsc_conv1d_destroy(ttsc_conv1d* c);

/* Weight gradient of the generator's convolutions (training: `Cubegan.training_step`, cube/networks/cubegan.py:85-189,
 * where torch autograd differentiates Generator.forward):
 *   G[a, b, j] += sum_n sum_t P[n,a,t] * leaky_relu(q_scale * Q[n,b,t + base + j*step], q_slope)       (zero outside [0,LQ))
 * Conv1d(weight [Co,Ci,K], dilation d, padding p): P = dL/dy [N,Co,Lout], Q = layer input [N,Ci,Lin], base = -p, step = d,
 * G = dL/dW [Co,Ci,K].  G (device, [A,B,J] fp32) is overwritten.  The position axis is split over ~2048 waves whose partial
 * tiles go through `ws_dev` (>= ttsc_conv_wgrad_workspace_bytes) and are added in a fixed order (deterministic).
 * |(J-1)*step| <= 64 per group of 12 taps. */
/* torch.nn.utils.weight_norm(dim=0) of the generator convolutions [EXTERNAL hifigan/models.py], fused: v [rows, cols] (cols =
 * product of the other dims), g [rows];  forward: w = v * g / ||v||_row, norm = ||v||_row;  backward: dv, dg from dw. */
int ttsc_weight_norm_forward(const float* v_dev, const float* g_dev, float* w_dev, float* norm_dev, int32_t rows, int64_t cols, void* stream);
int ttsc_weight_norm_backward(const float* dw_dev, const float* v_dev, const float* g_dev, const float* norm_dev, float* dv_dev,
                              float* dg_dev, int32_t rows, int64_t cols, void* stream);
/* torch.nn.utils.spectral_norm of the first scale discriminator ([EXTERNAL hifigan/models.py] MultiScaleDiscriminator:
 * DiscriminatorS(use_spectral_norm=True), used by cube/networks/cubegan.py:40-41): wn = W / sigma, sigma = u^T W v after one power iteration (v <- normalize(W^T u), u <- normalize(W v)).  The two
 * mat-vecs and the pieces around them, all with fixed summation orders:
 *   ttsc_matvec         W [rows, cols] row-major: out = W x (transpose 0) or W^T x (transpose 1; ws_dev >= ttsc_matvec_workspace_bytes)
 *   ttsc_l2_normalize   out[n] = x / max(||x||, eps), norm_dev[0] = ||x|| (either output may be NULL)
 *   ttsc_dot            out_dev[0] = sum a[i] b[i] (ws_dev >= ttsc_dot_workspace_bytes(n))
 *   ttsc_div_scalar     out = w / sigma_dev[0]
 *   ttsc_spectral_norm_backward   dW[r,c] = dWn[r,c] / sigma - (dot_dev[0] / sigma^2) u[r] v[c], dot_dev[0] = sum(dWn . W) */
size_t ttsc_matvec_workspace_bytes(int32_t rows, int64_t cols);
int ttsc_matvec(const float* w_dev, int32_t rows, int64_t cols, const float* x_dev, int32_t transpose, float* out_dev, void* ws_dev, size_t ws_bytes,
                void* stream);
int ttsc_l2_normalize(const float* x_dev, int32_t n, float eps, float* out_dev, float* norm_dev, void* stream);
size_t ttsc_dot_workspace_bytes(int64_t n);
int ttsc_dot(const float* a_dev, const float* b_dev, int64_t n, float* out_dev, void* ws_dev, size_t ws_bytes, void* stream);
int ttsc_div_scalar(const float* w_dev, const float* sigma_dev, float* out_dev, int64_t n, void* stream);
int ttsc_spectral_norm_backward(const float* dwn_dev, const float* u_dev, const float* v_dev, const float* sigma_dev, const float* dot_dev,
                                float* dw_dev, int32_t rows, int64_t cols, void* stream);
/* bias gradient db[c] = sum_{b,t} dy[b,c,t] (fixed summation order).  ws_is_fresh = 1 when the workspace was not left by a
 * previous ttsc_bias_grad call with the same shape (its ticket counters are then zeroed on the stream first). */
size_t ttsc_bias_grad_workspace_bytes(int32_t B, int32_t C, int64_t L);
int ttsc_bias_grad(const float* dy_dev, float* db_dev, int32_t B, int32_t C, int64_t L, void* ws_dev, size_t ws_bytes, int32_t ws_is_fresh,
                   void* stream);
/* torch.optim.AdamW (cube/networks/cubegan.py:275-298: betas (0.8, 0.99)) over ONE flat fp32 arena: parameters, gradients and both
 * moment estimates of a parameter group are four contiguous, 16-byte-aligned device arrays of n elements (the gradient arena is the
 * gradient-exchange bucket itself); `step` is the 1-based step count of the bias corrections.  Same update rule and operation order
 * as torch's single-tensor AdamW (decoupled weight decay, no amsgrad). */
int ttsc_adamw_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int64_t step, void* stream);
/* The same update behind a device-side guard: when *guard_dev != 0 at execution time the launch leaves parameters and moments untouched (null = no
 * guard).  The word is what ttsc_split_status_collect left on the stream: a training step can then queue its update without the host waiting for the
 * backward pass to learn whether a split recurrence gave up (cube/networks/cubegan.py:172-180 is the update; the reference has no such failure mode). */
int ttsc_adamw_step_guarded(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int64_t step, const uint32_t* guard_dev, void* stream);
/* GAN loss terms over a LIST of tensors in one launch, value and gradient together — hifigan.models.feature_loss / generator_loss /
 * discriminator_loss [EXTERNAL; call sites cube/networks/cubegan.py:144-149,160-167]:
 *   kind 0:  out = sum_k w_k * mean|a_k - b_k|      gb_k = w_k sign(b_k - a_k) / n_k,  ga_k = -gb_k      (feature matching: w = 2)
 *   kind 1:  out = sum_k w_k * mean (a_k - target)^2   ga_k = 2 w_k (a_k - target) / n_k              (least-squares GAN terms)
 * a_dev / b_dev / ga_dev / gb_dev: host arrays of nseg device pointers (gradient pointers, or the arrays themselves, may be null);
 * numel / weight: host arrays.  1 <= nseg <= 64 per call.  out_dev: one float.  Deterministic (fixed-order sums). */
/* nn.Embedding of the mel decoder's text stacks (cube/networks/modules.py:869-872) in training: out[i,:] = table[idx[i],:] (rows outside
 * [0,V) read as zero) and its gradient gtable[v,:] = sum_{i: idx[i]==v} gout[i,:] (every row written; row `skip_row` — padding_idx — gets
 * zeros; -1 = none).  Deterministic summation order. */
int ttsc_rows_gather(const float* table_dev, const int32_t* idx_dev, float* out_dev, int64_t n, int32_t C, int32_t V, void* stream);
int ttsc_rows_scatter_add(const float* gout_dev, const int32_t* idx_dev, float* gtable_dev, int64_t n, int32_t C, int32_t V, int32_t skip_row,
                          void* stream);
/* the same adjoint for a NON-DECREASING index list (phoneme rows -> frame rows, cube/networks/modules.py:1043-1053): O(n C) instead of O(V n C) */
int ttsc_rows_segment_sum(const float* gout_dev, const int32_t* idx_sorted_dev, float* gtable_dev, int64_t n, int32_t C, int32_t V, void* stream);
/* Phoneme rows of the word-conditioned text stacks (cube/networks/modules.py:930-940, 976-988, 1079-1082), one launch each way:
 *   out [B, N, Ch + Cs + Cw] = [ h[b, n, :] | spk[b, :] | cond[b, p2w[b, n], :] ]          h [B, N, Ch], spk [B, Cs], cond [B, Nw, Cw], p2w [B, N]
 *   gh = gout[:, :, :Ch],  gspk[b] = sum_n gout[b, n, Ch:Ch + Cs],  gcond[b, w] = sum_{n: p2w[b, n] == w} gout[b, n, Ch + Cs:]
 * The forward is a copy (bit-equal to cat / repeat / index); the sums run over n ascending inside one thread, without atomics (the same bits on
 * every run), a word no phoneme points at gets zeros, p2w need not be monotone.  p2w must lie in [0, Nw): the CALLER checks its host copy — the
 * kernels read an index outside that range as a zero row / skip it, they never touch memory through it. */
int ttsc_phone_rows_assemble(const float* h_dev, const float* spk_dev, const float* cond_dev, const int32_t* p2w_dev, float* out_dev, int32_t B, int32_t N,
                             int32_t Nw, int32_t Ch, int32_t Cs, int32_t Cw, void* stream);
int ttsc_phone_rows_assemble_bwd(const float* gout_dev, const int32_t* p2w_dev, float* gh_dev, float* gspk_dev, float* gcond_dev, int32_t B, int32_t N,
                                 int32_t Nw, int32_t Ch, int32_t Cs, int32_t Cw, void* stream);
/* Polyphase de-interleave of a strided Conv1d's operands (the discriminators' stride-2/3/4 layers [EXTERNAL hifigan/models.py DiscriminatorP /
 * DiscriminatorS; call sites cube/networks/cubegan.py:144-149,160-167]): the layer runs as a stride-1 convolution over
 *   xr[n, (g, r, ci), m P + w] = x[n, (g, ci), ((m s + r) - pad) P + w]   (zero outside; P = 1 or MPD's period, rows of P samples)
 * with taps  wp[co, (r, ci), j] = w[co, ci, s j + r]  (zero beyond K).  backward = 1 maps a gradient of xr / wp back onto x / w.
 * x [N, C, L P], xr [N, s C, M P]; w [Cout, Cg, K], wp [Cout, s Cg, ceil(K / s)]. */
int ttsc_deinterleave_x(const float* src_dev, float* dst_dev, int32_t N, int32_t C, int64_t L, int32_t groups, int32_t stride, int32_t period, int32_t pad,
                        int32_t M, int32_t backward, void* stream);
int ttsc_deinterleave_w(const float* src_dev, float* dst_dev, int32_t Cout, int32_t Cg, int32_t K, int32_t stride, int32_t backward, void* stream);
size_t ttsc_gan_loss_workspace_bytes(int32_t nseg);
int ttsc_gan_loss(int32_t kind, int32_t nseg, const void* const* a_dev, const void* const* b_dev, void* const* ga_dev, void* const* gb_dev,
                  const int64_t* numel, const float* weight, float target, float* out_dev, void* ws_dev, size_t ws_bytes, void* stream);
/* kind 0 over PRE-activations: slope[k] in [0, 1] (null = all 1) passes both operands of segment k through leaky_relu(., slope[k]) before the
 * difference and multiplies the gradients by the activation's derivative — the discriminators' feature maps are leaky_relu(conv output, 0.1)
 * ([EXTERNAL hifigan/models.py DiscriminatorP / DiscriminatorS forward]; feature_loss call sites cube/networks/cubegan.py:162-163): the training
 * step hands the convolution outputs over as they are instead of materialising ~90 activated copies and their backward launches per step. */
int ttsc_gan_loss_lrelu(int32_t kind, int32_t nseg, const void* const* a_dev, const void* const* b_dev, void* const* ga_dev, void* const* gb_dev,
                        const int64_t* numel, const float* weight, const float* slope, float target, float* out_dev, void* ws_dev, size_t ws_bytes,
                        void* stream);
size_t ttsc_conv_wgrad_workspace_bytes(int32_t N, int32_t A, int32_t B, int64_t LP, int32_t J);
/* grouped variant (torch Conv1d groups): P [N,A,LP], Q [N,groups*Bg,LQ], G [A,Bg,J] — row a only meets the Bg channels of its own
 * group.  Workspace: ttsc_conv_wgrad_workspace_bytes(N, A, Bg, LP, J). */
int ttsc_conv_wgrad_grouped(const float* p_dev, const float* q_dev, float* g_dev, int32_t N, int32_t A, int32_t Bg, int32_t groups, int64_t LP,
                            int64_t LQ, int32_t J, int32_t base, int32_t step, float q_scale, float q_slope, void* ws_dev, size_t ws_bytes,
                            void* stream);
int ttsc_conv_wgrad(const float* p_dev, const float* q_dev, float* g_dev, int32_t N, int32_t A, int32_t B, int64_t LP, int64_t LQ,
                    int32_t J, int32_t base, int32_t step, float q_scale, float q_slope, void* ws_dev, size_t ws_bytes, void* stream);

/* Split-precision weight gradient (csrc/conv_wgrad.hip::wgrad_f16x3_kernel): same contract as ttsc_conv_wgrad for the dense layers of the
 * training step (cubegan.py:137-170: every parameter gradient of MPD / MSD and of the generator), operands carried as fp16 hi + lo with
 * device-side ranges per launch, 128 x 64 tiles on v_mfma_f32_32x32x16_f16; agrees with ttsc_conv_wgrad to ~1e-6 of the largest entry.
 * `ttsc_conv_wgrad_split_supported` says whether a shape is taken (A >= 64 rows, Bc >= 32 columns, J <= 16 taps).  Range words as for
 * ttsc_conv_train: `measure` bit 0 = reduce max |Q| now, bit 1 = max |P| now, bit 2 = the caller's words were zeroed by the caller (pooled
 * words: no memset launch); null pointers = workspace words measured by this call. */
int32_t ttsc_conv_wgrad_split_supported(int32_t A, int32_t B, int32_t J, int32_t step);
size_t ttsc_conv_wgrad_split_workspace_bytes(int32_t N, int32_t A, int32_t B, int64_t LP, int32_t J);
int ttsc_conv_wgrad_split(const float* p_dev, const float* q_dev, float* g_dev, int32_t N, int32_t A, int32_t B, int64_t LP, int64_t LQ, int32_t J,
                          int32_t base, int32_t step, float q_scale, float q_slope, float* amax_q_dev, float* amax_p_dev, int32_t measure, void* ws_dev,
                          size_t ws_bytes, void* stream);
/* Grouped layers (MSD's k = 41 convolutions: groups of 16 .. 64 output channels) on the same split-precision scheme
 * (csrc/conv_wgrad.hip::wgrad_f16x3_grouped_kernel): p [N][A][LP], q [N][groups * Bg][LQ] -> g [A][Bg][J], group g = rows [g A / groups, (g + 1) A / groups)
 * against q's channels [g Bg, (g + 1) Bg).  Range words and `measure` as for ttsc_conv_wgrad_split. */
int32_t ttsc_conv_wgrad_split_grouped_supported(int32_t A, int32_t Bg, int32_t groups, int32_t J, int32_t step);
size_t ttsc_conv_wgrad_split_grouped_workspace_bytes(int32_t N, int32_t A, int32_t Bg, int32_t groups, int64_t LP, int32_t J);
int ttsc_conv_wgrad_split_grouped(const float* p_dev, const float* q_dev, float* g_dev, int32_t N, int32_t A, int32_t Bg, int32_t groups, int64_t LP, int64_t LQ,
                                  int32_t J, int32_t base, int32_t step, float q_scale, float q_slope, float* amax_q_dev, float* amax_p_dev, int32_t measure,
                                  void* ws_dev, size_t ws_bytes, void* stream);
/* The same call that also leaves the layer's bias gradient db[a] = sum_{n,t} p[n,a,t] in db_dev [A] (NULL = plain ttsc_conv_wgrad_split): its
 * slices are summed by surplus workgroups of the first weight-gradient launch and added in index order by surplus workgroups of the reduction —
 * the bits of ttsc_bias_grad, no launch of its own (same workspace size). */
int ttsc_conv_wgrad_split_bias(const float* p_dev, const float* q_dev, float* g_dev, float* db_dev, int32_t N, int32_t A, int32_t B, int64_t LP, int64_t LQ,
                               int32_t J, int32_t base, int32_t step, float q_scale, float q_slope, float* amax_q_dev, float* amax_p_dev, int32_t measure,
                               void* ws_dev, size_t ws_bytes, void* stream);
/* How ttsc_conv_wgrad_split(_bias) divides a shape, from the functions the launcher itself calls; no device is touched.  Returns TTSC_OK, < 0 (and
 * ttsc_last_error) for what the launch would refuse, and fills info[9] = {64-position chunks per batch item, work items N * chunks, 128 x 64 tiles,
 * CH = items per split, splits (grid x; the last split may own fewer than CH items, and a split's items may straddle batch items), taps per launch
 * min(5, 64 / |step| + 1), launches, taps of the last launch, bias-gradient slices per row}.  tests/test_conv_train_plan_cpu.py restates the rule,
 * and tests/test_conv_train_f64_gpu.py asks it before every weight-gradient case (a case names the CH and the tap groups it means to reach). */
int32_t ttsc_conv_wgrad_split_plan(int32_t N, int32_t A, int32_t B, int64_t LP, int32_t J, int32_t step, int32_t* info);

/* Split-precision convolution of the training step (csrc/conv_train.hip): forward and data gradient of a dense, stride-1, dilated Conv1d
 * of the generator [EXTERNAL hifigan/models.py; trained by cube/networks/cubegan.py:131-170] and of the MPD / MSD discriminators
 * (cubegan.py:144-149,160-167) on the fp16 hi/lo three-product MFMA path, stateless: weights come straight from the live torch parameter.
 *   y[b,co,t] = (( sum_ci sum_k W[co,ci,k] * lrelu(in_scale * x[b,ci,t - padding + k*dilation], in_slope) + bias[co] ) * g + resid[b,co,t]) * out_scale,
 *   g = 1 without `gate_dev`, else (gate[b,co,t] > 0 ? 1 : gate_slope)    (the leaky-relu derivative of a data-gradient launch),
 *   W = w_dev [Cout][Cin][K] (flip = 0), or W[co,ci,k] = w_dev[ci][co][K-1-k] with w_dev [Cin][Cout][K] (flip = 1: `w_dev` is the forward
 *   weight of the layer being differentiated).  x [B,Cin,Lin], y / resid / gate [B,Cout,Lout], Lout = Lin + 2 padding - dilation (K-1).
 *   groups > 1 (MSD's grouped k = 41 layers): torch Conv1d `groups`; w_dev [Cout][Cin/groups][K] (flip = 1: [Cin][Cout/groups][K]).
 * Both fp16 ranges are set per launch from device-side maxima of x and w (no host synchronisation, no calibration state); results agree
 * with the fp32 kernel to ~1e-6 relative.  The two range words (one float each, device) can be shared by the launches of one layer so that every
 * tensor is reduced once per step: forward measures max |x| and max |w| (`measure` = 3), the data gradient re-uses the weight word and measures
 * max |dy| (`measure` = 1), the weight gradient re-uses both; null pointers = measured into the workspace by this call; `measure` bit 2 = the words to be
 * measured were zeroed by the caller (words of a pool zeroed once per step: no memset launch).
 * `ttsc_conv_train_supported` says whether a shape is taken (receptive fields beyond 64 positions,
 * more than 41 taps and group sizes that do not tile into 32-row blocks stay on ttsc_conv1d_forward); the workspace holds the two range words and the packed weight fragments. */
int32_t ttsc_conv_train_supported(int32_t Cin, int32_t Cout, int32_t K, int32_t dilation, int32_t groups);
size_t ttsc_conv_train_workspace_bytes(int32_t Cin, int32_t Cout, int32_t K, int32_t groups);
int ttsc_conv_train(const float* x_dev, const float* w_dev, const float* bias_dev, const float* resid_dev, const float* gate_dev, float* y_dev,
                    int32_t B, int32_t Cin, int32_t Cout, int32_t K, int64_t Lin, int32_t padding, int32_t dilation, int32_t groups, int32_t flip, float in_scale,
                    float in_slope, float out_scale, float gate_slope, float* amax_x_dev, float* amax_w_dev, int32_t measure, void* ws_dev, size_t ws_bytes,
                    void* stream);
/* Which instantiation of conv_f16x3_kernel (folded) ttsc_conv_train / ttsc_conv_train_packed launch for a shape, from the function the launcher
 * itself calls (under the process's TTSC_TRAIN_NT, if set); no device is touched.  Returns TTSC_OK, < 0 (and ttsc_last_error) for what the launch
 * would refuse, and fills info[10] = {MI (row tile 32 MI), NJ (column tile 128 NJ: 2 when ceil(S B / 256) * (CoutP / MT) >= 512 and K <= 16), tap
 * bucket (3 / 7 / 11 / 16 / 21 / 41), S = max(Lin + padding, Lout) columns per utterance, S B, grid x, grid y, dynamic LDS bytes, CinP, CoutP}.
 * tests/test_conv_train_plan_cpu.py restates the rule, and tests/test_conv_train_f64_gpu.py asks it before every case (a case names its tile). */
int32_t ttsc_conv_train_plan(int32_t B, int32_t Cin, int32_t Cout, int32_t K, int64_t Lin, int32_t padding, int32_t dilation, int32_t groups,
                             int32_t* info);

/* The same convolution on weight fragments prepared by a weight bank (below): no weight reduction, no packing launch, no workspace.
 * wfrag_dev / amax_w_dev: the bank entry's `pack_fwd` (forward) or `pack_dgrad` (data gradient: pass the differentiated layer's Cout as Cin and
 * vice versa, as for flip = 1) and its `amax` word.  `measure` bit 0 = reduce max |x| into *amax_x_dev now (clear: the word already holds it — e.g.
 * the `amax_y_dev` word of the launch that produced x); bit 2 = the caller zeroed that word (words handed out from a pool zeroed once per step: no
 * memset launch).  amax_y_dev (or NULL): a ZEROED word that receives max |y| over the stored elements from the convolution's own epilogue, so that
 * the launches that read y next (the following layer, the preceding layer's data gradient, the weight gradient) need no reduction launch over it. */
int ttsc_conv_train_packed(const float* x_dev, const void* wfrag_dev, const float* bias_dev, const float* resid_dev, const float* gate_dev, float* y_dev,
                           int32_t B, int32_t Cin, int32_t Cout, int32_t K, int64_t Lin, int32_t padding, int32_t dilation, int32_t groups,
                           float in_scale, float in_slope, float out_scale, float gate_slope, float* amax_x_dev, const float* amax_w_dev,
                           int32_t measure, float* amax_y_dev, void* stream);

/* Weight bank: the per-step weight preparation of ALL convolutions of one module in three launches (csrc/conv_train.hip) — what the reference
 * leaves to torch.nn.utils.weight_norm's pre-forward hooks and to the cuDNN / MIOpen filter transforms inside every nn.Conv1d / nn.Conv2d call of
 * Generator / MultiPeriodDiscriminator / MultiScaleDiscriminator [EXTERNAL hifigan/models.py; cubegan.py:131,144-149,160-167].
 * Per entry (all pointers device memory owned by the caller, valid until ttsc_wbank_destroy):
 *   v [Cout][Cin/groups][K] fp32 and g [Cout] (weight_v / weight_g; g NULL: v is the plain weight);
 *   w (same shape as v) and norm [Cout]: receive g * v / ||v|| and the row norms (ttsc_weight_norm_forward's outputs; unused when g is NULL);
 *   amax: one float, receives max |w|;  pack_fwd / pack_dgrad: ttsc_conv_train_workspace_bytes(stride * Cin, Cout, ceil(K / stride), groups) - 256
 *   bytes (resp. with the two channel counts swapped), either may be NULL;
 *   stride > 1: the layer is a strided convolution evaluated as a stride-1 convolution over the phase-de-interleaved input
 *   (ttsc_deinterleave_x); the fragments hold w'[co][(r, ci)][j] = w[co][ci][stride * j + r] (zero beyond K) = ttsc_deinterleave_w's output.
 * ttsc_wbank_prepare re-reads v / g and refills every output (call it after the parameters changed, on the stream the convolutions follow on). */
typedef struct ttsc_wbank ttsc_wbank;
typedef struct ttsc_wbank_entry {
    const float* v;
    const float* g;
    float* w;
    float* norm;
    float* amax;
    void* pack_fwd;
    void* pack_dgrad;
    int32_t Cin, Cout, K, groups, stride;
} ttsc_wbank_entry;
int ttsc_wbank_create(const ttsc_wbank_entry* entries_host, int32_t n, ttsc_wbank** out);
int ttsc_wbank_prepare(ttsc_wbank* bank, void* stream);
void ttsc_wbank_destroy(ttsc_wbank* bank);

/* ------------------------------------------------------------------------------------------------
 * HiFi-GAN generator.  Replaces `hifigan.models.Generator(h)` [EXTERNAL submodule]:
 * constructed cube/networks/cubegan.py:41-43 and cube/io_utils/runtime.py:49-51,
 * called cubegan.py:72,83,131,234 and runtime.py:78 as generator(mel[B,80,T]) -> [B,1,L].
 * ------------------------------------------------------------------------------------------------ */
typedef struct ttsc_hifigan ttsc_hifigan;

#define TTSC_HIFIGAN_MAX_UPS 8
#define TTSC_HIFIGAN_MAX_RB 8
#define TTSC_HIFIGAN_MAX_DIL 8

typedef struct {
    int32_t num_mels;                 /* 80 */
    int32_t upsample_initial_channel; /* 512 */
    int32_t resblock;                 /* 1 or 2 (config key "resblock") */
    int32_t num_upsamples;
    int32_t upsample_rates[TTSC_HIFIGAN_MAX_UPS];
    int32_t upsample_kernel_sizes[TTSC_HIFIGAN_MAX_UPS];
    int32_t num_kernels;
    int32_t resblock_kernel_sizes[TTSC_HIFIGAN_MAX_RB];
    int32_t num_dilations[TTSC_HIFIGAN_MAX_RB];
    int32_t resblock_dilation_sizes[TTSC_HIFIGAN_MAX_RB][TTSC_HIFIGAN_MAX_DIL];
} ttsc_hifigan_cfg;

int ttsc_hifigan_create(const ttsc_hifigan_cfg* cfg, ttsc_hifigan** out);
/* name = folded state_dict key: "conv_pre.weight", "ups.0.bias", "resblocks.3.convs1.2.weight",
 * "conv_post.weight" ...; host fp32, torch layout, shape checked.  The host copy is kept and
 * packed/uploaded lazily by the next forward, so weights may be updated any number of times. */
int ttsc_hifigan_set_weight(ttsc_hifigan* g, const char* name, const float* host, const int64_t* shape, int32_t nd);
/* TTSC_PREC_* for every conv of the generator (default: TTSC_PREC_F16X3, overridable with env TTSC_HIFIGAN_PRECISION=fp32) */
int ttsc_hifigan_set_precision(ttsc_hifigan* g, int32_t precision);
int64_t ttsc_hifigan_out_len(const ttsc_hifigan* g, int64_t T);
size_t ttsc_hifigan_workspace_bytes(const ttsc_hifigan* g, int32_t B, int64_t T);
/* mel_dev [B,num_mels,T] -> wav_dev [B,1,out_len(T)] (tanh output in (-1,1)) */
int ttsc_hifigan_forward(ttsc_hifigan* g, const float* mel_dev, int32_t B, int64_t T, float* wav_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);
/* ragged batch: frames_host int32 [B] (HOST pointer, copied) = valid mel frames per utterance (<= T).  Every layer masks
 * its input beyond the utterance's own length, so wav_dev[b, 0, :out_len(frames[b])] equals that utterance run alone
 * and padding-only tiles are skipped.  The workspace must hold ttsc_hifigan_workspace_bytes(g,B,T) bytes. */
int ttsc_hifigan_forward_ragged(ttsc_hifigan* g, const float* mel_dev, int32_t B, int64_t T, const int32_t* frames_host,
                                float* wav_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* algorithmic FLOPs (2 x MAC) of one forward at (B, T): the roofline numerator used by bench.py */
/* Activation pre-scales of the split-precision path: one layer-by-layer forward on `mel` with an abs-max reduction in front of
 * every convolution; every layer's input scale becomes the power of two that puts that maximum in [2^9, 2^10) (six binades of
 * head-room below fp16's 65504, full 22-bit accuracy for values down to 2^-13 of the maximum).  The first ttsc_hifigan_forward
 * after the weights or the precision changed calibrates by itself — by default on a FIXED built-in probe mel (log-mel range
 * [-5, 1]), so the scales depend on the weights alone and a handle's output never depends on which utterance came first
 * (env TTSC_HIFIGAN_CALIBRATE=input: on that call's own input; =0: all scales stay 1).  Call this function to calibrate on other
 * data.  wav_dev / workspace as for the forward (wav_dev receives that forward's output).
 * Range guard: every split-precision forward checks (one stream synchronisation) whether conv_post emitted a non-finite sample —
 * an fp16 overflow in any layer reaches the waveform as NaN; it then re-calibrates on that input, reruns, and returns TTSC_ERANGE
 * only if the output is still non-finite.  ttsc_hifigan_recalibrations counts the reruns (env TTSC_HIFIGAN_RANGE_CHECK=0: off). */
int ttsc_hifigan_calibrate(ttsc_hifigan* g, const float* mel_dev, int32_t B, int64_t T, float* wav_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);
int ttsc_hifigan_get_activation_scale(const ttsc_hifigan* g, const char* layer_name, float* scale_out);
/* Restores persisted scales (the file a checkpoint keeps beside it): ALL n layers of the generator by name, powers of two.  Pending
 * weights are uploaded first; the handle then counts as calibrated until its weights change. */
int ttsc_hifigan_set_activation_scales(ttsc_hifigan* g, const char* const* layer_names, const float* scales, int32_t n);
int32_t ttsc_hifigan_recalibrations(const ttsc_hifigan* g);
/* The two side streams of the branch schedule (the ResBlocks of a layer-by-layer stage beside each other for ragged / small batches, TTSC_HIFIGAN_BRANCH_STREAMS):
 * by default the handle creates its own on first use; a host that keeps a stream pool hands two of ITS streams in (borrowed: never destroyed here; the caller
 * keeps them alive while the handle can run).  Why it matters: the runtime multiplexes all streams of a process onto four hardware queues, and two more
 * streams shift the queue every stream created after them lands on — a training step that followed a small-batch forward in the same process ran 61.5 -> 69 ms
 * (profiles/r06_branch_stream_queues.log).  Outputs are identical bit for bit whichever streams are used.  (nullptr, nullptr): back to the handle's own. */
int ttsc_hifigan_set_branch_streams(ttsc_hifigan* g, void* stream_a, void* stream_b);
/* Range guard mode: 1 (default) = every forward synchronises its stream, re-calibrates + reruns when tripped; 2 = deferred: forwards
 * never wait, the guard word stays sticky on the device until ttsc_hifigan_range_status() (which synchronises `stream`) reads and
 * clears it: 1 = some forward since the last call emitted a non-finite sample — its output must be discarded / recomputed —, 0 = all
 * clean; 0 = guard off. */
int ttsc_hifigan_set_range_check(ttsc_hifigan* g, int32_t mode);
int32_t ttsc_hifigan_range_status(ttsc_hifigan* g, void* stream);
int ttsc_hifigan_algorithmic_flops(const ttsc_hifigan* g, int32_t B, int64_t T, double* flops_out);
void ttsc_hifigan_destroy(ttsc_hifigan* g);

/* ------------------------------------------------------------------------------------------------
 * WaveRNN autoregressive vocoder network.  Replaces `cube.networks.modules.WaveRNN._inference`
 * (cube/networks/modules.py:453-503; constructed vocoder.py:45-57) — the per-sample python loop of
 * nn.GRU(seq=1) -> tanh(Linear) -> Linear -> output_functions.sample — with one persistent kernel.  Every output distribution
 * of cube/networks/loss.py is sampled in the kernel: MULAWOutput / RAWOutput (Categorical.sample as Gumbel-max, loss.py:218-307),
 * MOLOutput (the reference default; Gumbel-max over 10 mixtures + logistic inverse CDF, loss.py:163-201), GaussianOutput
 * (loss.py:50-52) and BetaOutput (two Marsaglia-Tsang gamma variates, loss.py:83-92).
 * Weight names are the reference state_dict keys: "_rnns.<l>.weight_ih_l0", "_rnns.<l>.weight_hh_l0",
 * "_rnns.<l>.bias_ih_l0", "_rnns.<l>.bias_hh_l0", "_lowres_conv.<i>.conv.weight|bias",
 * "_preoutput.linear_layer.weight|bias", "_output.linear_layer.weight|bias"; "_skip.*" is accepted and ignored
 * (dead layer, modules.py:424).  Arithmetic contract: include/ttscube_math.h + oracle/wavernn_ref.c.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ttsc_wavernn ttsc_wavernn;

enum { TTSC_WR_OUT_MULAW = 0, TTSC_WR_OUT_RAW = 1, TTSC_WR_OUT_MOL = 2, TTSC_WR_OUT_GM = 3, TTSC_WR_OUT_BETA = 4 };
/* sampler noise: none (arg-max / distribution mode) | injected [B,L,W] | in-kernel Philox-4x32-10 counters.
 * W (floats per step) = 256 for mulaw/raw (Gumbel terms), 11 for MOL (10 Gumbel terms -log(-log u) + 1 logistic term
 * log u - log(1-u)), 1 for Gaussian (0.8 * N(0,1)), 18 for Beta (per gamma variate: boost uniform + 4 (normal, uniform) rounds);
 * defined next to the samplers in include/ttscube_math.h. */
enum { TTSC_WR_MODE_ARGMAX = 0, TTSC_WR_MODE_NOISE = 1, TTSC_WR_MODE_PHILOX = 2 };

typedef struct {
    int32_t H;            /* layer_size (GRU hidden), multiple of 8, <= 512 */
    int32_t num_layers;   /* stacked GRUs (1..4) */
    int32_t use_lowres;   /* 1: high-res net conditioned on x_low (in_dim 102); 0: low-res net (in_dim 81) */
    int32_t upsample;     /* mel repeat factor: 240 (hr) / 24 (lr) */
    int32_t upsample_low; /* 10 */
    int32_t S;            /* output_functions.sample_size: 256 mulaw/raw, 30 mol, 2 gm/beta */
    int32_t n_mel;        /* 80 */
    int32_t out_kind;     /* TTSC_WR_OUT_* */
} ttsc_wavernn_cfg;

int ttsc_wavernn_create(const ttsc_wavernn_cfg* cfg, ttsc_wavernn** out);
int ttsc_wavernn_set_weight(ttsc_wavernn* w, const char* name, const float* host, const int64_t* shape, int32_t nd);
/* samples emitted for T mel frames / Tl low-res samples: min(T*upsample, Tl*upsample_low) (modules.py:467) */
int64_t ttsc_wavernn_out_len(const ttsc_wavernn* w, int64_t T, int64_t Tl);
size_t ttsc_wavernn_workspace_bytes(const ttsc_wavernn* w, int32_t B, int64_t T, int64_t Tl);
/* mel_dev [B,T,n_mel]; xlow_dev [B,Tl] (hr net) or NULL; noise_dev [B,L,W] (mode NOISE) or NULL;
 * forced_x_dev [B,L] or NULL (teacher forcing: feedback = forced_x[t], logits then equal _train_forward);
 * outputs idx_dev uint8 [B,L] (class index; mixture index for MOL; 0 for gm/beta), wav_dev fp32 [B,L] (what _inference returns), logits_dev
 * fp32 [B,L,S] or NULL. */
int ttsc_wavernn_decode(ttsc_wavernn* w, const float* mel_dev, const float* xlow_dev, int32_t B, int64_t T, int64_t Tl,
                        int32_t mode, const float* noise_dev, uint64_t seed, const float* forced_x_dev,
                        uint8_t* idx_dev, float* wav_dev, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream);
/* Ragged decode: per-row lengths in both decode kernels.  Arguments of ttsc_wavernn_decode plus four HOST tables, which are
 * copied (one stream synchronisation, as in ttsc_hifigan_forward_ragged):
 *   frames_host  int32 [B]   valid mel frames of row b, 1..T
 *   low_len_host int32 [B]   valid x_low samples of row b, 1..Tl (hr net); NULL for the low-resolution net
 *   seed_host    uint64 [B]  Philox key of row b, or NULL: every row uses `seed`
 *   stream_host  uint32 [B]  what stands in Philox counter word 2 in place of the row's batch position, or NULL: the row index
 * Row b emits L_b = min(frames[b]*upsample, low_len[b]*upsample_low) samples (frames[b]*upsample for the low-resolution net).  T,
 * Tl and L = out_len(T, Tl) stay the row strides of every [B, ...] buffer (noise, forced_x and logits included).  For t < L_b, idx /
 * wav / logits of row b are bit for bit what ttsc_wavernn_decode gives for that row's valid prefix alone, called with
 * T = frames[b], Tl = low_len[b], seed = seed[b] and the row at batch position stream[b]: the k = 7 convolutions' zero padding and
 * the interpolation's end clamp sit at the row's own low_len.  Nothing is stored at t >= L_b, and no input element beyond a row's
 * own lengths influences any output (the padding may hold anything, NaN included).  A length of 0 or above T / Tl, or a missing
 * low_len_host for the hr net, is TTSC_EINVAL before any launch.  Kernel choice and ttsc_wavernn_last_status are those of
 * ttsc_wavernn_decode; a tile of the tile kernel runs as many steps as the longest of ITS eight rows, a workgroup of the
 * streaming kernel as many as the longest of its rows. */
int ttsc_wavernn_decode_ragged(ttsc_wavernn* w, const float* mel_dev, const float* xlow_dev, int32_t B, int64_t T, int64_t Tl,
                               const int32_t* frames_host, const int32_t* low_len_host, const uint64_t* seed_host,
                               const uint32_t* stream_host, int32_t mode, const float* noise_dev, uint64_t seed,
                               const float* forced_x_dev, uint8_t* idx_dev, float* wav_dev, float* logits_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream);
/* Which kernel ran the last decode and whether its hand-offs completed.  Synchronises `stream`, then: -1 = single-workgroup
 * streaming kernel; 2 = tile kernel (8 workgroups step 8 utterances, each owning an eighth of the weight rows; chosen for
 * one-layer networks (any output head) when ceil(B/8)*8 <= number of CUs, H <= 512; env TTSC_WR_TILE=0 turns it off);
 * 1 = the tile kernel gave up on an inter-workgroup hand-off (bounded spin timed out; outputs invalid). */
int ttsc_wavernn_last_status(ttsc_wavernn* w, void* stream);
void ttsc_wavernn_destroy(ttsc_wavernn* w);

/* ------------------------------------------------------------------------------------------------
 * Linear (fp32 MFMA NT GEMM): y[M, :N] = act(x[M, :K] . w[N,K]^T + bias) [+ y if accumulate].
 * Replaces torch.nn.Linear inside LinearNorm (cube/networks/modules.py:24-34) for _dur_output, _pitch_output,
 * _cond_output, _mel_output, PreNet, and carries the hoisted LSTM input projections.  All pointers are device
 * pointers (the weight is whatever torch holds: [out, in] row-major).  ldx is a row stride only: 0 < ldx < K reads
 * overlapping rows (STFT framing, io_utils/melspec.py); ldy >= N.
 * ------------------------------------------------------------------------------------------------ */
int ttsc_linear_forward(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int64_t M, int32_t N,
                        int32_t K, int64_t ldx, int64_t ldy, int32_t act, int32_t accumulate, void* stream);
/* The same contract on the f16 matrix pipe with fp32-class accuracy (gemm.hip: gemm_nt_f16x3_kernel): operands split into fp16 hi / lo halves on
 * their way into LDS, three MFMA products per tile (lo.hi + hi.lo + hi.hi, fp32 accumulation).  The low half is stored scaled by 2^11 and its two
 * products are accumulated apart (added as acc_hi + 2^-11 acc_lo), so the accuracy does not depend on the operands' scale: ~2^-22 relative per
 * product, per element within 2^-20 of sum |x||w| for operand magnitudes 2^-14 .. 65504 (below 2^-14 a value keeps an absolute 2^-36).  Operands must lie
 * inside the fp16 range (|v| <= 65504): anything beyond sets a sticky per-device status word, read (and cleared; synchronises) by
 * ttsc_gemm_split_status — 1 = a result since the last call is invalid.  lengths_dev [M / period] or NULL: rows are [utterance][period]; 128-row
 * tiles that lie wholly at or beyond their utterances' lengths are skipped and stay unwritten (the recurrences never read them).
 * ttsc_linear_split_supported: K >= 32, K % 4 == 0, ldx % 4 == 0, ldx >= K (and 16-byte aligned x / w); otherwise TTSC_EINVAL — use
 * ttsc_linear_forward.  Callers: the hoisted input projections of the text-side BiLSTMs at inference (cube/networks/modules.py:873-905). */
int32_t ttsc_linear_split_supported(int64_t M, int32_t N, int32_t K, int64_t ldx);
int ttsc_linear_forward_split(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int64_t M, int32_t N, int32_t K,
                              int64_t ldx, int64_t ldy, int32_t act, int32_t accumulate, const int32_t* lengths_dev, int32_t period, void* stream);
int32_t ttsc_gemm_split_status(void);

/* General fp32-MFMA GEMM for the backward passes of the Linears and of the hoisted recurrent projections (training, row a9; the
 * reference leaves these to autograd over torch.nn.Linear / nn.GRU / nn.LSTM: cube/networks/modules.py:505-563, cubegan.py:85-189):
 *     C[M, :N] (+)= opA(A) . opB(B)     transA = 0: A is [M,K] (lda), 1: A is [K,M];   transB = 0: B is [K,N] (ldb), 1: B is [N,K]
 *   dx = dG . W (NN), dW = dG^T . x (TN), dW_hh = dG^T . h_prev (TN with b_row_shift = -1 / +1 and b_period = T: row r of the
 *   contraction reads B row r + shift when 0 <= r % period + shift < period and zero otherwise, so h_prev is never materialised).
 *   A non-zero shift needs |shift| < b_period and K % b_period == 0 (whole sequences: with a partial last period a forward shift would
 *   read B row K); anything else is TTSC_EINVAL before any launch.
 * When M x N tiles alone cannot fill the device the contraction is split over K; partial tiles go through ws_dev
 * (>= ttsc_gemm_workspace_bytes(M, N, K); may be NULL when that is 0) and are added in a fixed order (deterministic).
 * ttsc_colsum: out[c] (+)= sum_r x[r, c] (bias gradients), two fixed-order stages through ws_dev (>= ttsc_colsum_workspace_bytes). */
size_t ttsc_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int ttsc_gemm(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, const float* a_dev, int64_t lda, const float* b_dev, int64_t ldb,
              float* c_dev, int64_t ldc, int32_t accumulate, int64_t b_row_shift, int64_t b_period, void* ws_dev, size_t ws_bytes, void* stream);
size_t ttsc_colsum_workspace_bytes(int64_t R, int64_t C);
int ttsc_colsum(const float* x_dev, int64_t R, int64_t C, int64_t ld, float* out_dev, int32_t accumulate, void* ws_dev, size_t ws_bytes,
                void* stream);

/* Measurement helper (bench.py `roofline`): executed dense f16 MFMA TFLOP/s that a register-only v_mfma_f32_32x32x16_f16 loop sustains on every
 * CU of the current device for ~ms_target milliseconds, by operand data — mode 0: all-zero operands, 1: random fp16 operands, 2: the
 * split-precision mix (hi x hi, hi x lo, lo x hi with lo at 2^-11 scale).  The chip clocks to its power budget: real data sustains ~2/3 of the
 * nominal peak (csrc/probe.hip).  Synchronises `stream`.  No counterpart in the reference (it has no kernels). */
int ttsc_probe_mfma_tflops(int32_t mode, double ms_target, double* tflops_out, void* stream);

/* Test-only probes of include/ttscube_math.h (csrc/probe.hip, compiled with the library's ordinary flags): the device evaluates the shared
 * definitions element by element so that tests/test_shared_math_gpu.py can hold them equal, bit for bit, to the host build of the same header
 * (oracle/wavernn_ref.c: wr_math_array, wr_philox_array, wr_noise_array, wr_sample_array — same fn / kind numbering).  All asynchronous on
 * `stream`.  No counterpart in the reference. */
enum {
    TTSC_PROBE_EXPF = 0, TTSC_PROBE_LOGF = 1, TTSC_PROBE_SIGMOIDF = 2, TTSC_PROBE_TANHF = 3, TTSC_PROBE_NORMAL_ICDF = 4, TTSC_PROBE_LOGISTIC = 5,
    TTSC_PROBE_U01 = 6, TTSC_PROBE_U01_CLIP = 7, TTSC_PROBE_GUMBEL = 8   /* 6 - 8 read the input as uint32 */
};
/* out_dev[i] = fn(in_dev[i]), one thread per element; in_dev: n floats (fn <= 5) or n uint32 (fn >= 6) */
int ttsc_probe_math(int32_t fn, const void* in_dev, float* out_dev, int64_t n, void* stream);
/* out_dev[i, 0:4] = ttsc_philox4x32(counter ctr_dev[i, 0:4], key key_dev[i, 0:2]) */
int ttsc_probe_philox(const uint32_t* ctr_dev, const uint32_t* key_dev, uint32_t* out_dev, int64_t n, void* stream);
/* out_dev[i, 0:W] = ttsc_noise_mol / _gm / _beta (t_dev[i], b_dev[i], seed_dev[i]); kind = TTSC_WR_OUT_MOL / GM / BETA, W = 11 / 1 / 18 */
int ttsc_probe_noise(int32_t kind, const uint32_t* t_dev, const uint32_t* b_dev, const uint64_t* seed_dev, float* out_dev, int64_t n, void* stream);
/* One continuous sample per row of y_dev [n, S] (S = 30 MOL, 2 GM / BETA): wv_dev[i] the sample, k_dev[i] the mixture index (0 unless MOL).
 * mode = TTSC_WR_MODE_*: ARGMAX zero noise, NOISE noise_dev [n, W], PHILOX counters (t_dev[i], b_dev[i]) under key seed_dev[i] (unused
 * pointers may be NULL).  impl 0: ttsc_sample_mol / _gm / _beta of the header, one thread per row; impl 1: the decode kernels' wave-parallel
 * wr_sample_continuous (csrc/wavernn_sampler.hpp), one wave per row. */
int ttsc_probe_sample(int32_t out_kind, int32_t mode, int32_t impl, const float* y_dev, const float* noise_dev, const uint32_t* t_dev,
                      const uint32_t* b_dev, const uint64_t* seed_dev, float* wv_dev, int32_t* k_dev, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LSTM / BiLSTM recurrence.  Replaces the sequential part of torch.nn.LSTM (gate order i,f,g,o, `_reverse`
 * direction) for Languasito2 (modules.py:873-905) and CubenetTextcoder (textcoder.py:55-92).
 *   xg_dev        [B, T, ndir*4H]  pre-activations  x.W_ih^T + b_ih + b_hh  (from ttsc_linear_forward)
 *   whh_packed    from ttsc_lstm_pack_whh(weight_hh_l{k}[, weight_hh_l{k}_reverse] stacked [ndir,4H,H] on the host)
 *   y_dev         [B, T, ldy]; direction d writes columns [yoff + d*H, yoff + (d+1)*H)
 *   lengths_dev   int32 [B] or NULL: pack_padded_sequence semantics (outputs beyond the length are zero)
 *   h0/c0/hn/cn   optional [ndir, B, H] initial / final states (NULL = zeros / not returned)
 * ------------------------------------------------------------------------------------------------ */
int ttsc_lstm_pack_whh(const float* whh_host, int32_t ndir, int32_t H, float** whh_dev_out);
int ttsc_lstm_seq_forward(const float* xg_dev, const float* whh_packed_dev, float* y_dev, const int32_t* lengths_dev,
                          int32_t B, int32_t T, int32_t H, int32_t ndir, int64_t ldy, int32_t yoff, const float* h0_dev,
                          const float* c0_dev, float* hn_dev, float* cn_dev, void* stream);
/* Training of the mel-decoder stacks (Languasito2 / CubenetTextcoder LSTMs inside `Cubegan.training_step`, cubegan.py:85-189;
 * the reference differentiates torch.nn.LSTM):
 *   ttsc_lstm_pack_whh_device   weight_hh [ndir,4H,H] on the DEVICE -> out_dev [ndir*4H*H]: the forward packing (transpose = 0) or
 *                               the W_hh^T packing the backward kernel streams (transpose = 1); no host round trip
 *   ttsc_lstm_seq_forward_train same recurrence, additionally saves the post-activation gates [B,T,ndir*4H] (i,f,g,o) and the
 *                               cell states [B,T,ndir*H]
 *   ttsc_lstm_seq_backward      backward through time: dy [B,T,ldy] (columns yoff + d*H ...) -> gradient wrt the pre-activation
 *                               gates dgates [B,T,ndir*4H] (zero beyond lengths).  The caller finishes with plain GEMMs:
 *                               dx = dgates W_ih, dW_ih = dgates^T x, dW_hh = dgates^T h_prev, db = sum dgates. */
/* With few sequences (G * B * ndir <= number of CUs; G <= 4, env TTSC_LSTM_SPLIT caps it, 1 = off) the forward, train-forward and
 * backward recurrences split every (utterance, direction) over G workgroups (TTSC_LSTM_SPLIT_INFER=0 exempts inference) that exchange the state once per step (see
 * ttsc_gru_split_status); results then differ from the single-workgroup kernels in summation order only (<= 1e-6 relative).
 * ttsc_lstm_split_status: 0 = every hand-off since the last call completed, 1 = a bounded spin timed out (sticky until read:
 * later split launches give up at once, so callers that care check it once per step / synthesis).  Synchronises the device. */
int32_t ttsc_lstm_split_status(void);
/* The same verdict for the split recurrences (LSTM, GRU, mel-AR) launched on ONE stream, waiting for that stream only: bit 0 LSTM, bit 1 GRU,
 * bit 2 mel-AR; reported once, then re-armed; < 0 on a HIP error.  For a training step that runs its text side on a stream of its own and must know
 * that this stream's backward pass is sound BEFORE its gradients are exchanged and applied (cube/networks/cubegan.py:172-180 is the update it guards),
 * without draining the other streams. */
int32_t ttsc_split_status_stream(void* stream);
/* Device-side form of the same question: ONE launch on `stream` ORs the verdict bits of every split recurrence launched on that stream so far (bit 0 LSTM,
 * bit 1 GRU, bit 2 mel-AR, bit 3 other; bit 4 = the split-precision GEMM's range word) into *dst_dev and re-arms the sticky words; the host waits for
 * nothing.  flags: bit 0 = include the GEMM's range word, bit 1 = the recurrences of EVERY stream of the device (the caller has made `stream` wait for
 * them).  Returns the number of status words looked at (0: nothing to ask, no launch), < 0 on a HIP error. */
int32_t ttsc_split_status_collect(void* stream, uint32_t* dst_dev, int32_t flags);
/* Utterances per member group of the register-resident split recurrence (H = 256 / 512: 4 / 16 workgroups per group hold W_hh in registers).
 * 0 (default) = automatic: the smallest of 1 / 2 / 4 that takes the padded batch in one launch — the shortest step.  n = 1 / 2 / 4 / 8: n per
 * group whenever the batch has that many — n times fewer CUs held for a somewhat longer step, for callers that run the recurrence beside a
 * kernel that fills the chip (Cubegan.inference_pipelined).  Results do not depend on it (per utterance the arithmetic is the same).
 * Process-wide; returns the previous value, -1 for a bad n.  Not in the reference (B = 1 there, cube/networks/modules.py:946-953). */
int32_t ttsc_lstm_set_group_size(int32_t n);
int ttsc_lstm_pack_whh_device(const float* whh_dev, int32_t ndir, int32_t H, int32_t transpose, float* out_dev, void* stream);
int ttsc_lstm_seq_forward_train(const float* xg_dev, const float* whh_packed_dev, float* y_dev, const int32_t* lengths_dev,
                                int32_t B, int32_t T, int32_t H, int32_t ndir, int64_t ldy, int32_t yoff, float* gates_dev,
                                float* c_dev, void* stream);
int ttsc_lstm_seq_backward(const float* dy_dev, const float* gates_dev, const float* c_dev, const float* whhT_packed_dev,
                           float* dgates_dev, const int32_t* lengths_dev, int32_t B, int32_t T, int32_t H, int32_t ndir,
                           int64_t ldy, int32_t yoff, void* stream);
/* Which kernels ttsc_lstm_seq_forward_train (backward = 0) or ttsc_lstm_seq_backward (backward = 1) launch for a batch of B utterances, ndir
 * directions and hidden size H on the CURRENT device (lengths = NULL); the launchers call the same selection.  Returns a path id, < 0 for a bad shape,
 * and fills info[3] = {G members per (utterance, direction), NB utterances per member group (SPLIT_RES_NB) or per workgroup (SEQ), launches}:
 *   TTSC_LSTM_PATH_SEQ           lstm_seq_kernel<NB> / lstm_bwd_kernel            one workgroup per (utterance tile, direction), rows streamed
 *   TTSC_LSTM_PATH_SPLIT         lstm_seq_split_kernel / lstm_bwd_split_kernel    G workgroups per sequence, counter hand-off
 *   TTSC_LSTM_PATH_SPLIT_RES     lstm_seq_split_res_kernel / lstm_bwd_split_res_kernel   W_hh in registers over G members, granule hand-off
 *   TTSC_LSTM_PATH_SPLIT_RES_NB  lstm_seq_split_res_nb_kernel<NB> (forward only)  the same member groups stepping NB utterances together
 *   TTSC_LSTM_PATH_RESIDENT      lstm_seq_resident_kernel / lstm_bwd_resident_kernel   H = 64 / 128, one workgroup per sequence */
#define TTSC_LSTM_PATH_SEQ 0
#define TTSC_LSTM_PATH_SPLIT 1
#define TTSC_LSTM_PATH_SPLIT_RES 2
#define TTSC_LSTM_PATH_SPLIT_RES_NB 3
#define TTSC_LSTM_PATH_RESIDENT 4
int32_t ttsc_lstm_train_path(int32_t B, int32_t ndir, int32_t H, int32_t backward, int32_t* info);
/* Training of the WaveRNN vocoder (`WaveRNN._train_forward` cube/networks/modules.py:505-539 + `training_step` 553-563: torch.nn.GRU
 * over the teacher-forced sequence, differentiated by torch autograd).  Gate order r,z,n; one layer, unidirectional:
 *   ttsc_gru_pack_whh_device  weight_hh [3H,H] (device) -> out_dev [3H*H]: forward (transpose=0) / backward (transpose=1) packing
 *   ttsc_gru_seq_forward      xg = W_ih x + b_ih [B,T,3H] -> y [B,T,H]; saved_dev [B,T,4H] (r,z,n,W_hn h + b_hn) or NULL (inference)
 *   ttsc_gru_seq_backward     dy [B,T,H] -> dgi [B,T,3H] (grad wrt W_ih x + b_ih), dgh [B,T,3H] (grad wrt W_hh h + b_hh);
 *                             the caller finishes with GEMMs: dx = dgi W_ih, dW_ih = dgi^T x, dW_hh = dgh^T h_prev, biases = sums */
/* With few utterances (B * G <= number of CUs) both recurrences split every utterance over G workgroups (env TTSC_GRU_SPLIT caps
 * G, default 4, 1 = off) that exchange the state through y / dgh once per step; launches of one process must then be
 * stream-ordered (shared hand-off counters).  ttsc_gru_split_status: 0 = every hand-off since the last call completed, 1 = a spin timed out
 * (sticky until read).  Synchronises the device. */
int32_t ttsc_gru_split_status(void);
int ttsc_gru_pack_whh_device(const float* whh_dev, int32_t H, int32_t transpose, float* out_dev, void* stream);
int ttsc_gru_seq_forward(const float* xg_dev, const float* whh_packed_dev, const float* bhh_dev, float* y_dev, float* saved_dev,
                         const float* h0_dev, int32_t B, int32_t T, int32_t H, void* stream);
int ttsc_gru_seq_backward(const float* dy_dev, const float* saved_dev, const float* y_dev, const float* h0_dev,
                          const float* whhT_packed_dev, float* dgi_dev, float* dgh_dev, int32_t B, int32_t T, int32_t H, void* stream);
/* Which kernels ttsc_gru_seq_forward / ttsc_gru_seq_backward launch for B utterances of hidden size H on the CURRENT device (both directions of
 * time take the same path; the launchers call the same selection).  Returns a path id, < 0 for a bad shape, and fills info[3] = {G members per
 * utterance, 1, 1}:
 *   TTSC_GRU_PATH_SEQ        gru_seq_kernel / gru_bwd_kernel                      one workgroup per utterance
 *   TTSC_GRU_PATH_SPLIT      gru_seq_split_kernel / gru_bwd_split_kernel          G streaming members per utterance, counter hand-off
 *   TTSC_GRU_PATH_SPLIT_RES  gru_seq_split_res_kernel / gru_bwd_split_res_kernel  W_hh in registers over G members, granule hand-off */
#define TTSC_GRU_PATH_SEQ 0
#define TTSC_GRU_PATH_SPLIT 1
#define TTSC_GRU_PATH_SPLIT_RES 2
int32_t ttsc_gru_train_path(int32_t B, int32_t H, int32_t backward, int32_t* info);
/* frees a device buffer returned by a ttsc_*_pack_* function */
void ttsc_device_free(void* p);

/* ------------------------------------------------------------------------------------------------
 * Autoregressive mel decoder loop of CubenetTextcoder as one persistent kernel.  Replaces the python loop at
 * cube/networks/textcoder.py:174-185: per step PreNet (modules.py:159-164, dropout p=0.5 always on) -> 2-layer LSTM step
 * -> Linear H->O (three 80-bin frames) -> feedback of the last frame.  The caller hoists the overlay part of the layer-1
 * input projection: xg1_dev [B,S,4H] = overlay . W_ih1[:, :overlay]^T + b_ih1 + b_hh1 (ttsc_linear_forward).
 * masks_dev: {0,1} floats [B,S,2,P] (injected dropout masks) or NULL (Bernoulli(0.5) from Philox(seed)); steps_dev int32
 * [B] or NULL (all S); y_dev [B,S,O] pre-postnet mel (zeros beyond an utterance's steps).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ttsc_melar ttsc_melar;
int ttsc_melar_create(int32_t H, int32_t P, int32_t M, int32_t O, ttsc_melar** out);
int ttsc_melar_set_weights(ttsc_melar* m, const float* w_ih1, int64_t ld1, const float* w_hh1, const float* w_ih2,
                           const float* w_hh2, const float* b_ih2, const float* b_hh2, const float* w_out, const float* b_out,
                           const float* pn_w1, const float* pn_b1, const float* pn_w2, const float* pn_b2);
/* With few utterances (G * B <= number of CUs; G <= 8, env TTSC_MELAR_SPLIT caps it, 1 = off) the decode loop of one utterance is
 * split over G workgroups (each owns H/G units of both LSTM layers; h1 / h2 exchanged every step, protocol of
 * ttsc_lstm_split_status); results differ from the single-workgroup kernel in summation order only. */
int32_t ttsc_melar_split_status(void);
int ttsc_melar_decode(const ttsc_melar* m, const float* xg1_dev, int32_t B, int32_t S, const float* masks_dev, uint64_t seed,
                      const int32_t* steps_dev, float* y_dev, void* stream);
/* The split factor ttsc_melar_decode picks for B rows on the current device (env cap included); 0 for a bad argument. */
int32_t ttsc_melar_members(const ttsc_melar* m, int32_t B);
/* The ragged entry of a batched synthesis: one Philox key per row.  keys_dev uint64 [B] on the device (required when masks_dev is NULL):
 * row b draws its masks with key keys[b] and counter (unit >> 2, t, 0, layer) — the row index is NOT in the counter, so row b gets exactly
 * the masks ttsc_melar_decode(B = 1, seed = keys[b]) draws, wherever it stands in the batch, and every split member of a row draws the same.
 * steps_dev is required.  members: 0 = the rule of ttsc_melar_decode for this B; 1, 2, 4 or 8 force that split — refused (TTSC_EINVAL,
 * nothing launched) when the sizes do not split that way, when members * B exceeds the CU count (the members of a row spin on each other
 * and must be co-resident) or when B > 1024 with members > 1.  Row b is bit-identical to its solo decode at the same split. */
int ttsc_melar_decode_ragged(const ttsc_melar* m, const float* xg1_dev, int32_t B, int32_t S, const float* masks_dev,
                             const uint64_t* keys_dev, const int32_t* steps_dev, int32_t members, float* y_dev, void* stream);
void ttsc_melar_destroy(ttsc_melar* m);

/* Device-side duration -> alignment (row f2 of SURVEY.md §8; replaces the host round trip of
 * cube/networks/modules.py:946-953,1043-1053 and cube/networks/textcoder.py:160-166,291-302).
 * ttsc_align_durations: logits [B,N,D] fp32 (duration head) -> durs [B,N] int32 = argmax over D (first maximum; 0 beyond
 *   len_dev[b], len_dev NULL = N), f2p [B,Fcap] int32 frame -> phone map (phone p repeated durs[b,p] times, in order),
 *   flen [B] int32 = number of frames (clamped to Fcap).
 * ttsc_expand_rows: out [B,F,C] = rows of x [B,N,C] gathered through every stride-th entry of f2p; frames beyond an
 *   utterance's own count repeat its last aligned row (stride 1) or row N-1 (stride > 1), as the reference's gathers pad. */
int ttsc_align_durations(const float* logits_dev, const int32_t* len_dev, int32_t B, int32_t N, int32_t D, int32_t* durs_dev,
                         int32_t* f2p_dev, int32_t* flen_dev, int32_t Fcap, void* stream);
int ttsc_expand_rows(const float* x_dev, const int32_t* f2p_dev, const int32_t* flen_dev, int32_t B, int32_t N, int32_t C, int32_t Fcap,
                     int32_t stride, int32_t F, float* out_dev, void* stream);
/* Input of Languasito2's conditioning recurrence in one launch (cube/networks/modules.py:962-994: vuv = round(p[..., 1]), pitch = p[..., 0] * max_pitch * vuv,
 * cat[expand(g), pitch / max_pitch]): out [B,F,Cp] = rows of g [B,N,C] gathered through f2p (ttsc_expand_rows' rule at stride 1), column C = pitch * (1 / max_pitch),
 * columns C + 1 .. Cp - 1 zero (Cp = C + 1 rounded up to the split GEMM's multiple of 4); pitch [B,F] is written too.  pitch_out_dev [B,F,2] = the pitch head's
 * sigmoid outputs. */
int ttsc_cond_input(const float* g_dev, const int32_t* f2p_dev, const int32_t* flen_dev, const float* pitch_out_dev, float max_pitch, int32_t B, int32_t N,
                    int32_t C, int32_t Cp, int32_t Fcap, int32_t F, float* pitch_dev, float* out_dev, void* stream);

/* Prosody control inside those two launches (csrc/prosody.hip).  Under the identity controls both give their uncontrolled twin's
 * outputs bit for bit; a call without controls uses the twins themselves.
 * ttsc_align_durations_ctl: ttsc_align_durations with, per phone, dur_scale_q16_dev int32 [B,N] (duration multiplier in Q16, 65536 = unchanged;
 *   NULL = 65536 everywhere) and dur_set_dev int32 [B,N] (-1 = none, >= 0 = exactly that many frames; NULL = none), and dcap = the largest frame
 *   count of one phone.  With d = the argmax, per row over p < len[b] in order, in integers:
 *     acc = 0 (int64, Q16); emitted = 0
 *     set[p] >= 0: nd = min(set[p], dcap); emitted += nd; acc = emitted << 16
 *     d == 0:      nd = 0
 *     else:        acc += d * scale[p]; nd = ((acc + 32768) >> 16) - emitted; nd = min(max(nd, 1), dcap); emitted += nd
 *   durs[b,p] = nd; f2p and flen = min(emitted, Fcap) as ttsc_align_durations writes them.  The rounding error is carried, so the row's total
 *   follows the requested tempo; a phone that had frames keeps at least one.
 * ttsc_cond_input_ctl: ttsc_cond_input with pitch_mul_dev float [B,N] (per phone) and pitch_range_dev float [B] (per row).  A voiced frame
 *   (vuv == 1) with p0 = (o0 * max_pitch) * vuv becomes, every operation rounded on its own in float32,
 *     1. pitch_range[b] != 1 and the row has a voiced frame f < flen[b]:  p = m + pitch_range[b] * (p0 - m)
 *     2. p = p * pitch_mul[b, row(f)];  p = min(max(p, 0), max_pitch)
 *   m = float32(sum / count) of p0 over the row's voiced frames f < flen[b], summed in float64: lane t of 64 adds frames t, t + 64, ... in that
 *   order, the 64 partial sums are folded pairwise (part[t] += part[t + off], off = 32 .. 1).  The mean is formed inside the same launch by the
 *   workgroups that need it: no launch is added, and a row's result does not depend on the rest of the batch.  Unvoiced frames stay 0. */
int ttsc_align_durations_ctl(const float* logits_dev, const int32_t* len_dev, int32_t B, int32_t N, int32_t D, int32_t* durs_dev,
                             int32_t* f2p_dev, int32_t* flen_dev, int32_t Fcap, const int32_t* dur_scale_q16_dev, const int32_t* dur_set_dev,
                             int32_t dcap, void* stream);
int ttsc_cond_input_ctl(const float* g_dev, const int32_t* f2p_dev, const int32_t* flen_dev, const float* pitch_out_dev, float max_pitch, int32_t B,
                        int32_t N, int32_t C, int32_t Cp, int32_t Fcap, int32_t F, float* pitch_dev, float* out_dev, const float* pitch_mul_dev,
                        const float* pitch_range_dev, void* stream);

/* STFT-magnitude / mel-spectrogram helpers around ttsc_linear_forward (the DFT and the mel projection are GEMMs):
 * hifigan.meldataset.mel_spectrogram [EXTERNAL; cube/networks/cubegan.py:137-138,247-248 — the 45 x mel-L1 loss of the GAN step,
 * forward and backward] and MelVocoder.melspectrogram (cube/io_utils/vocoder.py:54-98, feature extraction, row f4).
 *   ttsc_stft_mag            reim [M, 2*NB] (re | im) -> mag [M, ldm] = sqrt(re^2 + im^2 + eps)  (columns >= NB zeroed)
 *   ttsc_stft_mag_backward   d(re|im) = dmag * (re|im) / mag
 *   ttsc_log_clamp           y = scale * ln(max(x, minv))  (scale 1: natural log; 1/ln 10: log10);  _backward: dx = dy*scale/x above minv
 *   ttsc_overlap_add         backward of the framing: y [B, Lp] = sum of frames [B, F, n_fft] at hop (fixed summation order) over the first
 *                            F_used rows of each utterance (the rest are rows of a batched DFT that straddle into the next utterance) */
int ttsc_stft_mag(const float* reim_dev, int64_t M, int32_t NB, int32_t ldm, float eps, float* mag_dev, void* stream);
int ttsc_stft_mag_backward(const float* dmag_dev, const float* reim_dev, const float* mag_dev, int64_t M, int32_t NB, int32_t ldm,
                           float* dreim_dev, void* stream);
int ttsc_log_clamp(const float* x_dev, int64_t n, float minv, float scale, float* y_dev, void* stream);
int ttsc_log_clamp_backward(const float* dy_dev, const float* x_dev, int64_t n, float minv, float scale, float* dx_dev, void* stream);
int ttsc_overlap_add(const float* frames_dev, int32_t B, int32_t F, int32_t F_used, int32_t n_fft, int32_t hop, int64_t Lp, float* y_dev, void* stream);

/* CubenetTextcoder training (cube/networks/textcoder.py:191-226; csrc/textcoder_train.hip).
 *   ttsc_bn_tanh_dropout_train_forward   the PostNet block after a convolution in TRAINING mode, one launch: per-channel mean / biased
 *                                        variance of x [B, C, F] over B x F (fixed order), y = keep * tanh(gamma x_hat + beta) / (1 - p),
 *                                        running_mean / running_var updated with `momentum` (unbiased variance, as torch); mean / invstd saved.
 *                                        mask_dev: {0,1} floats [B, C, F], or null = Philox-4x32-10 keyed by `seed`, counter word 2 = `layer`.
 *                                        B * F must exceed 1 (torch's BatchNorm raises there too).
 *   ttsc_bn_tanh_dropout_train_backward  dx, dgamma, dbeta from dy (the same mask / seed / layer as the forward call).
 *   ttsc_textcoder_loss                  the step's four loss terms in one launch: out[0] CE(duration), out[1] CE(pitch) (mean over the rows whose
 *                                        target is not ignore_index), out[2] mean|pre - t|, out[3] mean|post - t| (n values each, n % 4 == 0, 16-byte
 *                                        aligned), and the gradients of all four operands.  A target outside [0, K) that is not ignore_index
 *                                        contributes nothing and sets *status_dev |= 1 (duration) / 2 (pitch); no device assert.
 *                                        Workspace: ttsc_textcoder_loss_workspace_bytes(Rd, Rp, n). */
int ttsc_bn_tanh_dropout_train_forward(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* running_mean_dev, float* running_var_dev,
                                       int32_t B, int32_t C, int32_t F, float momentum, float eps, float p, const float* mask_dev, uint64_t seed,
                                       int32_t layer, float* y_dev, float* mean_dev, float* invstd_dev, void* stream);
int ttsc_bn_tanh_dropout_train_backward(const float* dy_dev, const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                                        const float* invstd_dev, int32_t B, int32_t C, int32_t F, float p, const float* mask_dev, uint64_t seed,
                                        int32_t layer, float* dx_dev, float* dgamma_dev, float* dbeta_dev, void* stream);
size_t ttsc_textcoder_loss_workspace_bytes(int32_t Rd, int32_t Rp, int64_t n);
int ttsc_textcoder_loss(const float* dur_logits_dev, const int64_t* dur_target_dev, int32_t Rd, int32_t Kd, const float* pitch_logits_dev,
                        const int64_t* pitch_target_dev, int32_t Rp, int32_t Kp, const float* pre_dev, const float* post_dev, const float* mel_target_dev,
                        int64_t n, int64_t ignore_index, float* out_dev, float* g_dur_dev, float* g_pitch_dev, float* g_pre_dev, float* g_post_dev,
                        int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Sentence phonemizer (cube/networks/phonemizer.py:12-103 CubenetPhonemizer, cube/io_utils/io_text.py:13-61; csrc/phonemizer.hip).
 *   ttsc_char_features   the tagger's input in one launch: out [B, Ec + Es, N] (channel-major, what ttsc_conv1d_forward reads) =
 *                        cat[char_table[x_char], case_table[x_case]] permuted, zero at positions n >= len_dev[b] (len_dev NULL: none).  Tables are
 *                        [G, Ec] and [Gc, Es]; an id outside its table writes zeros and sets bit 1 of the phonemizer status word.
 *   ttsc_tag_argmax      tags[m] = index of the FIRST maximum of x[m, :K] . W[P, K]^T + bias (torch.argmax's rule; bias may be NULL), 0 for
 *                        rows at or beyond their utterance's length (len_dev [M / period], rows are [utterance][period]; NULL: every row counts).
 *                        logits_dev [M, P] may be NULL (the product path never writes them); padding rows get zeros there.  K % 4 == 0,
 *                        ldx % 4 == 0, 16-byte aligned x / W, K + P <= 4096.  fp32 accumulation, k = 0 .. K-1 in order per (row, class): the
 *                        result of a row does not depend on M or on the rows around it.
 *   ttsc_masked_ce       *loss_dev = mean over the rows whose target != ignore_index of CE(logits[r, :K], target[r]) — 0 when there is no such
 *                        row (torch gives NaN there) — and dlogits [R, K] = d loss / d logits (already divided by the row count; ignored rows
 *                        zero).  Deterministic (fixed-order two-stage reduction).  A target outside [0, K) that is not ignore_index
 *                        contributes nothing, sets bit 2 of the phonemizer status word and, when status_dev is given, *status_dev = 2 (else 0).
 *                        Workspace: ttsc_masked_ce_workspace_bytes(R).
 *   ttsc_phonemizer_status   the sticky per-device status word of the kernels above (bit 1 | bit 2), cleared by the read; synchronises. */
int ttsc_char_features(const int32_t* x_char_dev, const int32_t* x_case_dev, const float* char_table_dev, const float* case_table_dev,
                       const int32_t* len_dev, int32_t B, int32_t N, int32_t G, int32_t Ec, int32_t Gc, int32_t Es, float* out_dev, void* stream);
int ttsc_tag_argmax(const float* x_dev, const float* w_dev, const float* bias_dev, const int32_t* len_dev, int32_t period, int64_t M, int32_t P,
                    int32_t K, int64_t ldx, int32_t* tags_dev, float* logits_dev, void* stream);
size_t ttsc_masked_ce_workspace_bytes(int32_t R);
int ttsc_masked_ce(const float* logits_dev, const int64_t* target_dev, int32_t R, int32_t K, int64_t ignore_index, float* loss_dev,
                   float* dlogits_dev, int32_t* status_dev, void* ws_dev, size_t ws_bytes, void* stream);
int32_t ttsc_phonemizer_status(void);

/* Word-level G2P (cube/networks/modules.py:58-88, 208-297 Seq2Seq + Attention in eval mode; cube/networks/g2p.py; csrc/g2p.hip).
 *   ttsc_g2p_decode   the autoregressive attention decoder of Seq2Seq.forward as ONE launch, one workgroup per word and no communication between
 *                     workgroups.  Per step: query = CELL state of the last decoder layer -> energy_n = tanh(W_att[:, :D] q + pe_n) ->
 *                     attention = softmax over ALL n_b positions of v . energy_n (padding included, as the reference) -> context -> two LSTM
 *                     layers -> logits = W_out h2 + b -> the fed-back label (first maximum of the logits, or gs[b, t]).  The start state is
 *                     the state after one step on a zero input from a zero state; the first fed-back embedding is zero.
 *                     The caller hoists pe = enc . W_att[:, D:]^T + b_att [B, Nmax, A] and tab = output_emb . W_ih0[:, E:]^T [L, 4D]
 *                     (ttsc_linear_forward); matrices are packed [K/4][rows][4] (see ttsc_lstm_pack_whh), biases are b_ih + b_hh.
 *                     n_dev [B]: the padded length of each word (1 .. Nmax; NULL: Nmax) — words of different batches share a launch and each
 *                     sees the padding it would see alone.  A word's encoder rows stay in LDS while they fit (64 KiB), else they are read from
 *                     global memory: no n is refused.  scratch_dev: 2 * B * Nmax floats.
 *                     stop != 0: a word ends with its first label == eos, at the latest after min(T, 10 * n_b + 1) steps; else every word runs T
 *                     steps.  idx_dev [B, T] int32 labels (0 beyond a word's steps), count_dev [B] steps run, logits_dev [B, T, L] (zeros beyond
 *                     a word's steps); each may be NULL.  gs_dev [B, T] int32 teacher labels or NULL.  D, E, A multiples of 4.
 *                     A teacher label outside [0, L) feeds back zeros and sets bit 2 of the G2P status word; an n_b outside [1, Nmax] is
 *                     clamped and sets bit 4.
 *   ttsc_g2p_embed    out [R, Em] = table[ids[r]] (table [G, Em]); an id outside the table writes zeros and sets bit 1 of the status word.
 *   ttsc_g2p_status   the sticky per-device status word of the two (bits 1 | 2 | 4), cleared by the read; synchronises. */
typedef struct ttsc_g2p_args {
    const float* enc_dev;      /* [B, Nmax, E] encoder states */
    const float* pe_dev;       /* [B, Nmax, A] */
    const int32_t* n_dev;      /* [B] or NULL */
    const int32_t* gs_dev;     /* [B, T] or NULL */
    const float* w_aq;         /* W_att[:, :D] packed [D/4][A][4] */
    const float* v;            /* [A] */
    const float* w_ic;         /* W_ih0[:, :E] packed [E/4][4D][4] */
    const float* tab;          /* [L, 4D] */
    const float* w_hh0;        /* packed [D/4][4D][4] */
    const float* b0;           /* [4D] */
    const float* w_ih1;        /* packed [D/4][4D][4] */
    const float* w_hh1;        /* packed [D/4][4D][4] */
    const float* b1;           /* [4D] */
    const float* w_out;        /* packed [D/4][L][4] */
    const float* b_out;        /* [L] */
    float* scratch_dev;        /* [2, B, Nmax] */
    int32_t* idx_dev;          /* [B, T] or NULL */
    int32_t* count_dev;        /* [B] or NULL */
    float* logits_dev;         /* [B, T, L] or NULL */
    int32_t B, Nmax, T, E, A, D, L, eos, stop;
} ttsc_g2p_args;
int ttsc_g2p_decode(const ttsc_g2p_args* args, void* stream);
int ttsc_g2p_embed(const int32_t* ids_dev, const float* table_dev, int64_t R, int32_t G, int32_t Em, float* out_dev, void* stream);
int32_t ttsc_g2p_status(void);

/* G2P training (modules.py:258-297 Seq2Seq.forward with gs_output in TRAIN mode; csrc/g2p_train.hip).  One workgroup per word, nothing between
 * workgroups.  Row r = 0 of every saved tensor is the start step (zero input, zero state), row r = t + 1 is teacher-forced step t.
 *   ttsc_g2p_train_forward    the start step and all T steps in one launch.  Per step: aq = W_att[:, :D] . c2 (CELL state of the top layer),
 *                             energy = keep_att * tanh(aq + pe_i) / (1 - p_att), attention = softmax over ALL N positions of v . energy, context,
 *                             layer 0 on [context; output_emb(y[t - 1])] (zero embedding at t = 0; the embedding enters as tab = output_emb .
 *                             W_ih0[:, E:]^T), keep_dec / (1 - p_dec) on layer 0's h towards layer 1 (a fresh mask every row, the start step
 *                             included), layer 1.  Saves activated gates (i, f, g, o) and cell states of both layers, h1, the masked h1, h2, aq,
 *                             the attention weights and the contexts (into columns [0, E) of the decoder-input rows x0 [B, T + 1, E + Em], whose
 *                             other entries the caller fills).  The energies are not stored: the backward recomputes them from aq.  No logits:
 *                             under teacher forcing they are one GEMM over the rows of h2.
 *   ttsc_g2p_train_backward   the reverse loop in one launch from dh2 [B, T, D]: gate gradients of both layers for all T + 1 rows (the rows of
 *                             the weight-gradient GEMMs), dq [B, T + 1, A] (row 0 untouched: the caller zeroes it), and per word denc [B, N, E]
 *                             (through the context only), dpe [B, N, A] and dv [B, A], accumulated over t descending by the owning thread: no
 *                             atomics, the same bits every run.  Streams [W_ih1^T; W_hh1^T], [W_hh0^T; W_ic^T] and W_aq^T in the forward packing.
 *   Masks: {0,1} floats, or NULL = Philox-4x32-10, counter (element >> 2, row, word, tag + stream_id), key = seed (p = 0: everything kept).
 *   A label outside [0, L) feeds zeros and sets bit 2 of the G2P status word (ttsc_g2p_status).  D, E, A multiples of 4.
 *   ttsc_dropout_scale        y[i] = x[i] * keep[i] / (1 - p): mask_dev {0,1} floats [n], or NULL = Philox keyed by (seed, stream_id).  Its
 *                             adjoint is the same call on dy. */
typedef struct ttsc_g2p_train_args {
    const float* enc_dev;        /* [B, N, E] */
    const float* pe_dev;         /* [B, N, A] = enc . W_att[:, D:]^T + b_att */
    const int32_t* y_dev;        /* [B, T] teacher labels */
    const float* w_aq;           /* W_att[:, :D] packed [D/4][A][4] */
    const float* v;              /* [A] */
    const float* w_ic;           /* W_ih0[:, :E] packed [E/4][4D][4] */
    const float* tab;            /* [L, 4D] */
    const float* w_hh0;          /* packed [D/4][4D][4] */
    const float* b0;             /* [4D] b_ih + b_hh */
    const float* w_ih1;          /* packed [D/4][4D][4] */
    const float* w_hh1;          /* packed [D/4][4D][4] */
    const float* b1;             /* [4D] */
    const float* w_l1t;          /* [W_ih1^T; W_hh1^T] ([2D, 4D]) packed [4D/4][2D][4]   (backward) */
    const float* w_l0t;          /* [W_hh0^T; W_ic^T] ([D + E, 4D]) packed [4D/4][D + E][4]   (backward) */
    const float* w_aqt;          /* W_att[:, :D]^T ([D, A]) packed [A/4][D][4]   (backward) */
    const float* att_mask_dev;   /* [B, T, N, A] {0,1} or NULL */
    const float* dec_mask_dev;   /* [B, T + 1, D] {0,1} or NULL */
    float* gates0_dev;           /* [B, T + 1, 4D] saved */
    float* cells0_dev;           /* [B, T + 1, D] */
    float* h1_dev;               /* [B, T + 1, D] */
    float* h1m_dev;              /* [B, T + 1, D] h1 through the inter-layer dropout */
    float* gates1_dev;           /* [B, T + 1, 4D] */
    float* cells1_dev;           /* [B, T + 1, D] */
    float* h2_dev;               /* [B, T + 1, D] */
    float* aq_dev;               /* [B, T, A] */
    float* att_dev;              /* [B, T, N] */
    float* x0_dev;               /* [B, T + 1, E + Em]; the forward writes columns [0, E) of rows 1 .. T */
    const float* dh2_dev;        /* [B, T, D]   (backward) */
    float* dgates0_dev;          /* [B, T + 1, 4D]   (backward outputs) */
    float* dgates1_dev;          /* [B, T + 1, 4D] */
    float* dq_dev;               /* [B, T + 1, A] */
    float* denc_dev;             /* [B, N, E] */
    float* dpe_dev;              /* [B, N, A] */
    float* dv_dev;               /* [B, A] */
    float* scratch_dev;          /* [B, 2, N] */
    uint64_t seed;
    int32_t B, N, T, E, A, D, L, Em, stream_id;
    float p_att, p_dec;
} ttsc_g2p_train_args;
int ttsc_g2p_train_forward(const ttsc_g2p_train_args* args, void* stream);
int ttsc_g2p_train_backward(const ttsc_g2p_train_args* args, void* stream);
int ttsc_dropout_scale(const float* x_dev, int64_t n, float p, const float* mask_dev, uint64_t seed, int32_t stream_id, float* y_dev, void* stream);

/* Pitch tracker of the corpus importer (csrc/pitch.hip; io_utils/pitch.py; the float64 statement is tests/pitch_reference.py): a single-rate RAPT
 * (Talkin 1995) without the decimated first pass and without the spectral-stationarity term.  Two launches for a batch of ragged utterances.
 *   nccf    x [B, Lmax] float32 in [-1, 1], len [B]; F_b = len[b] / hop frames, Fmax = Lmax / hop rows per utterance; window n, lags kmin .. kmax
 *           (K = kmax - kmin + 1, kmax >= kmin + 2).  Frame t starts at t * hop, samples at or past len[b] read as zero, the mean of its n + kmax
 *           samples is removed, phi[k] = sum_{j<n} s[j] s[j+k] / sqrt(e_0 e_k + A).  Writes the 20 largest peaks with phi >= 0.3 max phi, largest
 *           first, ties to the smaller lag, each refined by a parabola: cand_lag / cand_val [B, Fmax, 20] (unused slots 0), ncand [B, Fmax],
 *           maxphi [B, Fmax], rms [B, Fmax] of the window, and phi [B, Fmax, K] when phi_dev is not NULL.  Rows t >= F_b are written as zeros.
 *   track   Viterbi over 21 states per frame (candidates 0 .. ncand - 1, state 20 = unvoiced) from those tables (or injected ones) for nframes[b]
 *           frames, ties to the lowest state; f0 [B, Fmax] = sample_rate / lag of the chosen candidate, 0 where unvoiced and past nframes[b].
 *           workspace: ttsc_pitch_track_workspace_bytes(B, Fmax) bytes of back-pointers. */
int ttsc_pitch_nccf(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t hop, int32_t n, int32_t kmin, int32_t kmax,
                    float* cand_lag_dev, float* cand_val_dev, int32_t* ncand_dev, float* maxphi_dev, float* rms_dev, float* phi_dev, void* stream);
size_t ttsc_pitch_track_workspace_bytes(int32_t B, int64_t Fmax);
int ttsc_pitch_track(const float* cand_lag_dev, const float* cand_val_dev, const int32_t* ncand_dev, const float* maxphi_dev, const float* rms_dev,
                     const int32_t* nframes_dev, int32_t B, int64_t Fmax, int32_t kmax, float sample_rate, void* workspace_dev, size_t workspace_bytes,
                     float* f0_dev, void* stream);

/* Dynamic time warping of the dev-set evaluation (csrc/dtw.hip; io_utils/evaluate.py; the float64 and float32 statements are
 * tests/dtw_reference.py): P ragged pairs of feature sequences aligned in one launch, one workgroup per pair.
 *   a [P, Na_max, K], b [P, Nb_max, K] float32, contiguous; len_a, len_b [P] int32 ON THE DEVICE (clamped to [0, Na_max] / [0, Nb_max]); 1 <= K <= 80.
 *   d(i, j) = sqrt(sum_k (a[i,k] - b[j,k])^2) from the differences, float32, ascending k, every operation rounded on its own;
 *   D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) from (0, 0) to (len_a - 1, len_b - 1), steps unweighted; ties go to the diagonal,
 *   then to (i-1, j), then to (i, j-1) (strict <, taken in that order).
 *   cost [P] float32 = D at the end cell; plen [P] int32; path_a, path_b [P, Na_max + Nb_max - 1] int32 in forward order, -1 behind plen.  A pair
 *   with len_a == 0 or len_b == 0 gets plen 0, cost 0 and paths of -1.  Rows at or beyond a pair's own lengths are never read: a pair's bits do
 *   not depend on the batch around it.
 * The local costs are formed inside the launch (no Na x Nb matrix reaches memory), the back-pointers go to the workspace
 * (ttsc_dtw_workspace_bytes(P, Na_max, Nb_max) bytes, 16-byte aligned: one byte per cell of 64-column blocks, the boundary column between blocks
 * and the reversed path) and are walked back in the same launch; all index arithmetic is 64-bit and nothing synchronises with the host.
 * Checked before the launch (nonzero status, the last-error text set): P < 0, K outside 1 .. 80, negative or >= 2^30 lengths, a NULL pointer with
 * a nonzero size, a workspace that is too small or misaligned.  P == 0 launches nothing. */
size_t ttsc_dtw_workspace_bytes(int32_t P, int64_t Na_max, int64_t Nb_max);
int ttsc_dtw_align(const float* a_dev, const float* b_dev, const int32_t* len_a_dev, const int32_t* len_b_dev, int32_t P, int64_t Na_max,
                   int64_t Nb_max, int32_t K, void* workspace_dev, size_t workspace_bytes, float* cost_dev, int32_t* plen_dev, int32_t* path_a_dev,
                   int32_t* path_b_dev, void* stream);

/* Forced aligner (csrc/forced_align.hip; io_utils/forced_align.py; the float32 and float64 statements are tests/forced_align_reference.py): a
 * time-synchronous Viterbi search of a ragged batch of utterances through left-to-right lattices of diagonal-Gaussian states, and the statistics
 * of its alignments for Viterbi re-estimation.  Limits, from the 42 KiB of LDS of the search (8 frames x 1024 positions of emissions, two rows of
 * scores, 8 feature rows): Smax <= 1024 positions per utterance, D <= 63 feature dimensions.
 *   viterbi   feat [B, Tmax, D] float32, nframes [B] int32 (clamped to [0, Tmax]); the lattice of utterance b: state [B, Smax] int32 (model-state
 *             id per position), skip [B, Smax] int32 (one extra predecessor < j, or -1), start / final [B, Smax] uint8 flags, npos [B] int32
 *             (clamped to [0, Smax]); the model: mean, ivar [M, D], cst [M] float32.  All ON THE DEVICE.  In float32, every operation rounded on
 *             its own: acc = 0; for ascending d: diff = x[d] - mean[m][d], acc = acc + (diff * diff) * ivar[m][d]; e = cst[m] - 0.5f * acc;
 *             v_0[j] = start[j] ? e_0[j] : -inf; v_t[j] = e_t[j] + best of v_{t-1}[j], v_{t-1}[j-1], v_{t-1}[skip[j]], taken in that order with
 *             strict > (ties stay on the earlier candidate); the end is the final position with the largest v_{T-1}, ties to the lowest index.
 *             align [B, Tmax] int32 = position per frame, -1 behind nframes; score [B] float32; ok [B] int32.  An utterance with nframes == 0,
 *             npos == 0 or no finite path (fewer frames than mandatory positions) gets ok 0, score 0 and -1 throughout.  Nothing at or beyond
 *             an utterance's own nframes / npos is read: its bits do not depend on the batch around it.  The back-pointers go to the workspace
 *             (ttsc_fa_workspace_bytes(B, Tmax, Smax) bytes, 16-byte aligned: one byte per cell, 64-bit index arithmetic) and are walked back
 *             in the same launch; nothing synchronises with the host.
 *             Checked before the launch (nonzero status, the last-error text set): negative sizes, Tmax >= 2^30, Smax > 1024, D outside 1 .. 63,
 *             a NULL pointer with a nonzero size, a workspace that is too small or misaligned.  B == 0 launches nothing.
 *   check_lattice   the lattice tables live on the device, where a launch cannot be refused over their contents without a synchronisation; this
 *             entry point takes their HOST copies before they are uploaded (the Python wrapper always calls it) and refuses npos outside
 *             0 .. Smax, a state id outside 0 .. M - 1, a skip that is neither -1 nor an earlier position, and flags other than 0 / 1.  Inside
 *             the kernel a position with a state id outside the model is closed (-inf) and a skip outside -1 .. j - 1 is taken as -1, so
 *             unchecked tables cannot make it read out of bounds either.
 *   accumulate   adds the statistics of the aligned frames into running float64 tables count [M], sum [M, D], sumsq [M, D]: per (utterance,
 *             position) the sums of x and x * x over the frames with align == position in ascending t (x widened to double first, x * x taken in
 *             double); per model state those segment sums (segments without a frame left out) are added in ascending (b, position); that batch
 *             total is added ONCE to the running table.  Utterances with ok == 0 contribute nothing.  No atomics; the result does not depend on
 *             the launch geometry.  workspace: ttsc_fa_accumulate_workspace_bytes(B, Smax, D) bytes, 16-byte aligned (the segment sums). */
size_t ttsc_fa_workspace_bytes(int32_t B, int64_t Tmax, int32_t Smax);
int ttsc_fa_check_lattice(const int32_t* state, const int32_t* skip, const uint8_t* start, const uint8_t* final_, const int32_t* npos, int32_t B,
                          int32_t Smax, int32_t M);
int ttsc_fa_viterbi(const float* feat_dev, const int32_t* nframes_dev, const int32_t* state_dev, const int32_t* skip_dev, const uint8_t* start_dev,
                    const uint8_t* final_dev, const int32_t* npos_dev, const float* mean_dev, const float* ivar_dev, const float* cst_dev, int32_t B,
                    int64_t Tmax, int32_t Smax, int32_t D, int32_t M, void* workspace_dev, size_t workspace_bytes, int32_t* align_dev,
                    float* score_dev, int32_t* ok_dev, void* stream);
size_t ttsc_fa_accumulate_workspace_bytes(int32_t B, int32_t Smax, int32_t D);
int ttsc_fa_accumulate(const float* feat_dev, const int32_t* nframes_dev, const int32_t* align_dev, const int32_t* ok_dev, const int32_t* state_dev,
                       const int32_t* npos_dev, int32_t B, int64_t Tmax, int32_t Smax, int32_t D, int32_t M, void* workspace_dev,
                       size_t workspace_bytes, double* count_dev, double* sum_dev, double* sumsq_dev, void* stream);

/* Rational-rate polyphase FIR resampler of the audio readers (csrc/resample.hip; io_utils/resample.py; the float64 statement is
 * tests/resample_reference.py): scipy.signal.resample_poly(x, up, down) with its default Kaiser-5 filter, for a ragged batch in one launch.
 *   x [B, Lmax] float32, len [B] (clamped to [0, Lmax]); up, down coprime, both in [1, 1024]; half = 10 max(up, down), K = ceil((2 half + 1) / up).
 *   taps: the filter h[0 .. 2 half] (already multiplied by up) padded with zeros to ntaps = up * K4 floats, K4 = K rounded up to a multiple of 4.
 *   y [B, Omax], Omax >= ceil(Lmax up / down): row b holds y[n] = sum_i x[i] h[n down - i up + half] over |n down - i up| <= half for
 *   n < ceil(len[b] up / down), zeros behind; peak [B] = max |y| of the row (0 for an empty row).  fp32 sums in an order that depends on (n, up,
 *   down) alone: a row has the same bits alone and in any batch.  Index arithmetic is 64-bit. */
int ttsc_resample_poly(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t up, int32_t down, const float* taps_dev,
                       int64_t ntaps, float* y_dev, int64_t Omax, float* peak_dev, void* stream);

/* Timeline mixer of StoryCube (csrc/story.hip; io_utils/story_mix.py; ttscube_amd/story.py; the restatement is tests/story_reference.py): the
 * narrated track of cube/story.py in one launch.  out[j], j < n, is timeline sample t = t0 + j:
 *     s = trunc(fl32(speech[seg_src[p] + (t - seg_dst[p])] * 32767))   where seg_dst[p] <= t < seg_dst[p] + seg_len[p], else 0
 *     out[j] = int16(trunc(fl32(fl32(fl32(music[t % M] * music_gain) * music_scale) + s)))
 * three float32 operations rounded one by one (never fused), truncation toward zero: the bits of the reference's per-sample loop.  A sum outside
 * the int16 range (undefined in the reference) saturates to [-32768, 32767] and adds 1 to *clipped_dev when that is not NULL (an integer count:
 * the same value in any order; the caller zeroes it).  Every out[j] is written exactly once; P == 0 is the music bed alone; n == 0 launches nothing.
 *   speech   packed float32 waveforms in (-1, 1); only the elements inside a segment are read
 *   seg_*    [P] int64 ON THE DEVICE: first sample in speech, length >= 0, first sample on the timeline; ascending and non-overlapping
 *            (seg_dst[p] + seg_len[p] <= seg_dst[p + 1]; empty and adjacent segments are fine).  All index arithmetic is 64-bit.
 * Checked here, before any launch (nonzero status, the last-error text set): M < 1, negative P / n / t0, t0 + n beyond 64 bits, a NULL pointer with
 * a nonzero size, misaligned out / clipped.  The segment tables live on the device and are NOT read back here: negative lengths, unsorted or
 * overlapping segments and segments beyond the speech buffer are refused by the caller that still holds host copies
 * (io_utils/story_mix.py::mix_timeline with host tables raises the same error before the launch); tables handed over as device tensors are
 * the caller's promise.  A table that breaks it gives unspecified samples but reads nothing outside [seg_src[p], seg_src[p] + seg_len[p]). */
int ttsc_story_mix(const float* speech_dev, const int64_t* seg_src_dev, const int64_t* seg_len_dev, const int64_t* seg_dst_dev, int32_t P,
                   const float* music_dev, int64_t M, float music_gain, float music_scale, int64_t t0, int64_t n, int16_t* out_dev,
                   int64_t* clipped_dev, void* stream);

/* Complex STFT, inverse STFT and the Griffin-Lim projection on a radix-4 Stockham FFT held in LDS (csrc/stft_fft.hip; io_utils/stft.py; the float64
 * statement is tests/griffinlim_reference.py): the rest of MelVocoder (cube/io_utils/vocoder.py:42-52,69-75,100-124), librosa's conventions:
 * periodic Hann of length n_fft, centred frames over n_fft/2 samples of reflect padding, NB = n_fft/2 + 1 bins, F = 1 + L // hop frames, the
 * inverse returns hop (F - 1) samples.  n_fft in {256, 512, 1024, 2048}, 1 <= hop <= n_fft, else TTSC_EINVAL.
 *   Ragged batches: B rows of frames[b] frames each in buffers [B, Fmax, ...] / [B, L...]; frames_host is the caller's host copy of
 *   frames_dev (int32 [B]; both NULL: every row has Fmax frames) and serves the argument checks: every row needs 1 <= frames[b] <= Fmax and
 *   hop (frames[b] - 1) >= n_fft/2 + 1 samples (reflect padding), else TTSC_EINVAL.  Buffer rows at or beyond a row's own frames / samples are
 *   never read and are written as zeros; a row's bits do not depend on the batch around it.
 *   tables_dev: 3 n_fft floats — n_fft (re, im) twiddles, entry Ns + k = exp(-2 pi i k / (2 Ns)) for Ns = 1, 2 .. n_fft/2, k < Ns (entry 0
 *   unused), then the window; built in float64 and rounded once (io_utils/stft.py::tables).
 *   ttsc_stft_reflect_pad   y [B, Lmax] with len[b] samples (n_fft/2 + 1 .. Lmax) -> out [B, Lpad], Lpad >= Lmax + n_fft: numpy's reflect
 *                           padding by n_fft/2, zeros behind len[b] + n_fft
 *   ttsc_stft_analyze       padded signal [B, Lpad], Lpad >= hop (Fmax - 1) + n_fft -> spectrum [B, Fmax, NB] of interleaved (re, im); frame f
 *                           is read in place at f hop
 *   ttsc_stft_synthesize    spectrum [B, Fmax, NB] -> frames [B, Fmax, n_fft]: the real inverse transform / n_fft, times the window; the
 *                           imaginary parts of bins 0 and n_fft/2 are ignored
 *   ttsc_stft_project       one Griffin-Lim half step in one launch: padded signal, magnitude [B, Fmax, NB] -> frames [B, Fmax, n_fft] of
 *                           |mag| (re, im) / |(re, im)| of the signal's own STFT ((0, 0) has phase (1, 0)); the spectrum never leaves LDS
 *   ttsc_stft_overlap_add   frames [B, Fmax, n_fft] -> sum of the frames at hop, divided by the sum of the squared window where that exceeds
 *                           FLT_MIN (one thread per sample, ascending frames).  padded = 0: the audio [B, ldo = hop (Fmax - 1)];
 *                           padded = 1: the reflect-padded audio [B, ldo = hop (Fmax - 1) + n_fft] that the next ttsc_stft_project reads */
int ttsc_stft_reflect_pad(const float* y_dev, const int32_t* len_host, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t n_fft,
                          float* out_dev, int64_t Lpad, void* stream);
int ttsc_stft_analyze(const float* sig_dev, int64_t Lpad, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax,
                      int32_t n_fft, int32_t hop, const float* tables_dev, float* spec_dev, void* stream);
int ttsc_stft_synthesize(const float* spec_dev, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax, int32_t n_fft,
                         int32_t hop, const float* tables_dev, float* frames_out_dev, void* stream);
int ttsc_stft_project(const float* sig_dev, int64_t Lpad, const float* mag_dev, const int32_t* frames_host, const int32_t* frames_dev,
                      int32_t B, int32_t Fmax, int32_t n_fft, int32_t hop, const float* tables_dev, float* frames_out_dev, void* stream);
int ttsc_stft_overlap_add(const float* frames_in_dev, const int32_t* frames_host, const int32_t* frames_dev, int32_t B, int32_t Fmax,
                          int32_t n_fft, int32_t hop, const float* tables_dev, int32_t padded, float* out_dev, int64_t ldo, void* stream);

/* Segment feed of the HiFi-GAN trainer (csrc/segment_feed.hip; io_utils/segment_feed.py; the numpy restatement is
 * tests/segment_feed_reference.py): a batch of B crops of `frames` frames (frames * hop samples) from a device-resident corpus in one launch.
 * Row b is utterance u = utt[b] from frame s = start_frame[b]:
 *     y_out[b, 0, i]   = float(wav[wav_off[u] + s hop + i]) * gain[u]              0 at and beyond wav_off[u + 1]
 *     mel_out[b, c, t] = mel[(mel_off[u] + s + t) n_mels + c] * mel_scale          mel_pad where s + t >= mel_off[u + 1] - mel_off[u]
 * one float32 product per element; no sums, no atomics: a row has the same bits alone and in any batch.
 *   wav_arena  int16 samples of all U utterances, wav_off [U + 1] int64 (the 16-byte load path needs wav_off[u] + s hop on a multiple of 8 and an
 *              arena base aligned to 16 bytes; anything else takes the 2-byte path, same bits); gain [U] float32
 *   mel_arena  float32 [sum F_u, n_mels], frame-major, mel_off [U + 1] int64 in FRAMES; NULL: audio only (mel_off, mel_out are then ignored)
 *   utt, start_frame  [B] int32 ON THE DEVICE: 0 <= utt[b] < U, start_frame[b] >= 0 — the caller's promise (io_utils/segment_feed.py checks its
 *              host copies); a start beyond an utterance's end gives zeros / mel_pad and reads nothing
 *   y_out [B, 1, frames hop], mel_out [B, n_mels, frames] (channel-major: what Generator takes)
 * Checked here: 1 <= B <= 65535, frames, hop >= 1, frames hop < 2^31, 1 <= n_mels <= 255 with a mel arena, NULL pointers, alignment to the
 * element type.  All arena indexing is 64-bit. */
int ttsc_segment_gather(const int16_t* wav_arena_dev, const int64_t* wav_off_dev, const float* gain_dev, const float* mel_arena_dev,
                        const int64_t* mel_off_dev, const int32_t* utt_dev, const int32_t* start_frame_dev, int32_t B, int32_t n_mels,
                        int32_t frames, int32_t hop, float mel_scale, float mel_pad, float* y_out_dev, float* mel_out_dev, void* stream);

/* Loudness meter and gain stage (csrc/loudness.hip; io_utils/loudness.py; the float64 statement is tests/loudness_reference.py): ITU-R BS.1770-4
 * integrated loudness of mono rows at any rate sr that is a positive multiple of 10 with sr / 10 >= 64, a 4x true peak, one static gain per row.
 *   x [B, Lmax] float32, len [B] int32 (clamped to [0, Lmax]); samples behind a row's length are never read.  1 <= B <= 65535, Lmax < 2^31.
 * ttsc_loudness_measure:
 *   kweight_host  154 float64 ON THE HOST: b0 b1 b2 a1 a2 of the shelf, the same of the high-pass (transposed direct form II, a0 = 1), then nine
 *                 row-major 4x4 matrices A^(64 2^k), k = 0 .. 8, A being one step of the cascade's state at zero input (io_utils/loudness.py)
 *   taps_host     84 float32 ON THE HOST: [4][21], entry [p][d + 10] = fl32(h[4 d + p + 40]) of the 81-tap 4x filter h, 0 where outside
 *   sub [B, nsub_max] float64, nsub_max >= ceil(Lmax / (sr / 10)): sum of squares of the K-weighted row over samples [k sr/10, (k+1) sr/10) and
 *                 [0, len); 0 behind the row.  float64 state and sums in one fixed order: a row has the same bits alone and in any batch
 *   sample_peak, true_peak [B] float32: max |x|, and max |y| of the row oversampled 4x with h (zeros outside the row; the 4x signal is not stored)
 *   workspace     ttsc_loudness_workspace_bytes(B, Lmax, sr) bytes, 8-byte aligned
 * ttsc_loudness_finish (one workgroup per row): blocks z_j = (sub[j] + .. + sub[j+3]) / (4 sr/10) over whole sub-blocks, or ONE block, the mean
 *   square of the whole row, for 0 < len < 4 sr/10; none for len = 0.  Strict gates in the energy domain: z_j > abs_gate, then also
 *   z_j > 0.1 mean(z over the first gate).  zbar [B] float64 = mean z over both gates (0 and silent = 1 when none passes); blocks, gated, silent
 *   [B] int32.  With gain_dev: gain [B] float32 = fl32(min(sqrt(target_energy[b] / zbar), peak_lin[b] / max(sample peak, true peak),
 *   max_gain_lin when > 0)), 1 for a silent row; limited [B] int32 (may be NULL) = 1 where the peak ceiling set the gain.  target_energy and
 *   peak_lin are [B] float64 on the device: 10^((target + 0.691) / 10) and 10^(peak_db / 20).
 * ttsc_loudness_gain: the gain and limited of ttsc_loudness_finish from stored results, for another target.
 * ttsc_loudness_apply: y[b, n] = fl32(gain[b] x[b, n]) for n < len[b], nothing is written behind; y may be x; y [B, Lmax] like x.  16-byte
 *   accesses where a row of x and of y sit alike to a 16-byte boundary, 4-byte accesses otherwise, the same bits.
 * Every argument is checked before the first launch or memset: a refused call leaves its outputs untouched. */
size_t ttsc_loudness_workspace_bytes(int32_t B, int64_t Lmax, int32_t sr);
int ttsc_loudness_measure(const float* x_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int32_t sr, const double* kweight_host,
                          const float* taps_host, double* sub_dev, int64_t nsub_max, float* sample_peak_dev, float* true_peak_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);
int ttsc_loudness_finish(const double* sub_dev, const int32_t* len_dev, int32_t B, int64_t Lmax, int64_t nsub_max, int32_t sr,
                         const float* sample_peak_dev, const float* true_peak_dev, double abs_gate, const double* target_energy_dev,
                         const double* peak_lin_dev, double max_gain_lin, double* zbar_dev, int32_t* blocks_dev, int32_t* gated_dev,
                         int32_t* silent_dev, float* gain_dev, int32_t* limited_dev, void* stream);
int ttsc_loudness_gain(const double* zbar_dev, const float* sample_peak_dev, const float* true_peak_dev, const int32_t* silent_dev,
                       const double* target_energy_dev, const double* peak_lin_dev, double max_gain_lin, int32_t B, float* gain_dev,
                       int32_t* limited_dev, void* stream);
int ttsc_loudness_apply(const float* x_dev, const int32_t* len_dev, const float* gain_dev, int32_t B, int64_t Lmax, float* y_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTSCUBE_HIP_H */
