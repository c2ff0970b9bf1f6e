// The ONE place that decides how an inference convolution is launched: the phase geometry of a layer (conv_phases) and, per launch, the kernel
// family, the tile, and every ConvArgs field and launch dimension that follows from them (conv_plan).  ttsc_conv1d_forward_pitched launches what
// conv_plan returns, ttsc_conv1d_plan reports it; tests/conv_reference.py restates it and tests/test_conv_plan_cpu.py holds the two together.
// Plain C++: no HIP, no environment (the caller hands over a ConvSwitches), no global state.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/ttscube_hip.h"

namespace ttsc {

// One GEMM pass over the taps of a layer; a ConvTranspose1d that cannot run its phases as virtual rows has one per output phase.
struct ConvPhaseGeom {
    int ntaps = 0, tap_base = 0, tap_step = 0;
    int out_stride = 1, out_off = 0;
    int r = 0;  // phase index (transposed); -1 = all phases as virtual rows
    std::vector<int> taps;  // kernel taps (or tap indices when vfused) of this phase, in GEMM order
};

// Conv1d: one phase over all taps.  Transposed: output o = q * stride + r - padding gets the taps k = r (mod stride) — as tap INDICES 0..J-1 of
// one launch when vfused (the packers map (phase, index) -> kernel tap), else one phase per r with taps (a phase without taps is left out: the
// caller refuses kernel_size < stride).
inline std::vector<ConvPhaseGeom> conv_phases(const ttsc_conv1d_cfg& g, bool vfused) {
    std::vector<ConvPhaseGeom> out;
    const int r_end = g.transposed && !vfused ? g.stride : 1;
    for (int r = 0; r < r_end; ++r) {
        ConvPhaseGeom ph;
        if (!g.transposed) {
            for (int k = 0; k < g.kernel_size; ++k) ph.taps.push_back(k);
            ph.tap_base = -g.padding;
            ph.tap_step = g.dilation;
        } else {
            if (vfused)
                for (int j = 0; j < (g.kernel_size + g.stride - 1) / g.stride; ++j) ph.taps.push_back(j);
            else
                for (int k = r; k < g.kernel_size; k += g.stride) ph.taps.push_back(k);
            ph.r = vfused ? -1 : r;
            ph.tap_step = -1;
            ph.out_stride = g.stride;
            ph.out_off = (vfused ? 0 : r) - g.padding;
        }
        ph.ntaps = (int)ph.taps.size();
        if (ph.ntaps) out.push_back(ph);
    }
    return out;
}

// vfused layers whose split-precision rows are interleaved v = co * 4 + r (the last two upsamplers of HiFi-GAN V1)
inline bool conv_vrow4(const ttsc_conv1d_cfg& g, bool vfused, int precision) {
    return vfused && precision == TTSC_PREC_F16X3 && g.stride == 4 && g.kernel_size == 4 && g.padding == 0;
}
// the layers that get a plain-layout weight copy for conv_cout1_kernel
inline bool conv_wants_plain(const ttsc_conv1d_cfg& g) { return !g.transposed && g.out_channels == 1; }

// Every environment switch of the convolution dispatch, as values (read by conv_switches() in conv1d.hip; the defaults are the unset state).
struct ConvSwitches {
    int tile_state = 0;   // TTSC_CONV_TILE: 0 = unset, 1 = parsed into tile_rows x tile_cols, -1 = malformed
    int tile_rows = 0, tile_cols = 0;
    const char* tile_text = "";   // the variable as written, for the error message
    int wide = 1;         // TTSC_CONV_WIDE: 0 = wide and tall kernels off, 2 = also for problems too small to fill the chip (tests)
    bool lean = true;     // TTSC_CONV_LEAN != 0
    bool big_only = false;   // TTSC_F16_TILE == 0: the split kernel's first tile outright
    int acc_init = 1;     // TTSC_CONV_ACC_INIT
    bool tall = true;     // TTSC_CONV_TALL != 0
    long want = 512;      // TTSC_CONV_WANT: workgroups the fp32 fill rule asks of a tile
    int narrow = 1;       // TTSC_CONV_NARROW: the fp32 fill rule's padding test
    int epi_prefetch = 1; // TTSC_CONV_EPI_PREFETCH
    int tall_swizzle = 1; // TTSC_TALL_SWIZZLE
};

// What the planner reads of a layer handle (ttsc_conv1d) ...
struct ConvLayer {
    ttsc_conv1d_cfg cfg;
    int MT, NT, CinP, CoutP, groups, precision;
    bool vfused, vrow4;
    bool has_plain;    // a plain-layout weight exists (or, without weights yet, set_weight would create it)
    float act_scale;
};
// ... and of one launch
struct ConvLaunch {
    int B;
    int64_t Lin, Lout;
    bool gate;
    int out_act;
    float out_scale, in_scale;
};

struct ConvPlan {
    int family = TTSC_CONV_PATH_NONE;   // TTSC_CONV_PATH_*; NONE = this phase has no output position inside [0, Lout)
    int rows = 0, cols = 0;             // tile
    int inst = 0;                       // which instantiation of the family's launcher (ConvTile::inst; tall: 0 = ups.0's, 1 = ups.1's)
    int tap_bucket = 0;                 // F16X3: TMAX of conv_f16x3_kernel
    int q_lo = 0, q_cnt = 0, min_shift = 0, span = 0, span_pad = 0;
    int acc_init = 0, lean = 0, short_from = INT_MAX, epi_prefetch = 0, swz_nx = 0, swz_ny = 0, fold_B = 0;
    unsigned grid[3] = {0, 0, 0};
    size_t lds = 0;                     // dynamic LDS bytes
    char error[256] = {0};              // set when conv_plan returns false
};

// A tile of a general kernel: (rows, cols), its launcher instantiation, and (fp32) the narrower column count narrower_pays compares against.
struct ConvTile {
    int rows, cols, inst, narrow;
};
enum { F16_2x2, F16_2x1, F16_1x4, F16_1x2, F16_1x1 };                                          // launch_f16<MI, NJ>
enum { CFG_2222, CFG_1222, CFG_1122, CFG_2214, CFG_1414, CFG_1214, CFG_1114 };                 // launch_cfg<MI, NJ, WM, WN>
// One table per row class; the fill rule walks it top down, TTSC_CONV_TILE looks a tile up in it.
static constexpr ConvTile F16_TILES_M64[3] = {{64, 256, F16_2x2, 0}, {64, 128, F16_2x1, 0}, {32, 128, F16_1x1, 0}};   // (MT = 128 layers run as two M tiles)
static constexpr ConvTile F16_TILES_M32[3] = {{32, 512, F16_1x4, 0}, {32, 256, F16_1x2, 0}, {32, 128, F16_1x1, 0}};   // (32x128 is legal in both classes)
static constexpr ConvTile FP32_TILES_M128[3] = {{128, 128, CFG_2222, 64}, {64, 128, CFG_1222, 64}, {64, 64, CFG_1122, 0}};
static constexpr ConvTile FP32_TILES_M64[3] = {{64, 256, CFG_2214, 128}, {64, 128, CFG_1222, 64}, {64, 64, CFG_1122, 0}};
static constexpr ConvTile FP32_TILES_M32[3] = {{32, 512, CFG_1414, 256}, {32, 256, CFG_1214, 128}, {32, 128, CFG_1114, 0}};

inline const ConvTile* conv_tiles(int precision, int MT) {
    if (precision == TTSC_PREC_F16X3) return MT >= 64 ? F16_TILES_M64 : F16_TILES_M32;
    return MT == 128 ? FP32_TILES_M128 : (MT == 64 ? FP32_TILES_M64 : FP32_TILES_M32);
}

// dynamic LDS of the wide / tall tile pipeline (F16x3TilePipe::LDS_BYTES): two activation buffers of 4 planes + a dump slot pair, two weight slots
constexpr size_t conv_pipe_lds(int span, int mi) { return (size_t)2 * (4 * span + 2) * 16 + (size_t)2 * (2 * mi * 2 * 64) * 16; }

inline int64_t plan_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t plan_floor_div(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

#define TTSC_PLAN_FAIL(...)                                  \
    do {                                                     \
        snprintf(p.error, sizeof(p.error), __VA_ARGS__);     \
        return false;                                        \
    } while (0)

// false = the launch is refused, p.error says why
inline bool conv_plan(const ConvLayer& c, const ConvPhaseGeom& ph, const ConvLaunch& l, const ConvSwitches& sw, ConvPlan& p) {
    const auto& g = c.cfg;
    const int B = l.B;
    p = ConvPlan();
    if (!g.transposed) {
        p.q_lo = 0;
        p.q_cnt = (int)l.Lout;
    } else {
        // o = q*s + r - p in [0, Lout); vfused: the union over the phases r = 0..s-1 (per-element validity is checked in the epilogue)
        const int r_lo = c.vfused ? g.stride - 1 : ph.r, r_hi = c.vfused ? 0 : ph.r;
        const int64_t qlo = -plan_floor_div(r_lo - g.padding, g.stride);   // ceil((p - r) / s)
        const int64_t qhi = plan_floor_div(l.Lout - 1 - r_hi + g.padding, g.stride) + 1;   // exclusive
        if (qhi <= qlo) return true;
        p.q_lo = (int)qlo;
        p.q_cnt = (int)(qhi - qlo);
    }
    const int last = (ph.ntaps - 1) * ph.tap_step, halo = last < 0 ? -last : last;
    p.min_shift = ph.tap_base + (last < 0 ? last : 0);
    if (sw.tile_state < 0) TTSC_PLAN_FAIL("ttsc_conv1d_forward: TTSC_CONV_TILE must be <rows>x<cols>, e.g. 64x256 (got '%s')", sw.tile_text);
    auto set_grid = [&](int64_t x, int64_t y, int64_t z) { p.grid[0] = (unsigned)x, p.grid[1] = (unsigned)y, p.grid[2] = (unsigned)z; };

    if (!g.transposed && c.groups == 1 && g.out_channels == 1 && g.in_channels <= 64 && g.kernel_size <= 16 && g.dilation == 1 && c.has_plain && !l.gate) {
        // one output channel (conv_post): vector-ALU kernel, bound by the single read of its input
        p.family = TTSC_CONV_PATH_COUT1;
        p.rows = 1, p.cols = 1024;
        p.span = c.NT + halo;
        p.span_pad = p.span + 1;
        set_grid(plan_ceil_div(l.Lout, 1024), B, 1);
        return true;
    }
    const bool f16 = c.precision == TTSC_PREC_F16X3;
    const ConvTile* tiles = conv_tiles(c.precision, c.MT);
    const ConvTile* t = nullptr;
    // span of a tile of n columns: the split kernel stages exactly the window, the fp32 kernel pads its LDS rows by one word
    auto set_cols = [&](int n) {
        p.span = n + halo;
        p.span_pad = f16 ? p.span : p.span + 1;
    };
    auto wgs = [&](const ConvTile& u) { return (long)plan_ceil_div(p.q_cnt, u.cols) * (c.CoutP / u.rows) * B; };

    if (f16) {
        if (ph.ntaps > 16) TTSC_PLAN_FAIL("f16x3 path supports at most 16 taps per phase (got %d)", ph.ntaps);
        set_cols(tiles[0].cols);   // (what the wide and tall launches carry: they do not read it)
        const long want16 = 512;
        const float in_scale = l.in_scale * c.act_scale;   // activation pre-scale (see ttsc_conv1d_set_activation_scale)
        // square "same"-padded layers of the wide stages (the generator's ResBlock convolutions at 128 / 256 channels): the wide-tile kernel
        // (activation window staged once for all output channels)
        const bool wide_shape = !g.transposed && !l.gate && g.in_channels == g.out_channels && (g.out_channels == 128 || g.out_channels == 256) &&
                                ((g.kernel_size == 3 || g.kernel_size == 7 || g.kernel_size == 11)
#ifdef TTSC_PROBE_EVENK
                                 || ((g.kernel_size == 4 || g.kernel_size == 6) && g.dilation == 1)
#endif
                                 ) &&
                                (g.dilation == 1 || g.dilation == 3 || g.dilation == 5) && g.padding == g.dilation * (g.kernel_size - 1) / 2;
        // these layers start their sums at (residual + running sum + bias) / w_unscale in BOTH kernels that may run them (same bits whichever
        // the fill rule picks); TTSC_CONV_ACC_INIT=0 puts the operands back into the epilogue (measurement switch)
        p.acc_init = (sw.acc_init && sw.wide && wide_shape && l.out_act == TTSC_ACT_NONE && l.out_scale == 1.f && c.CoutP == g.out_channels &&
                      (size_t)B * g.out_channels * l.Lout < (1ull << 32)) ? 1 : 0;
        // the first upsamplers of the V1 generator: tall tiles (256 virtual rows x 128 input positions, or 128 x 256)
        const bool tall0 = g.in_channels == 512 && ph.ntaps == 4 && c.CoutP % 256 == 0;    // ups.0: 256-row tiles
        const bool tall1 = g.in_channels == 256 && ph.ntaps == 6 && c.CoutP % 128 == 0;    // ups.1: 128-row tiles
        const bool tall_shape = sw.tall && c.vfused && !c.vrow4 && !l.gate && c.CinP == g.in_channels && (tall0 || tall1);
        const int tall_rows = tall0 ? 256 : 128, tall_cols = tall0 ? 128 : 256;
        // lean staging and zero-tap skipping of the wide and tall kernels (see LEAN_OOB).  The buffer path needs 32-bit byte offsets into one
        // utterance's input with room for the out-of-range marker, and an in_scale for which 0 * in_scale is +0.
        p.lean = (sw.lean && (int64_t)g.in_channels * l.Lin * 4 < (1ll << 31) && in_scale > 0.f && std::isfinite(in_scale)) ? 1 : 0;
        // tall kernel: a row tile that is exactly one phase r lacks the last tap when r + (J - 1) * stride >= kernel_size; a tile that spans
        // phases keeps all J taps
        if (tall_shape && tall_rows == g.out_channels) p.short_from = g.kernel_size - (ph.ntaps - 1) * g.stride;
        if (tall_shape && (sw.wide == 2 || (long)plan_ceil_div(p.q_cnt, tall_cols) * (c.CoutP / tall_rows) * B >= want16)) {
            p.family = TTSC_CONV_PATH_TALL;
            p.rows = tall_rows, p.cols = tall_cols, p.inst = tall0 ? 0 : 1;
            set_grid(plan_ceil_div(p.q_cnt, tall_cols), c.CoutP / tall_rows, B);
            if (sw.tall_swizzle && p.grid[1] > 1) {   // XCD-aware 1-D launch (see the kernel): the row tiles of a q tile on one XCD, back to back
                p.swz_nx = (int)p.grid[0];
                p.swz_ny = (int)p.grid[1];
                p.fold_B = B;
                set_grid(plan_ceil_div((int64_t)p.swz_nx * B, 8) * 8 * p.swz_ny, 1, 1);
            }
            p.lds = conv_pipe_lds(tall_cols + ph.ntaps - 1, tall_rows / 64);
            return true;
        }
        if (sw.wide && wide_shape && (sw.wide == 2 || (long)plan_ceil_div(l.Lout, 256) * (g.out_channels / 128) * B >= want16)) {
            p.family = TTSC_CONV_PATH_WIDE;
            p.rows = 128, p.cols = 256;
            // deep-prefetched epilogue operands (bit-identical to the plain epilogue; TTSC_CONV_EPI_PREFETCH=0 restores the four-rows-at-a-time one)
            p.epi_prefetch = (sw.epi_prefetch && l.out_act == TTSC_ACT_NONE && (size_t)B * g.out_channels * l.Lout < (1ull << 32)) ? 1 : 0;   // (32-bit element offsets)
            set_grid(plan_ceil_div(l.Lout, 256), g.out_channels / 128, B);
            p.lds = conv_pipe_lds(256 + halo, 2);
            return true;
        }
        p.family = TTSC_CONV_PATH_F16X3;
        p.tap_bucket = ph.ntaps <= 3 ? 3 : (ph.ntaps <= 7 ? 7 : (ph.ntaps <= 11 ? 11 : 16));
    } else {
        p.family = TTSC_CONV_PATH_FP32;
    }

    if (sw.tile_state > 0) {
        // forced tile: one of the three the fill rule below could pick for this MT class, through the same span bookkeeping
        for (int i = 0; i < 3 && !t; ++i)
            if (tiles[i].rows == sw.tile_rows && tiles[i].cols == sw.tile_cols) t = &tiles[i];
        if (!t)
            TTSC_PLAN_FAIL("ttsc_conv1d_forward: TTSC_CONV_TILE=%dx%d is not %s tile of this layer (MT %d: %dx%d, %dx%d, %dx%d)", sw.tile_rows, sw.tile_cols,
                           f16 ? "a split-kernel" : "an fp32", c.MT, tiles[0].rows, tiles[0].cols, tiles[1].rows, tiles[1].cols, tiles[2].rows, tiles[2].cols);
    } else {
        // tile by machine fill: the largest tile that still gives >= 2 workgroups per CU (a single short utterance — the reference API's B=1
        // case —, training crops and the deep discriminator layers are small problems: the big tiles would leave most of the 256 CUs idle) ...
        // fp32: and, among the tiles that fill the machine, not one that is mostly padding: the deep layers of the discriminators see sequences
        // of 50-200 positions (a 128-column tile over 149 positions computes 256), so a narrower tile is taken whenever it cuts the padded
        // columns by more than an eighth (this kernel is bound by its MFMA count, not by operand reuse)
        auto padded = [&](int nt) { return (long)plan_ceil_div(p.q_cnt, nt) * nt; };
        auto narrower_pays = [&](const ConvTile& u) { return sw.narrow && padded(u.narrow) * 8 < padded(u.cols) * 7; };
        auto takes = [&](int i) {
            if (f16) return (i == 0 && sw.big_only) || wgs(tiles[i]) >= 512;
            return wgs(tiles[i]) >= sw.want && !narrower_pays(tiles[i]);
        };
        t = takes(0) ? &tiles[0] : (takes(1) ? &tiles[1] : &tiles[2]);   // (the third row is taken without testing its workgroup count)
    }
    p.rows = t->rows, p.cols = t->cols, p.inst = t->inst;
    set_cols(t->cols);
    set_grid(plan_ceil_div(p.q_cnt, t->cols), c.CoutP / t->rows, B);
    if (f16) {
        p.lds = (size_t)p.span_pad * 4 * 16 + (size_t)ph.ntaps * (t->rows / 32) * 2 * 64 * 16;
    } else {
        p.lds = (size_t)2 * 16 * p.span_pad * sizeof(float);   // 2 buffers x KC channels
        if (p.lds > 160 * 1024) TTSC_PLAN_FAIL("conv_mfma_kernel: receptive field too large for LDS (%zu bytes)", p.lds);
    }
    return true;
}
#undef TTSC_PLAN_FAIL

}  // namespace ttsc
