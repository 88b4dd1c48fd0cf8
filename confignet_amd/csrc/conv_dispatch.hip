// conv_dispatch.hip -- which launch a convolution gets (host code only).
//
// Every fp32 forward / data-gradient convolution is served in two steps: plan_conv_fwd decides the launch from the geometry and
// the request alone (route, tile, K split, profile family, grid -- no HIP call, no pointer), run_conv_fwd performs it (one switch
// over the route, one profile bracket, one launch check, the split-K protocol).  cn_conv_fwd_plan reports the plan without a
// device (cn_conv_fwd_plan_ep: the same for a request with the mask epilogue of cn_conv_dgrad_w_mask).  The kernels live in
// small_conv.hip (thin and image-side layers), fwd2.hip (the LDS-DMA loop) and igemm_conv.hip (the register-staged implicit-GEMM
// loop).  The filter gradient is served the same way by plan_conv_wgrad / run_conv_wgrad / cn_conv_wgrad_plan in the second half
// of this file; the tuning hooks are at its end.
#include "common.h"

#include <algorithm>
#include <vector>

#include "mma_tile.h"
#include "conv_geom.h"

namespace {

int g_tune_cfg = -1;                 // cn_conv_tune (sweeps, tests): forced tile / split-K factor / filter-gradient workgroup target
int g_tune_splits = 0;
long g_tune_wg_blocks = 0;
int g_tune_wg2_ns = 0;               // cn_conv_loop_select(ns): stage count of the LDS-DMA filter-gradient kernel (0 = default)
int g_fwd2_sel = -1;                 // cn_conv_loop_select override: 0 = keep the LDS-DMA loop (fwd2.hip) off
constexpr int g_fwd2_min_nks = 1;    // the LDS-DMA loop takes reductions of MORE K steps than this
constexpr int g_fwd2_min_c = 48;     // thinnest layer it takes

// What the caller asks for, as far as the choice of the launch depends on it.  bt = 1: w is the original filter of the convolution
// whose data gradient the geometry describes (see igemm_fwd_kernel); stats_mode: cn_conv_fwd_stats; x_dt / y_dt: storage types of
// input and output (anything but fp32 on both sides: cn_conv_fwd_dt); has_mask: the consumer's ReLU backward (and its column sums) in
// the launch's epilogue (cn_conv_dgrad_w_mask).
struct ConvReq {
    int bt, has_bias, act, has_res, stats_mode, x_dt, y_dt, has_mask = 0;
};

// The operands of the mask epilogue: the saved activation (shaped like the output) and the destinations of the column sums.
struct ConvEp {
    const float* mask = nullptr;
    float* colsum = nullptr;
    float* colsum2 = nullptr;
};

struct ConvPlan {
    int route = CN_ROUTE_UNSUPPORTED;
    int ret = CN_EUNSUPPORTED;       // what the request gets when nothing is launched (route == CN_ROUTE_UNSUPPORTED)
    int cfg = -1;                    // tile of the implicit-GEMM numbering (FWD2 / IGEMM)
    int splits = 1, par = 0;
    bool vec = false;
    bool plain = false;              // FWD2: a plain 1x1 product, no gather
    int family = -1;                 // CN_FAM_* of the profile bracket; -1: the launch has none
    int srows = 1, sper = 1;         // statistics: rows of one sample / of one parity class
    int grid[3] = {0, 0, 0};
};

// The image-side layers: 3x3 / 7x7 convolutions OF the 3-channel fp32 image (output fp32 or bf16) and the data gradients of the 3x3
// ones INTO it (output gradient fp32 or, stride 2 only, bf16).  CN_ROUTE_UNSUPPORTED: none of them.
int image_route(const CnConvGeom& g, const ConvReq& q) {
    const bool x32 = q.x_dt == CN_F32, y32 = q.y_dt == CN_F32, x16 = q.x_dt == CN_BF16, y16 = q.y_dt == CN_BF16;
    if (x32 && (y32 || y16) && !q.bt && g.nd == 2 && g.cin == 3 && g.dl_h == 1 && g.dl_w == 1 && !g.up && g.cout > 4 && g.cout <= 64) {
        if (g.k_h == 3 && g.k_w == 3 && g.s_h == g.s_w && (g.s_h == 1 || g.s_h == 2)) return CN_ROUTE_C3;
        if (g.k_h == 7 && g.k_w == 7 && g.s_h == 2 && g.s_w == 2 && !q.has_res) return CN_ROUTE_C7S2;
    }
    if (y32 && g.nd == 2 && g.k_h == 3 && g.k_w == 3 && g.s_h == 1 && g.s_w == 1 && !g.up && g.cout == 3 && !q.has_bias &&
        q.act == CN_ACT_NONE && g.p_h >= 0 && g.p_h <= 2 && g.p_w >= 0 && g.p_w <= 2) {
        if ((x32 || x16) && g.dl_h == 2 && g.dl_w == 2 && g.cin == 48 && g.out_h <= 2 * g.in_h && g.out_w <= 2 * g.in_w) return CN_ROUTE_S2_IMAGE_DGRAD;
        if (x32 && g.dl_h == 1 && g.dl_w == 1 && g.cin == 64) return CN_ROUTE_S1_IMAGE_DGRAD;
    }
    return CN_ROUTE_UNSUPPORTED;
}

// Pure: reads the geometry, the request, cn_det(), cn_cu_count() and the tuning overrides.
ConvPlan plan_conv_fwd(const CnConvGeom& g, const ConvReq& q) {
    ConvPlan p;
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    // a mask request is a residual request to the plan (only an unsplit launch carries either; a split is priced against the pass
    // that then follows it) that, like the statistics, only the LDS-DMA loop serves
    const bool mask = q.has_mask != 0;
    const bool res = q.has_res != 0 || mask, stats = q.stats_mode != 0;
    const int bt = q.bt;
    auto small = [&p](int route, int family, long grid_x) {      // a single launch of a small_conv.hip / thin kernel
        p.route = route;
        p.ret = CN_OK;
        p.family = family;
        p.grid[0] = (int)grid_x; p.grid[1] = p.grid[2] = 1;
        return p;
    };
    auto refuse = [&p](int code) {                               // nothing is launched
        p.ret = code;
        return p;
    };
    const int img = image_route(g, q);
    const long img_grid = img == CN_ROUTE_S2_IMAGE_DGRAD ? (long)g.n * cn_cdiv(g.in_h, 8) * cn_cdiv(g.in_w, 32)
                                                         : (long)g.n * cn_cdiv(g.out_h, 8) * cn_cdiv(g.out_w, 32);
    const int img_family = img == CN_ROUTE_C3 || img == CN_ROUTE_C7S2 ? CN_FAM_C3_FWD : CN_FAM_S2_IMAGE_DGRAD;
    if (q.x_dt != CN_F32 || q.y_dt != CN_F32)        // mixed storage types: the image-side kernels or nothing
        return img != CN_ROUTE_UNSUPPORTED && !mask ? small(img, img_family, img_grid) : p;
    // res: only the unsplit implicit-GEMM launches carry the residual add in their epilogue -- anything else answers
    // CN_EUNSUPPORTED before launching (the caller then adds it with a pass of its own)
    if ((res || stats) && (g.cout <= 4 || g.cin == 3 || g.cout % 4 != 0)) return p;
    // stats: the launch must be one that can carry the statistics in its epilogue -- the unsplit LDS-DMA loop with tiles inside one
    // sample -- or nothing is launched
    if (stats && (bt || cn_det() || g.cin % BK != 0)) return p;
    // bt: only the vectorised implicit-GEMM path takes the original filter
    if (bt && (g.cout <= 4 || g.cin % BK != 0 || g.cout % 4 != 0)) return p;
    if (g.cout <= 4) {
        p.vec = g.cin % 4 == 0;
        p.par = parity_ordered(g);
        const size_t lds = sizeof(float) * 4 * (size_t)g.k_d * g.k_h * g.k_w * g.cin;
        if (lds > 64 * 1024) {
            cn_set_error("thin conv: filter of %zu bytes does not fit the LDS stage", lds);
            return refuse(CN_EINVAL);
        }
        const int T = g.k_d * g.k_h * g.k_w, CL = g.cin / 4;
        const bool dl1 = g.dl_d * g.dl_h * g.dl_w == 1;
        if (g.nd == 2 && g.up == 1 && g.k_h == 4 && g.k_w == 4 && g.s_h == 1 && g.s_w == 1 && g.dl_h == 1 && g.dl_w == 1 &&
            g.cout == 3 && g.cin == 32 && g.p_h == 1 && g.p_w == 1 && g.out_h <= 2 * g.in_h && g.out_w <= 2 * g.in_w)
            return small(CN_ROUTE_UP2K4_RGB, CN_FAM_THIN, (long)g.n * cn_cdiv(g.in_h, 8) * cn_cdiv(g.in_w, 16));
        if (img != CN_ROUTE_UNSUPPORTED) return small(img, img_family, img_grid);          // (the two data gradients into the image)
        if (p.par && g.cin % BK == 0 && q.act == CN_ACT_NONE && T <= CN_MAX_MASKED_TAPS) return small(CN_ROUTE_THIN_PAR_IGEMM, CN_FAM_FWD_128x32, cn_cdiv(M, 128));
        if (p.vec && g.cout == 3 && CL >= 5 && CL <= 16 && T <= 32 && (p.par || dl1) && g.dl_d * g.dl_h * g.dl_w <= 8)
            return small(CN_ROUTE_THIN_COOP, -1, cn_cdiv(M, (256 / (CL <= 8 ? 8 : 16)) * CN_THIN_COOP_PX));
        return small(CN_ROUTE_THIN, -1, cn_cdiv(M, 256));
    }
    if (img != CN_ROUTE_UNSUPPORTED) return small(img, img_family, img_grid);              // (the two first layers)
    if (g.cout % 4 != 0) {
        cn_set_error("cout=%d: implicit-GEMM path needs cout %% 4 == 0", g.cout);
        return refuse(CN_EINVAL);
    }
    const bool vec = g.cin % BK == 0;
    // the vectorised gathers (igemm_fwd_kernel, fwd2.hip) walk the taps of a tile through one 64-bit mask: a longer filter would lose
    // its taps past the 64th without a word (the scalar gather, cin % 16 != 0, counts K elements and has no such limit)
    if (vec && (long)g.k_d * g.k_h * g.k_w > CN_MAX_MASKED_TAPS) {
        cn_set_error("%d taps: the vectorised implicit-GEMM gather takes at most %d", g.k_d * g.k_h * g.k_w, CN_MAX_MASKED_TAPS);
        return refuse(CN_EUNSUPPORTED);
    }
    const int par = parity_ordered(g) && vec;
    // tile choice: the biggest tile that still gives >= 2 workgroups per CU (256 CUs)
    const long t128 = (long)cn_cdiv(M, 128) * cn_cdiv(g.cout, 128);
    const long t128x64 = (long)cn_cdiv(M, 128) * cn_cdiv(g.cout, 64);
    int cfg;
    long tiles;
    if (g.cout <= 32) { cfg = 3; tiles = (long)cn_cdiv(M, 128) * cn_cdiv(g.cout, 32); }
    else if (g.cout > 64 && t128 >= 512) { cfg = 0; tiles = t128; }
    else if (t128x64 >= 512) { cfg = 1; tiles = t128x64; }
    else { cfg = 2; tiles = (long)cn_cdiv(M, 64) * cn_cdiv(g.cout, 64); }
    // cout = 96 / 192 (discriminator blocks 1-2 and the data gradients of blocks 2-3): a 128 x 96 tile wastes nothing
    // where 128- or 64-wide tiles pad a quarter of their columns
    if (g.cout % 96 == 0 && g.cout % 128 != 0 &&
        (long)cn_cdiv(M, 128) * (g.cout / 96) >= (g.cout == 96 ? 256 : 384)) {
        cfg = 4;
        tiles = (long)cn_cdiv(M, 128) * (g.cout / 96);
    }
    // split-K for small outputs with a long reduction (ResNet stage 4/5, Conv3D at 4^3->8^3)
    int splits = 1;
    // (parity-ordered data gradients: tiles of the 4-tap class carry 4x the K of the 1-tap class, so more, smaller
    // K slices also even out the load -- conv_tune.py dgrad: 123 -> 95 us at M=16384 N=192, 124 -> 104 us at M=4096 N=384)
    const bool par_small = par && cfg == 2;          // 64 x 64 tiles of a parity-ordered data gradient
    const long nks_total = vec ? (long)g.k_d * g.k_h * g.k_w * (g.cin / BK) : 0;
    // a short reduction (<= 8 steps) is all prologue and epilogue: the narrower tile spreads the stores over twice the workgroups
    if (cfg == 0 && vec && !par && nks_total <= 8) { cfg = 1; tiles = t128x64; }
    // one workgroup per CU and a short reduction: the zero pass, the atomics and the separate bias / activation pass of a K
    // split cost more than the idle SIMD slots they would fill (conv_tune.py: M=8192 K=512 N=128 31 -> 25 us unsplit)
    const bool short_full = !par && tiles >= 256 && nks_total < 64;
    if (vec && tiles < (par_small ? 1024 : 512) && !short_full) {
        long nks = nks_total;
        if (par) nks /= (long)g.dl_d * g.dl_h * g.dl_w;
        long want = ((par_small ? 3072 : 1024) + tiles - 1) / tiles;      // aim at ~4 (12) workgroups per CU
        if (want > 16) want = 16;
        const long min_steps = par_small ? 8 : 16;   // average K steps per workgroup
        if (want > nks / min_steps) want = nks / min_steps;
        if (want > 1) splits = (int)want;
    }
    // The LDS-DMA main loop (fwd2.hip) keeps the matrix pipe fed from ONE workgroup per CU (its loads run NS steps ahead of the
    // MFMAs and none of its instructions sits outside an MFMA's shadow), so it does not need the 4 workgroups per CU the
    // register-staged loops are split for -- and every K split it avoids saves the zero pass, a tile of atomics per workgroup and
    // the separate bias / activation pass (13 us of a 60 us launch at M = 4096, K = 2304, N = 256; scripts/dev/fwd2_sweep.py).
    // (32 output channels: the 128 x 32 tile of the same loop, input channels from 32 up)
    const bool n32 = g.cout == 32 && g.cin >= 32;
    const bool fwd2_takes = g_fwd2_sel != 0 && vec && nks_total > g_fwd2_min_nks && ((g.cin >= g_fwd2_min_c && g.cout >= g_fwd2_min_c) || n32) &&
                            g.dl_d <= 2 && g.dl_h <= 2 && g.dl_w <= 2 && (double)g.n * g.in_d * g.in_h * g.in_w * g.cin < 5.3e8 &&
                            (double)g.k_d * g.k_h * g.k_w * g.cin * g.cout < 5.3e8;
    if (fwd2_takes) {
        const int T = g.k_d * g.k_h * g.k_w;
        // a parity-ordered 1x1 data gradient (ResNet's strided projections) has ONE live class: only M / (dl_d dl_h dl_w) of
        // its rows do any work, the tiles of the other classes store zeros and leave
        const long Me = (par && T == 1) ? M / ((long)g.dl_d * g.dl_h * g.dl_w) : M;
        long nks = nks_total;
        if (par) nks /= (long)g.dl_d * g.dl_h * g.dl_w;
        splits = 1;
        // parity classes with the same number of live taps (k % dl == 0 on every axis: the upsample-folded layers' class filters)
        // are one balanced launch; the data gradients of the stride-2 3x3 layers mix classes of 1 / 2 / 2 / 4 taps
        const bool par_balanced = par && g.k_d % g.dl_d == 0 && g.k_h % g.dl_h == 0 && g.k_w % g.dl_w == 0;
        if (n32) {
            cfg = 3;
            tiles = cn_cdiv(M, 128);
        } else if (par && T > 1 && !par_balanced) {
            // classes of 1 / 2 / 2 / 4 live taps (a quarter of the rows each): the 64 x 64 tile (128 x 96 for cout = 96 once it fills
            // the chip twice), K slices only for the 64 x 64 tile, where they also even out the load between the classes
            cfg = 2;
            tiles = (long)cn_cdiv(M, 64) * cn_cdiv(g.cout, 64);
            if (g.cout % 96 == 0 && g.cout % 64 != 0 && (long)cn_cdiv(M, 128) * (g.cout / 96) >= 512) {
                cfg = 4;
                tiles = (long)cn_cdiv(M, 128) * (g.cout / 96);
            }
            if (cfg == 2 && tiles < 1024) {
                long want = (1536 + tiles / 2) / tiles;
                if (want > 16) want = 16;
                if (want > nks / 8) want = nks / 8;
                if (want > 1) splits = (int)want;
            }
        } else {
            // Tile and K split together from a cost model of the launch (microseconds): the workgroups of one CU share its matrix
            // pipes, so a launch of W workgroups takes ceil(W / 256) workgroup lifetimes of (K steps) x (MFMA time of a step +
            // what the tile leaves exposed: measured per tile, scripts/dev/fwd2_sweep.py), plus a fixed start / drain, plus --
            // with a K split -- the zero pass, the separate bias / activation pass and one tile of atomics per workgroup.  What
            // the thresholds of the register-staged loops could not see is the quantisation: 384 workgroups on 256 CUs take as
            // long as 512.
            // The 64 x 64 tile wins the tile sweep almost everywhere with this loop (16 accumulator registers and 32 KB of LDS: five
            // workgroups per CU, so their barriers and fills interleave, and 4x finer load balance than a 128 x 128 tile); the one
            // exception is cout = 96, where 64-wide tiles pad a quarter of their columns and the 128 x 96 tile pads nothing.
            struct Cand { int cfg, bm, bn; double step_us; };
            const Cand cands[2] = {{2, 64, 64, 0.265}, {4, 128, 96, 0.68}};
            double best = 0.0;
            bool have = false;
            for (const Cand& c : cands) {
                if (c.cfg == 4 && (g.cout % 96 != 0 || g.cout % 64 == 0 || (long)cn_cdiv(Me, 128) * (g.cout / 96) < 256)) continue;
                const long tl = (long)cn_cdiv(Me, c.bm) * cn_cdiv(g.cout, c.bn);
                const long smax = nks / 8 > 1 ? (nks / 8 > 16 ? 16 : nks / 8) : 1;
                for (long s_ = 1; s_ <= smax; ++s_) {
                    const double waves = (double)cn_cdiv(tl * s_, cn_cu_count());
                    double t = 10.0 + waves * (double)cn_cdiv(nks, s_) * c.step_us * (waves == 1.0 ? 1.06 : 1.0);
                    if (s_ > 1) t += 9.0 + (double)s_ * (double)M * g.cout * 4.0 / 6.0e6;
                    // a split launch cannot carry the residual add / the statistics in its epilogue: the caller then runs a pass of
                    // its own over y (read + write at ~3 TB/s, one more launch) -- priced here so that a fused request splits only
                    // where the split still wins with that pass added
                    if (s_ > 1 && (res || stats)) t += 5.0 + 2.0 * (double)M * g.cout * 4.0 / 3.0e6;
                    if (!have || t < best) { have = true; best = t; cfg = c.cfg; tiles = tl; splits = (int)s_; }
                }
            }
        }
    }
    if (g_tune_cfg >= 0) cfg = g_tune_cfg;                        // tuning overrides (cn_conv_tune; scripts/conv_sweep.py)
    if (g_tune_splits > 0) splits = g_tune_splits;
    if (res && splits > 1) return p;
    if (stats) {
        // rows of one sample (inside one parity class for class-major rows); every tile must lie inside one sample
        const int qd = par ? g.out_d / g.dl_d : g.out_d, qh = par ? g.out_h / g.dl_h : g.out_h, qw = par ? g.out_w / g.dl_w : g.out_w;
        p.srows = qd * qh * qw;
        p.sper = par ? g.n * p.srows : (int)M;
        if (!fwd2_takes || splits > 1 || cfg == 3 || p.srows % (cfg == 2 ? 64 : 128) != 0) return p;
    }
    if (cn_det() && splits > 1) {
        // deterministic mode: the K splits write partial outputs into the stream's workspace (as many splits as it holds) and a
        // second launch adds them in split order -- no atomics
        const long cap = (long)(CN_DET_WS_FLOATS / ((size_t)M * g.cout));
        if (splits > cap) splits = (int)cap;
        if (splits <= 1 || !vec) splits = 1;
    }
    // the LDS-DMA main loop; everything it does not take (K or cout no multiple of 16 / 4, thin layers, > 2 GiB operands, a forced
    // 128 x 32 tile on more than 32 channels): igemm_fwd_kernel
    p.route = fwd2_takes && (cfg != 3 || n32) && cfg >= 0 && cfg <= 4 ? CN_ROUTE_FWD2 : CN_ROUTE_IGEMM;
    if (stats && p.route != CN_ROUTE_FWD2) return refuse(CN_EINVAL);      // (a forced tile nobody has: never a kernel without the statistics)
    if (mask && p.route != CN_ROUTE_FWD2) {          // igemm_fwd_kernel has no mask epilogue: nothing is launched
        p.route = CN_ROUTE_UNSUPPORTED;
        return p;
    }
    p.ret = CN_OK;
    p.cfg = cfg;
    p.splits = splits;
    p.par = par;
    p.vec = vec;
    p.family = cfg == 0 ? CN_FAM_FWD_128x128 : cfg == 1 ? CN_FAM_FWD_128x64 : cfg == 3 ? CN_FAM_FWD_128x32 : cfg == 4 ? CN_FAM_FWD_128x96 : CN_FAM_FWD_64x64;
    if (p.route == CN_ROUTE_FWD2) {
        p.plain = !par && g.k_d * g.k_h * g.k_w == 1 && g.s_d == 1 && g.s_h == 1 && g.s_w == 1 && g.dl_d == 1 && g.dl_h == 1 &&
                  g.dl_w == 1 && !g.up && g.p_d == 0 && g.p_h == 0 && g.p_w == 0 && g.out_d == g.in_d && g.out_h == g.in_h &&
                  g.out_w == g.in_w;
        cn_fwd2_grid(cfg, M, g.cout, par, splits, p.grid);
    } else {
        cn_igemm_fwd_grid(cfg, g, vec, par, splits, p.grid);
    }
    return p;
}

// Performs the plan: the split-K protocol (zero pass or, in deterministic mode, partial slabs + cn_sum_parts; the bias / activation
// pass behind a split) around ONE launch.  A plan without a launch returns its code before anything is enqueued.
int run_conv_fwd(const ConvPlan& p, const CnConvGeom& g, const ConvReq& q, const void* x, const float* w, const float* bias,
                 const float* res, void* y, float slope, float* stats, float stats_slope, hipStream_t s, const ConvEp& ep = ConvEp{}) {
    if (p.route == CN_ROUTE_UNSUPPORTED) return p.ret;
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    const int splits = p.splits;
    float* parts = nullptr;
    if (cn_det() && splits > 1) {
        parts = cn_det_ws(s, (size_t)splits * M * g.cout);
        if (!parts) return CN_EINVAL;
    }
    const int kact = splits > 1 ? CN_ACT_NONE : q.act;
    if (splits > 1 && !parts) {
        if (int ez__ = cn_zero_async(y, sizeof(float) * M * g.cout, s)) return ez__;
    }
    const long part_stride = parts ? (long)M * g.cout : 0;
    float* const out = parts ? parts : (float*)y;
    const double ep_bytes = ep.mask ? 4.0 * (double)M * g.cout : 0.0;      // (the mask is read once, like the output is written)
    if (p.family >= 0)
        cn_prof_begin(s, conv_flops(g), conv_bytes(g, q.x_dt == CN_BF16 ? 2.0 : 4.0, q.y_dt == CN_BF16 ? 2.0 : 4.0) + ep_bytes, p.family);
    int e = CN_OK;
    switch (p.route) {
        case CN_ROUTE_FWD2: {
            const double xe = (double)g.n * g.in_d * g.in_h * g.in_w * g.cin, we = (double)g.k_d * g.k_h * g.k_w * g.cin * g.cout;
            e = cn_fwd2(p.plain ? nullptr : &g, p.cfg, q.bt, (const float*)x, w, bias, out, M, g.cout, g.cin, kact, slope, splits, part_stride,
                        p.plain ? 0 : p.par, s, res, xe, we, stats, q.stats_mode, stats_slope, p.srows, p.sper, ep.mask, ep.colsum, ep.colsum2);
            break;
        }
        case CN_ROUTE_IGEMM:
            e = cn_igemm_fwd(p.cfg, g, p.vec, p.par, splits, (const float*)x, w, bias, out, kact, slope, s, q.bt, part_stride, res);
            break;
        case CN_ROUTE_THIN_PAR_IGEMM:
            e = cn_igemm_fwd_thin(g, (const float*)x, w, bias, out, kact, slope, s);
            break;
        default:
            cn_small_conv(p.route, (unsigned)p.grid[0], g, p.vec, p.par, x, q.x_dt, w, bias, y, q.y_dt, kact, slope, s);
            break;
    }
    if (p.family >= 0) cn_prof_end(s);
    CN_CHECK_ARG(e != CN_EUNSUPPORTED, "convolution plan (route %d, tile %d) refused by its kernel", p.route, p.cfg);      // (a bug: never "nothing launched")
    if (e != CN_OK) return e;
    CN_LAUNCH_CHECK();
    if (parts) e = cn_sum_parts(parts, (float*)y, splits, (long)M * g.cout, 0, 1.f, s);
    if (e == CN_OK && splits > 1 && q.act != CN_ACT_NONE) e = cn_act_fwd(y, y, (size_t)M * g.cout, q.act, slope, CN_F32, s);
    return e;
}

// argument checks, plan, run: the body of every forward / data-gradient entry below
int conv_fwd(const CnConvGeom* gp, const ConvReq& q, const void* x, const float* w, const float* bias, const float* res, void* y,
             float slope, float* stats, float stats_slope, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(x && w && y, "NULL tensor");
    return run_conv_fwd(plan_conv_fwd(*gp, q), *gp, q, x, w, bias, res, y, slope, stats, stats_slope, (hipStream_t)stream);
}

}  // namespace

extern "C" int cn_conv_fwd(const CnConvGeom* gp, const float* x, const float* w, const float* bias, float* y, int act,
                           float slope, void* stream) {
    return conv_fwd(gp, ConvReq{0, bias != nullptr, act, 0, 0, CN_F32, CN_F32}, x, w, bias, nullptr, y, slope, nullptr, 0.f, stream);
}

extern "C" int cn_conv_fwd_stats(const CnConvGeom* gp, const float* x, const float* w, const float* bias, float* y, int act,
                                 float slope, float* stats, int stats_mode, float stats_slope, void* stream) {
    CN_CHECK_ARG(stats && (stats_mode == 1 || stats_mode == 2), "cn_conv_fwd_stats: stats buffer and mode 1 / 2");
    CN_CHECK_ARG(stats_mode == 1 || act == CN_ACT_NONE, "cn_conv_fwd_stats: mode 2 takes the statistics of the pre-activation output");
    return conv_fwd(gp, ConvReq{0, bias != nullptr, act, 0, stats_mode, CN_F32, CN_F32}, x, w, bias, nullptr, y, slope, stats, stats_slope, stream);
}

// y = act(conv(x, w) + bias + res): the residual add of a ResNet block in the convolution's epilogue (real_encoder.py:13 --
// keras ResNet50's `Add` + `Activation("relu")` behind the block's last 1x1 convolution).  Only unsplit implicit-GEMM launches
// carry it; CN_EUNSUPPORTED (nothing launched) otherwise.
extern "C" int cn_conv_fwd_res(const CnConvGeom* gp, const float* x, const float* w, const float* bias, const float* res, float* y,
                               int act, float slope, void* stream) {
    CN_CHECK_ARG(res, "cn_conv_fwd_res: res is NULL");
    return conv_fwd(gp, ConvReq{0, bias != nullptr, act, 1, 0, CN_F32, CN_F32}, x, w, bias, res, y, slope, nullptr, 0.f, stream);
}

// First / last layers with mixed storage types (the bf16 path keeps 3-channel images in fp32, everything wider in bf16):
//   * 3x3 / 7x7 convolution of a 3-channel fp32 image written in bf16 (c3_fwd_kernel, c7s2_fwd_kernel), and
//   * the data gradient of the stride-2 3x3 one INTO the fp32 image from a bf16 output gradient (s2_image_dgrad_kernel, the
//     geometry cn_conv_dgrad_dt builds),
// without a conversion pass over the 48 / 64-channel tensor.  Everything else: CN_EUNSUPPORTED, nothing launched.
extern "C" int cn_conv_fwd_dt(const CnConvGeom* gp, const void* x, int x_dt, const float* w, const float* bias, void* y, int y_dt,
                              int act, float slope, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(x && w && y, "NULL tensor");
    if (x_dt == CN_F32 && y_dt == CN_F32) return CN_EUNSUPPORTED;      // (cn_conv_fwd's case)
    const ConvReq q{0, bias != nullptr, act, 0, 0, x_dt, y_dt};
    return run_conv_fwd(plan_conv_fwd(*gp, q), *gp, q, x, w, bias, nullptr, y, slope, nullptr, 0.f, (hipStream_t)stream);
}

extern "C" int cn_conv_dgrad(const CnConvGeom* gp, const float* gy, const float* w_tflip, float* gu, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(gp->dl_d == 1 && gp->dl_h == 1 && gp->dl_w == 1, "dgrad of a dilated-input geometry is not defined here");
    const CnConvGeom d = dgrad_geom(*gp);
    return cn_conv_fwd(&d, gy, w_tflip, nullptr, gu, CN_ACT_NONE, 0.f, stream);
}

extern "C" int cn_conv_dgrad_dt(const CnConvGeom* gp, const void* gy, int gy_dt, const float* w_tflip, void* gu, int gu_dt,
                                void* stream) {
    if (int e = check_geom(gp)) return e;
    if (gp->dl_d != 1 || gp->dl_h != 1 || gp->dl_w != 1) return CN_EUNSUPPORTED;
    const CnConvGeom d = dgrad_geom(*gp);
    return cn_conv_fwd_dt(&d, gy, gy_dt, w_tflip, nullptr, gu, gu_dt, CN_ACT_NONE, 0.f, stream);
}

// Data gradient straight from the ORIGINAL filter w [t][cin][cout] (no cn_conv_weight_tflip copy): CN_EUNSUPPORTED (nothing
// launched) where the shape does not reach the vectorised implicit-GEMM kernel -- the caller then uses cn_conv_dgrad.
extern "C" int cn_conv_dgrad_w(const CnConvGeom* gp, const float* gy, const float* w, float* gu, void* stream) {
    if (int e = check_geom(gp)) return e;
    if (gp->dl_d != 1 || gp->dl_h != 1 || gp->dl_w != 1) return CN_EUNSUPPORTED;
    const CnConvGeom d = dgrad_geom(*gp);
    return conv_fwd(&d, ConvReq{1, 0, CN_ACT_NONE, 0, 0, CN_F32, CN_F32}, gy, w, nullptr, nullptr, gu, 0.f, nullptr, 0.f, stream);
}

// gu = (data gradient of cn_conv_dgrad_w) + res, res shaped like gu: the SECOND contribution to the gradient of a tensor that
// feeds a convolution AND a skip connection (a ResNet bottleneck's input, real_encoder.py:13: the gradient of keras' `Add`),
// added in the data-gradient launch's epilogue instead of by a separate pass.  Stride-1 layers whose launch is an unsplit
// implicit-GEMM one; CN_EUNSUPPORTED (nothing launched) otherwise -- the caller then adds with a pass of its own.
extern "C" int cn_conv_dgrad_w_res(const CnConvGeom* gp, const float* gy, const float* w, const float* res, float* gu, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(res, "cn_conv_dgrad_w_res: res is NULL");
    if (gp->dl_d != 1 || gp->dl_h != 1 || gp->dl_w != 1 || gp->up) return CN_EUNSUPPORTED;
    if (gp->s_d != 1 || gp->s_h != 1 || gp->s_w != 1) return CN_EUNSUPPORTED;      // (parity-ordered rows: not with a residual)
    const CnConvGeom d = dgrad_geom(*gp);
    return conv_fwd(&d, ConvReq{1, 0, CN_ACT_NONE, 1, 0, CN_F32, CN_F32}, gy, w, nullptr, res, gu, 0.f, nullptr, 0.f, stream);
}

// cn_conv_dgrad_w[_res] with the ReLU backward of the layer in front in the launch's epilogue (include/confignet_hip.h):
//     gu = (data gradient (+ res)) * (mask > 0),   colsum[c] += sum_rows gu[.][c],   colsum2[c] += the same
// -- the bits cn_conv_dgrad_w[_res] followed by cn_act_bwd(.., mask, CN_ACT_RELU) stores, and the shift sums cn_act_bwd_bias would
// take in a pass of its own (a ResNet block's shortcut convolution receives the sums of its last convolution: colsum2).  res, colsum
// and colsum2 may be NULL.  Served by the unsplit launches of the LDS-DMA loop on 32-wide blocks, stride 1, no upsampling;
// everything else -- and any request for sums in deterministic mode, whose order of additions the atomics do not fix --
// CN_EUNSUPPORTED with nothing enqueued: the caller then runs the data gradient and the pass.
extern "C" int cn_conv_dgrad_w_mask(const CnConvGeom* gp, const float* gy, const float* w, const float* res, const float* mask, float* gu,
                                    float* colsum, float* colsum2, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(gy && w && mask && gu, "cn_conv_dgrad_w_mask: NULL tensor");
    if (gp->dl_d != 1 || gp->dl_h != 1 || gp->dl_w != 1 || gp->up) return CN_EUNSUPPORTED;
    if (gp->s_d != 1 || gp->s_h != 1 || gp->s_w != 1) return CN_EUNSUPPORTED;      // (parity-ordered rows: as cn_conv_dgrad_w_res)
    if ((colsum || colsum2) && cn_det()) return CN_EUNSUPPORTED;
    const CnConvGeom d = dgrad_geom(*gp);
    const ConvReq q{1, 0, CN_ACT_NONE, res != nullptr, 0, CN_F32, CN_F32, 1};
    const ConvPlan p = plan_conv_fwd(d, q);
    if (p.route == CN_ROUTE_UNSUPPORTED) return p.ret;
    // (what the plan does not know: a tile forced by cn_conv_tune that has no mask instance, the 16-wide-block body at 48 channels)
    if (p.splits > 1 || !cn_fwd2_takes_mask(p.cfg, 1, !p.plain, d.cout, 0, CN_ACT_NONE, 0)) return CN_EUNSUPPORTED;
    return run_conv_fwd(p, d, q, gy, w, nullptr, res, gu, 0.f, nullptr, 0.f, (hipStream_t)stream, ConvEp{mask, colsum, colsum2});
}

// Diagnostic (include/confignet_hip.h): the launch a request WOULD get -- needs no device, enqueues nothing.
extern "C" int cn_conv_fwd_plan(const CnConvGeom* gp, int bt, int has_bias, int act, int has_res, int stats_mode, int x_dt, int y_dt,
                                int out[8]) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(out, "cn_conv_fwd_plan: out is NULL");
    const ConvPlan p = plan_conv_fwd(*gp, ConvReq{bt, has_bias, act, has_res, stats_mode, x_dt, y_dt});
    const int v[8] = {p.route, p.cfg, p.splits, p.par, p.family, p.grid[0], p.grid[1], p.grid[2]};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return p.ret;
}

// cn_conv_fwd_plan for a request with the mask epilogue (has_mask = 0: cn_conv_fwd_plan itself).
extern "C" int cn_conv_fwd_plan_ep(const CnConvGeom* gp, int bt, int has_bias, int act, int has_res, int stats_mode, int has_mask, int x_dt,
                                   int y_dt, int out[8]) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(out, "cn_conv_fwd_plan_ep: out is NULL");
    const ConvPlan p = plan_conv_fwd(*gp, ConvReq{bt, has_bias, act, has_res, stats_mode, x_dt, y_dt, has_mask != 0});
    const int v[8] = {p.route, p.cfg, p.splits, p.par, p.family, p.grid[0], p.grid[1], p.grid[2]};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return p.ret;
}

// ---- the filter gradient --------------------------------------------------------------------------------------------------------
// plan_conv_wgrad decides the launch from the geometry and the request alone (route, tile, row slices, grid, profile family, the
// workspace the caller provides, zero pass, the reduction that follows -- no HIP call, no pointer); run_conv_wgrad performs it and is
// the only place a filter-gradient kernel is launched from.  The entry points build a request -- the storage types, whether the
// slabs stay with the caller, and the routes the entry has always taken -- plan and run; cn_conv_wgrad_dt takes every route.
namespace {

struct WgradReq {
    int x_dt, gy_dt;
    bool caller_slabs;       // a row-split LDS-DMA launch leaves its slabs in the workspace for the caller to add
    unsigned routes;         // bit r set: route r (WgradRoute) may be taken
    bool det = cn_det() != 0;        // deterministic mode (cn_conv_wgrad_plan may ask for either)
};
constexpr unsigned wg_bit(int r) { return 1u << r; }
constexpr unsigned WG_ATOMIC = wg_bit(CN_WG_TINY) | wg_bit(CN_WG_IGEMM), WG_FP32_GEMM = wg_bit(CN_WG_WGRAD2) | WG_ATOMIC, WG_ALL = ~0u;

enum { WG_SUM_NONE = 0, WG_SUM_PARTS, WG_SUM_C3, WG_SUM_CALLER };      // what follows the launch: nothing, cn_sum_parts, c3_wgrad_reduce_kernel, the caller's own sum

struct WgradPlan {
    int route = CN_WG_NONE;
    int ret = CN_EUNSUPPORTED;       // what the request gets when nothing is launched (route == CN_WG_NONE)
    int cfg = -1;                    // tile of the GEMM routes, implicit-GEMM numbering (5 = 256 x 64)
    int stages = 0;                  // WGRAD2: stages of the LDS-DMA loop
    long splits = 1, rows = 0;       // GEMM routes: row slices and rows per slice
    int tx = 0, ty = 0;              // WGRAD2: tiles over filter rows / output channels; IGEMM / BF16: the same when the grid is the XCD-ordered 1-D one, else 0; C3 / THIN: tiles of output pixels per row / column
    int family = -1;                 // CN_FAM_* of the profile bracket; -1: the launch has none
    int grid[3] = {0, 0, 0};
    size_t lds = 0;                  // C3 / THIN: dynamic LDS bytes
    size_t ws_floats = 0;            // workspace the caller provides: slabs (WGRAD2), partial filters (C3, THIN)
    size_t det_floats = 0;           // TINY / IGEMM / BF16 in deterministic mode: partials in the stream's workspace instead of atomics
    bool zero = false;               // the atomic routes: a zero pass precedes the launch when the target is to be written
    int sum = WG_SUM_NONE;
};

struct WgTile { int bm, bn; };       // rows of (tap, ci) x output channels
WgTile wgrad_tile(int cfg) { return cfg == 3 ? WgTile{128, 32} : cfg == 4 ? WgTile{128, 96} : cfg == 0 ? WgTile{128, 128} : cfg == 5 ? WgTile{256, 64} : WgTile{64, 64}; }
int wgrad_family(int cfg) {
    return cfg == 3 ? CN_FAM_WGRAD_128x32 : cfg == 4 ? CN_FAM_WGRAD_128x96 : cfg == 0 ? CN_FAM_WGRAD_128x128 : cfg == 5 ? CN_FAM_WGRAD_256x64 : CN_FAM_WGRAD_64x64;
}

// Grid of the atomic and the bf16 kernel: (filter-row tiles, channel tiles, slices), or from 16 slices of more than one tile up the
// XCD-aware 1-D order (igemm_wgrad_kernel: every tile of ONE row slice on the same XCD), padded to whole groups of 8 slices
void sliced_grid(const CnConvGeom& g, WgTile t, WgradPlan& p) {
    const long Ktot = (long)g.k_d * g.k_h * g.k_w * g.cin;
    const int gx = cn_cdiv(Ktot, t.bm), gy = cn_cdiv(g.cout, t.bn);
    p.grid[0] = gx; p.grid[1] = gy; p.grid[2] = (int)p.splits;
    if ((long)gx * gy > 1 && p.splits >= 16) {
        p.tx = gx; p.ty = gy;
        p.grid[0] = cn_cdiv(p.splits, 8) * 8 * gx * gy; p.grid[1] = p.grid[2] = 1;
    }
}

// Row slices of the atomic kernel (igemm_wgrad_kernel): from a workgroup target, at least 256 rows each.  false (+ error string): in
// deterministic mode not even one partial filter fits the stream's workspace.
bool igemm_wgrad_slices(const CnConvGeom& g, WgTile t, long wg_target, bool det, WgradPlan& p) {
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    const long Ktot = (long)g.k_d * g.k_h * g.k_w * g.cin;
    const long tiles = (long)cn_cdiv(Ktot, t.bm) * cn_cdiv(g.cout, t.bn);
    const long wg_blocks = wg_target > 0 ? wg_target : 2048;   // sweep 256..4096: flat from 1536 up
    long splits = (wg_blocks + tiles - 1) / tiles;
    if (det) {
        // deterministic mode: per-split partial filters in the stream's workspace, added in split order by a second launch
        // (every split of every tile writes its whole slab region: no clearing).  As many splits as the workspace holds.
        const long cap = (long)(CN_DET_WS_FLOATS / ((size_t)Ktot * g.cout));
        if (cap < 1) {
            cn_set_error("deterministic filter gradient: %ld x %d filter does not fit the workspace", Ktot, g.cout);
            return false;
        }
        if (splits > cap) splits = cap;
    }
    long rows = (M + splits - 1) / splits;
    if (rows < 256) rows = 256;
    rows = (rows + BK - 1) / BK * BK;
    p.rows = rows;
    p.splits = (M + rows - 1) / rows;
    return true;
}

// Row slices of the bf16 kernel (round-5 sweep, profiles/round5_bf16_wgrad_splits.txt).  What the sweep showed: (1) a slice shorter
// than ~512 rows is mostly prologue + the tile's atomic adds; (2) one workgroup more than the CUs hold at once costs a whole extra
// round -- the kernels hold 3 (128 x 128), 4 (128 x 96) or 5 workgroups per CU -- and the narrow tiles like two rounds; (3) with the
// XCD order a slice count that is not a multiple of 8 leaves XCDs with one slice more than others.
// det: the slices' partial filters go to the stream's deterministic workspace, so no more slices than it holds -- a clamp that the
// rule above never reaches today (its largest slices x filter over taps 1..64, channels 8..2048 and 2^8..2^22 rows is 0.75 of the
// workspace: tests/test_bf16_det_plan_cpu.py) and that only keeps a later rule from overflowing.  Where not even one partial filter
// fits, one slice: it needs no partials.
void bf16_wgrad_slices(const CnConvGeom& g, WgTile t, bool det, WgradPlan& p) {
    constexpr long KS = 32, min_rows = 512;          // (KS: bf16 reduction rows per LDS stage, igemm_bf16.hip)
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    const long Ktot = (long)g.k_d * g.k_h * g.k_w * g.cin;
    const long tiles = (long)cn_cdiv(Ktot, t.bm) * cn_cdiv(g.cout, t.bn);
    const long per_cu = t.bm * t.bn >= 128 * 128 ? 3 : t.bm * t.bn >= 128 * 96 ? 4 : 5;
    const long target = 256 * per_cu * (t.bn >= 96 ? 1 : 2);
    long splits = target / tiles;
    if (splits > M / min_rows) splits = M / min_rows;
    const long fill = std::min<long>(M / 256, (256 + tiles - 1) / tiles);        // ... but at least one workgroup per CU
    if (splits < fill) splits = fill;
    if (splits >= 16) splits &= ~7L;
    if (splits < 1) splits = 1;
    long rows = (M + splits - 1) / splits;
    if (rows < 256) rows = std::min<long>(256, (M + KS - 1) / KS * KS);
    rows = (rows + KS - 1) / KS * KS;
    p.rows = rows;
    p.splits = (M + rows - 1) / rows;
    const long cap = std::max<long>(1, (long)(CN_DET_WS_FLOATS / ((size_t)Ktot * g.cout)));
    if (det && p.splits > cap) {
        p.rows = ((M + cap - 1) / cap + KS - 1) / KS * KS;
        p.splits = (M + p.rows - 1) / p.rows;
    }
}

// Pure: reads the geometry, the request (deterministic mode is part of it), cn_cu_count() and the tuning overrides.  The routes are asked in the order the
// callers always asked them: K = 27, thin, bf16, then the fp32 GEMM kernels.
WgradPlan plan_conv_wgrad(const CnConvGeom& g, const WgradReq& q) {
    WgradPlan p;
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    const long Ktot = (long)g.k_d * g.k_h * g.k_w * g.cin;
    const size_t count = (size_t)Ktot * g.cout;
    const bool x32 = q.x_dt == CN_F32, y32 = q.gy_dt == CN_F32, x16 = q.x_dt == CN_BF16, y16 = q.gy_dt == CN_BF16;
    auto may = [&q](int route) { return (q.routes & wg_bit(route)) != 0; };
    auto take = [&p](int route, int family) {
        p.route = route;
        p.ret = CN_OK;
        p.family = family;
    };
    // K = 27 first layers (3x3 on the 3-channel fp32 image, stride 1 / 2; gy in either storage type): staged-tile kernel without
    // atomics -- the generic split-over-rows kernel runs them at 10 TFLOP/s
    if (may(CN_WG_C3) && x32 && (y32 || y16) && g.nd == 2 && g.cin == 3 && g.k_h == 3 && g.k_w == 3 && g.k_d == 1 && g.s_h == g.s_w &&
        (g.s_h == 1 || g.s_h == 2) && g.dl_h == 1 && g.dl_w == 1 && g.up == 0 && g.cout <= 64 && g.cout >= 4 && g.cout % 4 == 0) {
        take(CN_WG_C3, CN_FAM_C3_WGRAD);
        p.tx = cn_cdiv(g.out_w, CN_C3_WGRAD_TILE);
        p.grid[0] = CN_C3_WGRAD_PARTS; p.grid[1] = p.grid[2] = 1;
        const int pw = CN_C3_WGRAD_TILE * g.s_h + 2, gpitch = (g.cout + 3) & ~3;
        p.lds = sizeof(float) * 4 * (size_t)(3 * pw * 3 + CN_C3_WGRAD_TILE * gpitch);
        if (p.lds < sizeof(float) * 4 * 2 * 16 * 64) p.lds = sizeof(float) * 4 * 2 * 16 * 64;
        p.ws_floats = CN_C3_WGRAD_PARTS * count;
        p.sum = WG_SUM_C3;
        return p;
    }
    // thin output (map_final): staged-tile VALU kernel with ordered partial sums -- the implicit-GEMM kernel runs it at 6 TFLOP/s.
    // A patch that does not fit the LDS goes on to the next route.
    const int T = g.k_h * g.k_w;
    if (may(CN_WG_THIN) && x32 && y32 && g.nd == 2 && g.cout <= 4 && g.cin % 4 == 0 && g.cin >= 8 && g.cin <= 64 && g.s_h == 1 && g.s_w == 1 &&
        g.dl_h == 1 && g.dl_w == 1 && T <= 16 && T * (g.cin / 4) <= 256) {
        const int PH0 = ((CN_THIN_WGRAD_TH + g.k_h - 1) >> g.up) + 2, PW0 = ((CN_THIN_WGRAD_TW + g.k_w - 1) >> g.up) + 2;
        size_t lds = sizeof(float) * ((size_t)PH0 * PW0 * g.cin + CN_THIN_WGRAD_TH * CN_THIN_WGRAD_TW * 4);
        const size_t red = sizeof(float) * 256 * 4 * g.cout;
        if (lds < red) lds = red;
        if (lds <= 64 * 1024) {
            take(CN_WG_THIN, -1);
            p.ty = cn_cdiv(g.out_h, CN_THIN_WGRAD_TH); p.tx = cn_cdiv(g.out_w, CN_THIN_WGRAD_TW);
            const int ntiles = g.n * p.ty * p.tx;
            p.grid[0] = ntiles < CN_THIN_WGRAD_PARTS ? ntiles : CN_THIN_WGRAD_PARTS; p.grid[1] = p.grid[2] = 1;
            p.lds = lds;
            p.ws_floats = CN_THIN_WGRAD_PARTS * count;
            p.sum = WG_SUM_PARTS;
            return p;
        }
    }
    if (x16 && y16) {        // bf16 operands: 16-byte pieces of 8 channels; the slices' tiles meet in fp32 atomics, in deterministic mode in ordered slabs
        if (!may(CN_WG_BF16) || g.cin % 8 || g.cout % 8) return p;
        take(CN_WG_BF16, CN_FAM_BF16_WGRAD);
        p.cfg = wgrad_tile_cfg(g);
        bf16_wgrad_slices(g, wgrad_tile(p.cfg), q.det, p);
        sliced_grid(g, wgrad_tile(p.cfg), p);
        p.zero = true;
        if (q.det && p.splits > 1) {      // (one slice: one writer per element and launch, the atomics are ordered as they are)
            p.det_floats = (size_t)p.splits * count;
            p.sum = WG_SUM_PARTS;
        }
        return p;
    }
    if (!x32 || !y32) return p;
    // Every geometry the LDS-DMA kernel can take (round 6: with the slot layout and the XCD-aware slice plan it is at or ahead of
    // the round-3 kernel -- split over rows, fp32 atomics -- on every shape of the iteration, profiles/round6_wgrad_shapes.txt): row
    // slices through slabs in the caller's workspace + one ordered reduction, bit-reproducible in every mode.
    // The round-3 kernel keeps the rest: channel counts that are no multiple of 4, K < 64, > 2 GiB operands.
    if (may(CN_WG_WGRAD2) && cn_wgrad2_ok(g) && Ktot >= 64) {
        const int t = g_tune_cfg;          // (cn_conv_tune: the tiles this kernel has, anything else = its own choice)
        const Wg2Plan w = cn_wgrad2_plan(g, t == 0 || t == 2 || t == 3 || t == 4 || t == 5 ? t : -1, g_tune_wg_blocks);
        take(CN_WG_WGRAD2, wgrad_family(w.cfg));
        p.cfg = w.cfg;
        p.stages = w.cfg == 3 || g_tune_wg2_ns == 3 ? 3 : 4;
        p.splits = w.splits; p.rows = w.rows;
        p.tx = (int)w.tiles_x; p.ty = (int)w.tiles_y;
        // (from 8 slices up the XCD-aware order, padded to whole groups of 8 slices)
        p.grid[0] = (int)((w.splits >= 8 ? cn_cdiv(w.splits, 8) * 8 : w.splits) * w.tiles_x * w.tiles_y); p.grid[1] = p.grid[2] = 1;
        if (w.splits > 1) {
            p.ws_floats = (size_t)w.splits * count;
            p.sum = q.caller_slabs ? WG_SUM_CALLER : WG_SUM_PARTS;
        }
        return p;
    }
    // the from-RGB shapes (1x1, cin and cout <= 4)
    if (may(CN_WG_TINY) && Ktot <= 4 && g.cout <= 4 && g.k_d * g.k_h * g.k_w == 1 && g.s_h == 1 && g.s_w == 1 && g.s_d == 1 && !g.up &&
        g.p_h == 0 && g.p_w == 0 && g.p_d == 0) {
        take(CN_WG_TINY, -1);
        p.grid[0] = cn_cdiv(M, 256) > 1024 ? 1024 : cn_cdiv(M, 256); p.grid[1] = p.grid[2] = 1;
        p.zero = true;
        if (q.det) {                     // deterministic mode: per-workgroup partials, added in workgroup order
            p.det_floats = (size_t)p.grid[0] * 16;
            p.sum = WG_SUM_PARTS;
        }
        return p;
    }
    if (!may(CN_WG_IGEMM)) return p;
    const int cfg = wgrad_tile_cfg(g);
    if (!igemm_wgrad_slices(g, wgrad_tile(cfg), g_tune_wg_blocks, q.det, p)) {
        p.ret = CN_EINVAL;
        return p;
    }
    take(CN_WG_IGEMM, wgrad_family(cfg));
    p.cfg = cfg;
    sliced_grid(g, wgrad_tile(cfg), p);
    p.zero = true;
    if (q.det) {
        p.det_floats = (size_t)p.splits * count;
        p.sum = WG_SUM_PARTS;
    }
    return p;
}

// The launch check and the reduction that follows a launch: cn_sum_parts over the workspace's (or, in deterministic mode, the stream's)
// partials, the K = 27 kernel's own sum, or nothing here where the slabs stay with the caller.
int sum_conv_wgrad(const WgradPlan& p, int nparts, long count, int mode, float* gw, const float* ws, const float* det, int* parts_out,
                   hipStream_t s) {
    CN_LAUNCH_CHECK();
    const int add = mode != CN_WGRAD_WRITE;
    if (p.sum == WG_SUM_PARTS) return cn_sum_parts(det ? det : ws, gw, nparts, count, det ? 1 : add, 1.f, s);      // (det: gw was cleared or holds the sum so far)
    if (p.sum == WG_SUM_C3) {
        cn_c3_wgrad_reduce(ws, gw, nparts, (int)count, mode == CN_WGRAD_ADD, s);
        CN_LAUNCH_CHECK();
    }
    if (p.sum == WG_SUM_CALLER) *parts_out = nparts;
    return CN_OK;
}

// Performs the plan: zero pass, profile bracket, ONE launch, launch check, the reduction that follows.  A plan without a launch
// returns its code before anything is enqueued.  mode: CN_WGRAD_WRITE / _ADD / _ZEROED (include/confignet_hip.h) -- a target known
// to be zero is added to, except by the K = 27 route, which writes it.
int run_conv_wgrad(const WgradPlan& p, const CnConvGeom& g, const WgradReq& q, const void* x, const void* gy, float* gw, int mode,
                   float* ws, size_t ws_bytes, int* parts_out, hipStream_t s) {
    if (parts_out) *parts_out = 0;
    if (p.route == CN_WG_NONE) return p.ret;
    CN_CHECK_ARG(mode == CN_WGRAD_WRITE || mode == CN_WGRAD_ADD || mode == CN_WGRAD_ZEROED, "filter gradient: mode %d", mode);
    CN_CHECK_ARG(p.ws_floats == 0 || (ws && ws_bytes >= sizeof(float) * p.ws_floats), "filter gradient: workspace of %zu bytes, %zu needed",
                 ws ? ws_bytes : (size_t)0, sizeof(float) * p.ws_floats);
    CN_CHECK_ARG(p.sum != WG_SUM_CALLER || parts_out, "filter gradient: slabs left to a caller that takes none");
    CN_CHECK_ARG(p.route != CN_WG_BF16 || (((uintptr_t)x | (uintptr_t)gy) & 15) == 0, "bf16 convolution needs 16-byte aligned tensors");
    const long count = (long)g.k_d * g.k_h * g.k_w * g.cin * g.cout;
    const int add = mode != CN_WGRAD_WRITE;
    float* det = nullptr;
    if (p.det_floats) {
        det = cn_det_ws(s, p.det_floats);
        if (!det) return CN_EINVAL;
    }
    if (p.zero && !add) {
        if (int ez__ = cn_zero_async(gw, sizeof(float) * count, s)) return ez__;
    }
    if (p.family >= 0)
        cn_prof_begin(s, p.route == CN_WG_C3 ? 2.0 * 27.0 * g.cout * (double)g.n * g.out_h * g.out_w : conv_flops(g),
                      conv_bytes(g, q.x_dt == CN_BF16 ? 2.0 : 4.0, q.gy_dt == CN_BF16 ? 2.0 : 4.0, 4.0), p.family);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    int nparts = (int)p.splits, e = CN_OK;       // partials the reduction adds: row slices, or the workgroups of the C3 / THIN / TINY launch
    switch (p.route) {
        case CN_WG_C3:
            e = cn_c3_wgrad(g, (const float*)x, gy, q.gy_dt, ws, p.tx, g.n * g.out_h * p.tx, nparts = p.grid[0], p.lds, s);
            break;
        case CN_WG_THIN:
            cn_thin_wgrad(g, (const float*)x, (const float*)gy, ws, nparts = p.grid[0], p.lds, p.ty, p.tx, g.n * p.ty * p.tx, s);
            break;
        case CN_WG_TINY:
            nparts = cn_tiny_wgrad(g, (const float*)x, (const float*)gy, gw, p.grid[0], det, s);
            break;
        case CN_WG_WGRAD2:
            cn_wgrad2(p.cfg, p.stages, g, (const float*)x, (const float*)gy, p.splits > 1 ? ws : gw, p.splits > 1 ? count : 0, (int)p.rows,
                      p.tx, p.ty, (int)p.splits, add, grid.x, s);
            break;
        case CN_WG_IGEMM:
            cn_igemm_wgrad(p.cfg, g, (const float*)x, (const float*)gy, gw, (int)p.rows, det, p.tx, p.ty, (int)p.splits, grid, s);
            break;
        default:
            cn_bf16_wgrad(p.cfg, g, x, gy, gw, (int)p.rows, det, p.tx, p.ty, (int)p.splits, grid, s);
            break;
    }
    const bool sum_in_bracket = p.route != CN_WG_C3;      // (the K = 27 bracket has always closed in front of its reduction)
    if (p.family >= 0 && !sum_in_bracket) cn_prof_end(s);
    if (e == CN_OK) e = sum_conv_wgrad(p, nparts, count, mode, gw, ws, det, parts_out, s);
    if (p.family >= 0 && sum_in_bracket) cn_prof_end(s);
    return e;
}

// argument checks, plan, run: the body of the filter-gradient entries below
int conv_wgrad(const CnConvGeom* gp, const WgradReq& q, const void* x, const void* gy, float* gw, int mode, void* ws, size_t ws_bytes,
               int* parts, void* stream) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(x && gy && gw, "NULL tensor");
    return run_conv_wgrad(plan_conv_wgrad(*gp, q), *gp, q, x, gy, gw, mode, (float*)ws, ws_bytes, parts, (hipStream_t)stream);
}

}  // namespace

// The atomic kernels alone (the from-RGB shapes, the row-split kernel): no workspace of the caller's.
extern "C" int cn_conv_wgrad(const CnConvGeom* gp, const float* x, const float* gy, float* gw, int accumulate, void* stream) {
    return conv_wgrad(gp, WgradReq{CN_F32, CN_F32, false, WG_ATOMIC}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, nullptr, 0, nullptr, stream);
}

// Workspace (bytes) that cn_conv_wgrad_ws needs for this geometry: room for the partial filters of its row splits; 0 = none.
extern "C" size_t cn_conv_wgrad_workspace_bytes(const CnConvGeom* gp) {
    if (!gp || check_geom(gp) != CN_OK) return 0;
    return sizeof(float) * plan_conv_wgrad(*gp, WgradReq{CN_F32, CN_F32, false, WG_FP32_GEMM}).ws_floats;
}

// Filter gradient with a CALLER-OWNED workspace (the caller owns all device memory): the LDS-DMA kernel where it takes
// the geometry, else the atomic kernels, which need no workspace.
extern "C" int cn_conv_wgrad_ws(const CnConvGeom* gp, const float* x, const float* gy, float* gw, int accumulate, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return conv_wgrad(gp, WgradReq{CN_F32, CN_F32, false, WG_FP32_GEMM}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, workspace,
                      workspace_bytes, nullptr, stream);
}

// cn_conv_wgrad_ws that leaves the slabs to the caller (include/confignet_hip.h): *parts = 0 -> gw is complete
extern "C" int cn_conv_wgrad_ws_slabs(const CnConvGeom* gp, const float* x, const float* gy, float* gw, int accumulate, void* workspace,
                                      size_t workspace_bytes, int* parts, void* stream) {
    CN_CHECK_ARG(parts, "cn_conv_wgrad_ws_slabs: parts is NULL");
    return conv_wgrad(gp, WgradReq{CN_F32, CN_F32, true, WG_FP32_GEMM}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, workspace,
                      workspace_bytes, parts, stream);
}

extern "C" int cn_conv_wgrad_bf16(const CnConvGeom* gp, const uint16_t* x, const uint16_t* gy, float* gw, int accumulate,
                                  void* stream) {
    return conv_wgrad(gp, WgradReq{CN_BF16, CN_BF16, false, wg_bit(CN_WG_BF16)}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, nullptr, 0,
                      nullptr, stream);
}

// Number of partial filters (27 x cout floats each) the caller provides as scratch.
extern "C" int cn_conv_wgrad_c3_partials(void) { return CN_C3_WGRAD_PARTS; }

// Filter gradient of a 3x3 convolution of a 3-channel fp32 image (g->cin == 3, stride 1 or 2, no dilation / upsample,
// cout <= 64 and a multiple of 4); gy in fp32 or bf16 (gy_dt).  scratch: cn_conv_wgrad_c3_partials() * 27 * cout floats.  accumulate: add to gw.
// Returns CN_EUNSUPPORTED (nothing launched) for other geometries.
extern "C" int cn_conv_wgrad_c3(const CnConvGeom* gp, const float* x, const void* gy, int gy_dt, float* scratch, float* gw,
                                int accumulate, void* stream) {
    CN_CHECK_ARG(gp && x && gy && scratch && gw && (gy_dt == CN_F32 || gy_dt == CN_BF16), "conv_wgrad_c3: bad args");
    return conv_wgrad(gp, WgradReq{CN_F32, gy_dt, false, wg_bit(CN_WG_C3)}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, scratch, SIZE_MAX,
                      nullptr, stream);
}

extern "C" int cn_conv_wgrad_thin_partials(void) { return CN_THIN_WGRAD_PARTS; }

// Filter gradient for cout <= 4 (thin_wgrad.hip).  scratch: cn_conv_wgrad_thin_partials() * taps * cin * cout floats.
// accumulate: add to gw.  CN_EUNSUPPORTED (nothing launched) for every other geometry.
extern "C" int cn_conv_wgrad_thin(const CnConvGeom* gp, const float* x, const float* gy, float* scratch, float* gw, int accumulate,
                                  void* stream) {
    CN_CHECK_ARG(scratch, "conv_wgrad_thin: NULL");
    return conv_wgrad(gp, WgradReq{CN_F32, CN_F32, false, wg_bit(CN_WG_THIN)}, x, gy, gw, accumulate ? CN_WGRAD_ADD : CN_WGRAD_WRITE, scratch, SIZE_MAX,
                      nullptr, stream);
}

// The routed filter gradient (include/confignet_hip.h): every route, the operands in the storage types the caller holds them in.
extern "C" int cn_conv_wgrad_dt_workspace_bytes(const CnConvGeom* gp, int x_dt, int gy_dt, size_t* bytes) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(bytes, "cn_conv_wgrad_dt_workspace_bytes: bytes is NULL");
    const WgradPlan p = plan_conv_wgrad(*gp, WgradReq{x_dt, gy_dt, false, WG_ALL});
    *bytes = sizeof(float) * p.ws_floats;
    return p.ret;
}

extern "C" int cn_conv_wgrad_dt(const CnConvGeom* gp, const void* x, int x_dt, const void* gy, int gy_dt, float* gw, int mode, void* workspace,
                                size_t workspace_bytes, int* parts, void* stream) {
    return conv_wgrad(gp, WgradReq{x_dt, gy_dt, parts != nullptr, WG_ALL}, x, gy, gw, mode, workspace, workspace_bytes, parts, stream);
}

// Diagnostic (include/confignet_hip.h): the launch a filter-gradient request WOULD get -- needs no device, enqueues nothing.
extern "C" int cn_conv_wgrad_plan(const CnConvGeom* gp, int x_dt, int gy_dt, int caller_slabs, unsigned routes, int det, long long out[12]) {
    if (int e = check_geom(gp)) return e;
    CN_CHECK_ARG(out, "cn_conv_wgrad_plan: out is NULL");
    const WgradPlan p = plan_conv_wgrad(*gp, WgradReq{x_dt, gy_dt, caller_slabs != 0, routes, det < 0 ? cn_det() != 0 : det != 0});
    const long long v[12] = {p.route, p.cfg, p.splits, p.rows, p.family, p.grid[0], p.grid[1], p.grid[2], (long long)p.ws_floats, p.zero, p.sum, p.stages};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return p.ret;
}

// ---- many filter gradients in a few launches ------------------------------------------------------------------------------------
// The filter gradients of a backward pass whose data gradients alone feed its chain (the ResNet-50 trunk: 52 of them at the exposed
// end of the generator step) need not each fill the chip by themselves.  plan_conv_wgrad_group decides for the whole list -- tile,
// launch, row slices, first workgroup of every job -- and is the only place that does; cn_conv_wgrad_grouped performs the plan,
// cn_conv_wgrad_grouped_plan reports it without a device.  The slabs of the jobs with row slices always stay with the caller.
namespace {

struct WgGroupJob {
    int cfg = -1, stages = 0, tx = 0, ty = 0, launch = 0;
    long splits = 1, rows = 0, blk0 = 0, wgs = 0;
    size_t ws_floats = 0;
};

bool wgrad_groupable(const CnConvGeom& g) { return cn_wgrad2_ok(g) && (long)g.k_d * g.k_h * g.k_w * g.cin >= 64; }

// The rule.  A launch holds jobs of ONE tile configuration, at most CN_WG2_GROUP of them (the argument block), in the order of the
// list; its workgroups number about two per CU -- one full round as wg2_cost models it -- and a job gets the share of them that
// its matrix work (rows x filter elements) has in the launch's; cn_wgrad2_plan(group) turns that share into slices (whole XCD
// rounds from 8 up, never more than the job would take alone).  Equal shares of work per workgroup are equal lifetimes: the launch
// ends everywhere at once, most 1x1 layers need one slice or a few, and a job whose tiles alone exceed its share runs unsplit.
// The tile is chosen first, from the job's share of the whole list (the tile that takes least of the chip), since the launches are
// cut by it.
// solo: every job planned as the launch of its own that cn_conv_wgrad_ws gives it (tests: the same body on the same numbers).
// Pure: reads the geometries, cn_cu_count() and the tuning overrides.  false: a job the LDS-DMA kernel does not take.
bool plan_conv_wgrad_group(int njobs, const CnConvGeom* g, bool solo, std::vector<WgGroupJob>& jobs, std::vector<long>& grids) {
    jobs.assign(njobs, WgGroupJob{});
    grids.clear();
    std::vector<double> work(njobs);
    double work_all = 0.0;
    for (int j = 0; j < njobs; ++j) {
        if (!wgrad_groupable(g[j])) return false;
        work[j] = (double)g[j].n * g[j].out_d * g[j].out_h * g[j].out_w * g[j].k_d * g[j].k_h * g[j].k_w * g[j].cin * g[j].cout;
        work_all += work[j];
    }
    const double chip = 2.0 * cn_cu_count();
    auto share = [&](double w, double of, double launches) { return std::max(1L, (long)(chip * launches * w / of + 0.5)); };
    const int tuned = g_tune_cfg == 0 || (g_tune_cfg >= 2 && g_tune_cfg <= 5) ? g_tune_cfg : -1;
    // 1. the tile (solo: the whole plan)
    for (int j = 0; j < njobs; ++j) {
        WgGroupJob& q = jobs[j];
        if (solo) {
            const WgradPlan p = plan_conv_wgrad(g[j], WgradReq{CN_F32, CN_F32, true, WG_FP32_GEMM});
            q.cfg = p.cfg; q.splits = p.splits; q.rows = p.rows; q.tx = p.tx; q.ty = p.ty;
        } else {
            q.cfg = cn_wgrad2_plan(g[j], tuned, share(work[j], work_all, cn_cdiv(njobs, CN_WG2_GROUP)), true).cfg;
        }
        q.stages = q.cfg == 3 ? 3 : 4;
    }
    // 2. the launches: by tile, in list order, as many jobs as the argument block holds
    std::vector<int> open(8, -1), count;
    std::vector<double> work_of;
    for (int j = 0; j < njobs; ++j) {
        int& l = open[jobs[j].cfg];
        if (l < 0 || count[l] == CN_WG2_GROUP) {
            l = (int)count.size();
            count.push_back(0);
            work_of.push_back(0.0);
        }
        jobs[j].launch = l;
        ++count[l];
        work_of[l] += work[j];
    }
    // 3. the slices from the job's share of its launch; the workgroup ranges, the jobs with the longest workgroups first (the
    // hardware starts workgroups in id order as slots come free: short ones at the end fill the tail, long ones would be it)
    grids.assign(count.size(), 0);
    std::vector<int> order(njobs);
    for (int j = 0; j < njobs; ++j) {
        WgGroupJob& q = jobs[j];
        order[j] = j;
        if (!solo) {
            const Wg2Plan w = cn_wgrad2_plan(g[j], q.cfg, share(work[j], work_of[q.launch], 1.0), true);
            q.splits = w.splits; q.rows = w.rows; q.tx = (int)w.tiles_x; q.ty = (int)w.tiles_y;
        }
        q.wgs = (q.splits >= 8 ? cn_cdiv(q.splits, 8) * 8 : q.splits) * q.tx * q.ty;      // (the XCD-round order pads to 8 slices)
        if (q.splits > 1) q.ws_floats = (size_t)q.splits * g[j].k_d * g[j].k_h * g[j].k_w * g[j].cin * g[j].cout;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return jobs[a].rows > jobs[b].rows; });
    for (int j : order) {
        WgGroupJob& q = jobs[j];
        q.blk0 = grids[q.launch];
        grids[q.launch] += q.wgs;
    }
    for (long gr : grids)
        if (gr >= 0x7fffffffL) return false;
    return true;
}

}  // namespace

// The grouped filter gradient (include/confignet_hip.h).  Checks everything, then launches: a refused list has enqueued nothing.
extern "C" int cn_conv_wgrad_grouped(int njobs, const CnConvGeom* geoms, const float* const* x, const float* const* gy, float* const* out,
                                     float* const* ws, const size_t* ws_bytes, const int* accumulate, int solo, int* parts, void* stream) {
    CN_CHECK_ARG(njobs >= 0 && (njobs == 0 || (geoms && x && gy && out && accumulate && parts)), "cn_conv_wgrad_grouped: bad arguments");
    for (int j = 0; j < njobs; ++j) {
        if (int e = check_geom(geoms + j)) return e;
        CN_CHECK_ARG(x[j] && gy[j] && out[j], "cn_conv_wgrad_grouped: job %d has a NULL tensor", j);
    }
    std::vector<WgGroupJob> jobs;
    std::vector<long> grids;
    if (!plan_conv_wgrad_group(njobs, geoms, solo != 0, jobs, grids)) {
        cn_set_error("cn_conv_wgrad_grouped: a job the LDS-DMA filter-gradient kernel does not take");
        return CN_EUNSUPPORTED;
    }
    for (int j = 0; j < njobs; ++j)
        CN_CHECK_ARG(jobs[j].ws_floats == 0 || (ws && ws_bytes && ws[j] && ws_bytes[j] >= sizeof(float) * jobs[j].ws_floats),
                     "cn_conv_wgrad_grouped: job %d needs a workspace of %zu bytes", j, sizeof(float) * jobs[j].ws_floats);
    const hipStream_t s = (hipStream_t)stream;
    std::vector<int> order(njobs);
    for (int j = 0; j < njobs; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return jobs[a].blk0 < jobs[b].blk0; });
    for (int l = 0; l < (int)grids.size(); ++l) {
        Wg2Jobs J{};
        int n = 0, cfg = -1;
        double flops = 0.0, bytes = 0.0;
        for (int j : order) {                   // (in the order of their first workgroups)
            const WgGroupJob& q = jobs[j];
            if (q.launch != l) continue;
            const CnConvGeom& g = geoms[j];
            const long count = (long)g.k_d * g.k_h * g.k_w * g.cin * g.cout;
            Wg2Job& o = J.job[n];
            o.g = g;
            o.rows = (int)q.rows; o.tiles_x = q.tx; o.tiles_y = q.ty; o.nsplits = (int)q.splits; o.accumulate = accumulate[j] ? 1 : 0;
            o.x = x[j]; o.gy = gy[j];
            o.out = q.splits > 1 ? ws[j] : out[j];
            o.slab_stride = q.splits > 1 ? count : 0;
            J.blk0[n++] = (int)q.blk0;
            cfg = q.cfg;
            flops += conv_flops(g);
            bytes += conv_bytes(g, 4.0, 4.0, 4.0);
            parts[j] = q.splits > 1 ? (int)q.splits : 0;
        }
        J.blk0[n] = (int)grids[l];
        J.n = n;
        cn_prof_begin(s, flops, bytes, wgrad_family(cfg));
        cn_wgrad2_grouped(cfg, J, (unsigned)grids[l], s);
        cn_prof_end(s);
        CN_LAUNCH_CHECK();
    }
    return CN_OK;
}

// Diagnostic: the plan cn_conv_wgrad_grouped WOULD follow -- needs no device, enqueues nothing.
extern "C" int cn_conv_wgrad_grouped_plan(int njobs, const CnConvGeom* geoms, int solo, long long* out, long long info[4]) {
    CN_CHECK_ARG(njobs >= 0 && (njobs == 0 || (geoms && out)) && info, "cn_conv_wgrad_grouped_plan: bad arguments");
    for (int j = 0; j < njobs; ++j)
        if (int e = check_geom(geoms + j)) return e;
    std::vector<WgGroupJob> jobs;
    std::vector<long> grids;
    info[0] = 0; info[1] = CN_WG2_GROUP; info[2] = (long long)sizeof(Wg2Jobs); info[3] = CN_KERNARG_BYTES;
    if (!plan_conv_wgrad_group(njobs, geoms, solo != 0, jobs, grids)) {
        cn_set_error("cn_conv_wgrad_grouped: a job the LDS-DMA filter-gradient kernel does not take");
        return CN_EUNSUPPORTED;
    }
    info[0] = (long long)grids.size();
    for (int j = 0; j < njobs; ++j) {
        const WgGroupJob& q = jobs[j];
        const long long v[10] = {q.cfg, q.stages, q.splits, q.rows, q.tx, q.ty, q.blk0, q.wgs, q.launch, (long long)q.ws_floats};
        for (int i = 0; i < 10; ++i) out[10 * j + i] = v[i];
    }
    return CN_OK;
}

// Tuning hook of the forward / data-gradient main loop (include/confignet_hip.h): loop = 1 / 0 forces the LDS-DMA loop on / off for
// the layers it can take, kb / ns / np its stage depth, stage count and loader waves.  Process-wide; not for production use.
extern "C" int cn_conv_loop_select(int loop, int kb, int ns, int np) {
    CN_CHECK_ARG(loop >= -1 && loop <= 1 && (kb == 0 || kb == 16 || kb == 32) && (ns == 0 || ns == 3 || ns == 4) && np >= -1 && np <= 2,
                 "cn_conv_loop_select: bad argument");
    g_fwd2_sel = loop;
    cn_fwd2_tune(kb, ns, np);
    g_tune_wg2_ns = ns;
    return CN_OK;
}

// Tuning hook (scripts/conv_sweep.py): force the tile configuration (0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 128x32, 4 = 128x96;
// -1 = heuristic), the split-K factor of cn_conv_fwd / cn_conv_dgrad (0 = heuristic) and the workgroup target of the filter gradient
// (0 = default).  Of the filter-gradient kernels the LDS-DMA one takes the tile (0 / 4 / 2 / 3, 5 = 256x64) and the target, the atomic
// one the target (plan_conv_wgrad).  Process-wide; not for production use.
extern "C" int cn_conv_tune(int cfg, int splits, long wg_blocks) {
    g_tune_cfg = cfg;
    g_tune_splits = splits;
    g_tune_wg_blocks = wg_blocks;
    return CN_OK;
}
