// common.h -- shared helpers of libconfignet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/confignet_hip.h"

void cn_set_error(const char* fmt, ...);

#define CN_CHECK_ARG(cond, ...)            \
    do {                                   \
        if (!(cond)) {                     \
            cn_set_error(__VA_ARGS__);     \
            return CN_EINVAL;              \
        }                                  \
    } while (0)

#define CN_HIP(expr)                                                              \
    do {                                                                          \
        hipError_t e__ = (expr);                                                  \
        if (e__ != hipSuccess) {                                                  \
            cn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return CN_EHIP;                                                       \
        }                                                                         \
    } while (0)

#define CN_LAUNCH_CHECK()                                                         \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            cn_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
            return CN_EHIP;                                                       \
        }                                                                         \
    } while (0)

// Zero `bytes` (multiple of 4) bytes at p with an ordinary kernel.  hipMemsetAsync nodes were observed NOT to
// re-execute on HIP-graph replay (ROCm 7.2, gfx950: accumulators kept growing across replays), so every
// accumulate-into buffer is cleared by a kernel node instead.
int cn_zero_async(void* p, size_t bytes, hipStream_t s);

// Deterministic mode (cn_set_deterministic, prof.hip): reductions in a fixed order instead of fp32 atomics.  Kernels that
// need room for their partial results take it from a per-stream workspace (allocated when the mode is switched on).
int cn_det();
float* cn_det_ws(hipStream_t s, size_t need_floats);     // NULL (+ error string) if the request does not fit
constexpr size_t CN_DET_WS_FLOATS = (size_t)16 << 20;     // 64 MiB per stream, 16 streams (prof.hip: CN_DET_SLOTS; 1 GiB, allocated when the mode is first switched on)
// dst[i] (+)= scale * sum_{p < parts} src[p * count + i], parts added in index order (one thread per i)
int cn_sum_parts(const float* src, float* dst, int parts, long count, int accumulate, float scale, hipStream_t s);

// fwd2.hip: C[M][N] (+)= A[M][K] B for the 1x1 stride-1 convolutions (gp = NULL) and, with a geometry, the same main loop over the
// gathered rows of a vec convolution (par: parity-ordered rows); tile cfg 0 / 1 / 2 / 3 / 4 of the implicit-GEMM numbering, bt = B is the
// original filter [N][K] (data gradient), the split-K protocol of igemm_fwd_kernel; both operands go straight into LDS (LDS-DMA), NS
// stages deep; x_elems / w_elems size the buffer descriptors; CN_EUNSUPPORTED for anything it does not take.
// mask (shaped like C) / colsum / colsum2: the consumer's ReLU backward and its column sums in the epilogue of an unsplit bt launch
// (cn_conv_dgrad_w_mask); cn_fwd2_takes_mask says which launches carry it
int cn_fwd2(const CnConvGeom* gp, int cfg, int bt, const float* A, const float* B, const float* bias, float* C, long M, int N, int K,
            int act, float slope, int splits, long part_stride, int par, hipStream_t s, const float* res, double x_elems, double w_elems,
            float* stats = nullptr, int stats_mode = 0, float stats_slope = 0.f, int srows = 1, int sper = 1, const float* mask = nullptr,
            float* colsum = nullptr, float* colsum2 = nullptr);
bool cn_fwd2_takes_mask(int cfg, int bt, int gathered, int n, int has_bias, int act, int has_stats);
void cn_fwd2_tune(int kb, int ns, int np);
void cn_fwd2_grid(int cfg, long M, int N, int par, int splits, int grid[3]);      // the launch grid cn_fwd2 uses
// igemm_conv.hip: the register-staged implicit-GEMM loop on tile cfg (anything but 0 / 1 / 3 / 4: 64 x 64), the same split-K protocol;
// cn_igemm_fwd_thin: its 128 x 32 tile with guarded filter loads for parity-ordered data gradients into a thin (cout <= 4) image
int cn_igemm_fwd(int cfg, const CnConvGeom& g, bool vec, int par, int splits, const float* x, const float* w, const float* bias, float* y,
                 int act, float slope, hipStream_t s, int bt, long part_stride, const float* res);
void cn_igemm_fwd_grid(int cfg, const CnConvGeom& g, bool vec, int par, int splits, int grid[3]);
int cn_igemm_fwd_thin(const CnConvGeom& g, const float* x, const float* w, const float* bias, float* y, int act, float slope, hipStream_t s);
// Which launch a forward / data-gradient convolution gets (conv_dispatch.hip: plan_conv_fwd; the numbers are what cn_conv_fwd_plan
// reports).  small_conv.hip launches everything before CN_ROUTE_FWD2 except CN_ROUTE_THIN_PAR_IGEMM.
enum ConvRoute { CN_ROUTE_UP2K4_RGB = 0, CN_ROUTE_S2_IMAGE_DGRAD, CN_ROUTE_S1_IMAGE_DGRAD, CN_ROUTE_THIN_PAR_IGEMM, CN_ROUTE_THIN_COOP,
                 CN_ROUTE_THIN, CN_ROUTE_C3, CN_ROUTE_C7S2, CN_ROUTE_FWD2, CN_ROUTE_IGEMM, CN_ROUTE_UNSUPPORTED };
constexpr int CN_THIN_COOP_PX = 4;        // output pixels per thread of thin_conv_coop_kernel
void cn_small_conv(int route, unsigned grid_x, const CnConvGeom& g, bool vec, int par, const void* x, int x_dt, const float* w,
                   const float* bias, void* y, int y_dt, int act, float slope, hipStream_t s);
int cn_fwd2_bf16(const CnConvGeom& g, int cfg, int flip, const void* x, const void* wb, const float* bias, void* y, int act, float slope,
                 int par, hipStream_t s);

// Which launch a filter gradient gets (conv_dispatch.hip: plan_conv_wgrad; the numbers are what cn_conv_wgrad_plan reports): the
// K = 27 first layers (c3_wgrad.hip), thin outputs (thin_wgrad.hip), the from-RGB 1x1 shapes and the atomic row-split kernel
// (igemm_conv.hip), the LDS-DMA kernel (wgrad2.hip), the bf16 kernel (igemm_bf16.hip).  The functions below launch ONE instantiation
// with the plan's numbers and decide nothing.
enum WgradRoute { CN_WG_C3 = 0, CN_WG_THIN, CN_WG_TINY, CN_WG_WGRAD2, CN_WG_IGEMM, CN_WG_BF16, CN_WG_NONE };
constexpr int CN_C3_WGRAD_TILE = 64, CN_C3_WGRAD_PARTS = 512;                          // output pixels of a tile; workgroups = partial filters
constexpr int CN_THIN_WGRAD_TH = 8, CN_THIN_WGRAD_TW = 32, CN_THIN_WGRAD_PARTS = 512;  // output pixels of a tile; most workgroups = partial filters
struct Wg2Plan {
    int cfg;          // implicit-GEMM numbering: 0 = 128x128, 4 = 128x96, 2 = 64x64, 3 = 128x32, 5 = 256x64
    long tiles_x, tiles_y, splits, rows;
};
bool cn_wgrad2_ok(const CnConvGeom& g);
Wg2Plan cn_wgrad2_plan(const CnConvGeom& g, int forced_cfg, long wg_target, bool group = false);
void cn_wgrad2(int cfg, int ns, const CnConvGeom& g, const float* x, const float* gy, float* out, long slab_stride, int rows, int tiles_x,
               int tiles_y, int splits, int accumulate, unsigned grid, hipStream_t s);
// A grouped launch of the LDS-DMA kernel: jobs of one tile configuration, by value in the kernel arguments (< 4 KB)
constexpr int CN_WG2_GROUP = 24, CN_KERNARG_BYTES = 4096;
struct Wg2Job {
    CnConvGeom g;
    int rows, tiles_x, tiles_y, nsplits, accumulate;
    const float* x;
    const float* gy;
    float* out;            // the filter gradient, or with slab_stride != 0 the slabs
    long slab_stride;
};
struct Wg2Jobs {
    Wg2Job job[CN_WG2_GROUP];
    int blk0[CN_WG2_GROUP + 1];       // first workgroup of job j
    int n;
};
static_assert(sizeof(Wg2Jobs) <= CN_KERNARG_BYTES, "the jobs of a grouped launch travel in its kernel arguments");
void cn_wgrad2_grouped(int cfg, const Wg2Jobs& J, unsigned grid, hipStream_t s);
void cn_igemm_wgrad(int cfg, const CnConvGeom& g, const float* x, const float* gy, float* gw, int rows, float* parts, int tx, int ty,
                    int splits, dim3 grid, hipStream_t s);
int cn_tiny_wgrad(const CnConvGeom& g, const float* x, const float* gy, float* gw, int blocks, float* parts, hipStream_t s);
void cn_bf16_wgrad(int cfg, const CnConvGeom& g, const void* x, const void* gy, float* gw, int rows, float* parts, int tx, int ty, int splits,
                   dim3 grid, hipStream_t s);
int cn_c3_wgrad(const CnConvGeom& g, const float* x, const void* gy, int gy_dt, float* scratch, int tiles_x, int ntiles, int nparts,
                size_t lds, hipStream_t s);
void cn_c3_wgrad_reduce(const float* scratch, float* gw, int nparts, int count, int accumulate, hipStream_t s);
void cn_thin_wgrad(const CnConvGeom& g, const float* x, const float* gy, float* scratch, int nwg, size_t lds, int tiles_y, int tiles_x,
                   int ntiles, hipStream_t s);

// profiling hooks (prof.hip): bracket one launch of the dominant kernel class
// family: which kernel of the class is launched (cn_prof_collect_by_family); bytes: the launch's algorithmic HBM bytes
enum { CN_FAM_FWD_128x128 = 0, CN_FAM_FWD_128x64, CN_FAM_FWD_64x64, CN_FAM_FWD_128x32, CN_FAM_FWD_128x96, CN_FAM_WGRAD_128x128,
       CN_FAM_WGRAD_128x96, CN_FAM_WGRAD_64x64, CN_FAM_WGRAD_128x32, CN_FAM_WINO, CN_FAM_C3_FWD, CN_FAM_S2_IMAGE_DGRAD,
       CN_FAM_THIN, CN_FAM_C3_WGRAD, CN_FAM_BF16_FWD, CN_FAM_BF16_WGRAD, CN_FAM_WGRAD_256x64, CN_FAM_WGRAD_SLAB_SUM };
void cn_prof_begin(hipStream_t s, double flops, double bytes = 0.0, int family = 31);
void cn_prof_end(hipStream_t s);

// q = m / d, r = m % d for m >= 0, d > 0.  The extents of this path are powers of two almost everywhere (256 / 128 / ... / 4 pixels,
// 2 x 2 parity classes): a shift and a mask behind a wave-uniform test instead of the ~40-instruction software division (the target
// has no integer divide) -- a workgroup's prologue decodes its rows with 3 - 11 of them per row.
__device__ __forceinline__ void divmod_pos(int m, int d, int& q, int& r) {
    if ((d & (d - 1)) == 0) {
        q = m >> (__builtin_ctz(d));
        r = m & (d - 1);
    } else {
        q = m / d;
        r = m - q * d;
    }
}

__device__ __forceinline__ float cn_apply_act(float v, int act, float slope) {
    switch (act) {
        case CN_ACT_LRELU: return v > 0.f ? v : v * slope;
        case CN_ACT_RELU: return v > 0.f ? v : 0.f;
        case CN_ACT_TANH: return tanhf(v);
        default: break;
    }
    // the classifier's codes (CN_ACT_RELU6, CN_ACT_SIGMOID) behind the original three: the dispatch of those stays as it was
    if (act == CN_ACT_RELU6) return fminf(fmaxf(v, 0.f), 6.f);
    if (act == CN_ACT_SIGMOID) return __fdividef(1.f, 1.f + __expf(-v));        // (native exp / rcp: rel. error ~1e-6)
    return v;
}

// derivative of an activation evaluated from its OUTPUT o
__device__ __forceinline__ float act_deriv(float o, int act, float slope) {
    if (act == CN_ACT_LRELU) return o > 0.f ? 1.f : slope;
    if (act == CN_ACT_RELU) return o > 0.f ? 1.f : 0.f;
    if (act == CN_ACT_TANH) return 1.f - o * o;
    return 1.f;
}

static inline int cn_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// compute units of the current device (hipDeviceAttributeMultiprocessorCount, read once; 256 on an MI355X): the launch cost models
// count workgroup rounds with it
int cn_cu_count();
