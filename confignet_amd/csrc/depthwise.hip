// depthwise.hip -- the two kernels of the CelebA attribute classifier (metrics/mobilenet_v2.py) that no other file covers:
// the depthwise 3x3 convolution of keras MobileNetV2 (DepthwiseConv2D, depth_multiplier 1, with the folded BatchNormalization
// as a per-channel bias and ReLU6 in the epilogue) and the one-pass image preprocessing in front of it (cv2.resize INTER_LINEAR +
// keras.applications.mobilenet_v2.preprocess_input).
#include "common.h"

namespace {

// ---- depthwise 3x3 ----------------------------------------------------------------------------------------------------------
// Padding.  Keras MobileNetV2 pads a stride-2 depthwise layer with ZeroPadding2D(correct_pad(x, 3)) and convolves VALID;
// correct_pad(k = 3) = ((1 - adj_h, 1), (1 - adj_w, 1)) with adj = 1 for an even extent, 0 for an odd one.  TF "same" (the
// stride-1 layers) pads total = max((ceil(e / s) - 1) s + 3 - e, 0), low side total // 2:
//   s = 1:          total = 2                       -> (1, 1)
//   s = 2, e even:  total = (e/2 - 1) 2 + 3 - e = 1  -> (0, 1)  = correct_pad (1 - 1, 1)
//   s = 2, e odd:   total = ((e+1)/2 - 1) 2 + 3 - e = 2 -> (1, 1) = correct_pad (1 - 0, 1)
// and the VALID output of the padded extent, (e + lo + 1 - 3) / 2 + 1, is ceil(e / 2) in both cases: one rule serves both
// layer kinds, with the low pad p below and the high side implied by the bounds test.
//
// Work split.  Memory bound (2 * 9 flops per 8 bytes of the smallest tensor): a lane owns V consecutive channels (V = 4: one
// float4, lanes of a wave on consecutive channel groups -> coalesced NHWC rows) and an OPY x OPX block of output pixels.  The
// 9 taps of its channels sit in registers; each input row it needs ((OPY - 1) S + 3 of them) is loaded ONCE, (OPX - 1) S + 3
// pixels wide, and feeds every output row / column of the block that reads it -- 24 float4 loads for 8 outputs at stride 1
// (instead of 72), 25 for 4 at stride 2 (instead of 36).
template <int V>
struct VecIO;
template <>
struct VecIO<4> {
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <>
struct VecIO<1> {
    static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = *p; }
    static __device__ __forceinline__ void st(float* p, const float* v) { *p = v[0]; }
};

template <int S, int V, int OPX, int OPY>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int h, int wd, int c,
                                                        int oh, int ow, int ph, int pw, int nxb, int nyb, long total, int act, float slope) {
    constexpr int NC = (OPX - 1) * S + 3;          // input columns of one row of the block
    constexpr int NR = (OPY - 1) * S + 3;          // input rows of the block
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cgs = c / V;
    const int cg = (int)(t % cgs);
    long r = t / cgs;
    const int xb = (int)(r % nxb);
    r /= nxb;
    const int yb = (int)(r % nyb);
    const int b = (int)(r / nyb);
    const int ch = cg * V;
    const int oy0 = yb * OPY, ox0 = xb * OPX;
    const int iy0 = oy0 * S - ph, ix0 = ox0 * S - pw;

    float wt[9][V];
#pragma unroll
    for (int k = 0; k < 9; ++k) VecIO<V>::ld(w + (long)k * c + ch, wt[k]);
    float acc[OPY][OPX][V];
#pragma unroll
    for (int i = 0; i < OPY; ++i)
#pragma unroll
        for (int j = 0; j < OPX; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[i][j][v] = 0.f;

    const float* xb_ = x + (long)b * h * wd * c + ch;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        const int iy = iy0 + rr;
        if (iy < 0 || iy >= h) continue;            // zero padding rows (uniform per block row)
        float col[NC][V];
        const float* row = xb_ + (long)iy * wd * c;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int ix = ix0 + q;
            if (ix >= 0 && ix < wd) {
                VecIO<V>::ld(row + (long)ix * c, col[q]);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) col[q][v] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < OPY; ++i) {
            const int ky = rr - i * S;                 // the filter row this input row is for output row i
            if (ky < 0 || ky > 2) continue;            // (compile-time after unrolling)
#pragma unroll
            for (int j = 0; j < OPX; ++j)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[i][j][v] = fmaf(col[j * S + kx][v], wt[ky * 3 + kx][v], acc[i][j][v]);
        }
    }

    float bv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) bv[v] = 0.f;
    if (bias) VecIO<V>::ld(bias + ch, bv);
    float* yb_ = y + (long)b * oh * ow * c + ch;
#pragma unroll
    for (int i = 0; i < OPY; ++i) {
        const int oy = oy0 + i;
        if (oy >= oh) break;
#pragma unroll
        for (int j = 0; j < OPX; ++j) {
            const int ox = ox0 + j;
            if (ox >= ow) break;
            float o[V];
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = cn_apply_act(acc[i][j][v] + bv[v], act, slope);
            VecIO<V>::st(yb_ + ((long)oy * ow + ox) * c, o);
        }
    }
}

template <int S, int V, int OPX, int OPY>
int launch_dw(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int c, int act, float slope,
              hipStream_t s) {
    const int oh = (h + S - 1) / S, ow = (wd + S - 1) / S;
    const int ph = ((oh - 1) * S + 3 - h) / 2, pw = ((ow - 1) * S + 3 - wd) / 2;     // total >= 1 for k = 3, s <= 2
    const int nxb = cn_cdiv(ow, OPX), nyb = cn_cdiv(oh, OPY);
    const long total = (long)n * nyb * nxb * (c / V);
    const int threads = 256;
    const long blocks = (total + threads - 1) / threads;
    CN_CHECK_ARG(blocks < 0x7fffffffL, "cn_dwconv3x3_fwd: tensor too large");
    hipLaunchKernelGGL((dwconv3x3_kernel<S, V, OPX, OPY>), dim3((unsigned)blocks), dim3(threads), 0, s, x, w, bias, y, h, wd, c, oh, ow,
                       ph, pw, nxb, nyb, total, act, slope);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

// ---- image preprocessing ---------------------------------------------------------------------------------------------------------
// y[b, oy, ox, ch] = bilinear(x)[...] / 127.5 - 1 with cv2's INTER_LINEAR sampling: source coordinate (o + 0.5) * in / out - 0.5,
// clamped to [0, in - 1] (half-pixel centres, edge replication); each source value first mapped v * in_mul + in_add.
// The source coordinate ((2 o + 1) in - out) / (2 out) as an exact integer quotient and remainder: its fraction carries no
// rounding of the coordinate (a float product (o + 0.5) * in / out - 0.5 near 255 keeps only ~1.5e-5 of it).
__device__ __forceinline__ void src_coord(int o, int in, int out, int& i0, float& frac) {
    const long num = (long)(2 * o + 1) * in - out, den = 2L * out;
    if (num <= 0) { i0 = 0; frac = 0.f; return; }                       // clamped at the low edge
    i0 = (int)(num / den);
    if (i0 >= in - 1) { i0 = in - 1; frac = 0.f; return; }              // clamped at the high edge
    frac = (float)(num - (long)i0 * den) / (float)den;
}

template <typename T>
__global__ __launch_bounds__(256) void image_preprocess_kernel(const T* __restrict__ x, float* __restrict__ y, int h, int wd, int c,
                                                               int oh, int ow, float in_mul, float in_add, long total) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int ch = (int)(t % c);
    long r = t / c;
    const int ox = (int)(r % ow);
    r /= ow;
    const int oy = (int)(r % oh);
    const int b = (int)(r / oh);
    int y0, x0;
    float ay, ax;
    src_coord(oy, h, oh, y0, ay);
    src_coord(ox, wd, ow, x0, ax);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, wd - 1);
    const T* xb = x + (long)b * h * wd * c + ch;
    const float v00 = (float)xb[((long)y0 * wd + x0) * c] * in_mul + in_add, v01 = (float)xb[((long)y0 * wd + x1) * c] * in_mul + in_add;
    const float v10 = (float)xb[((long)y1 * wd + x0) * c] * in_mul + in_add, v11 = (float)xb[((long)y1 * wd + x1) * c] * in_mul + in_add;
    const float top = v00 + (v01 - v00) * ax, bot = v10 + (v11 - v10) * ax;
    y[t] = (top + (bot - top) * ay) / 127.5f - 1.f;
}

}  // namespace

extern "C" int cn_dwconv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int c, int stride,
                                int act, float slope, void* stream) {
    CN_CHECK_ARG(x && w && y, "cn_dwconv3x3_fwd: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0, "cn_dwconv3x3_fwd: bad extents n %d h %d w %d c %d", n, h, wd, c);
    CN_CHECK_ARG(stride == 1 || stride == 2, "cn_dwconv3x3_fwd: stride must be 1 or 2 (got %d)", stride);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = c % 4 == 0 && ((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)bias) % 16 == 0;
    if (stride == 1)
        return v4 ? launch_dw<1, 4, 4, 2>(x, w, bias, y, n, h, wd, c, act, slope, s) : launch_dw<1, 1, 4, 2>(x, w, bias, y, n, h, wd, c, act, slope, s);
    return v4 ? launch_dw<2, 4, 2, 2>(x, w, bias, y, n, h, wd, c, act, slope, s) : launch_dw<2, 1, 2, 2>(x, w, bias, y, n, h, wd, c, act, slope, s);
}

extern "C" int cn_image_preprocess(const void* x, int x_dt, float* y, int n, int h, int wd, int c, int oh, int ow, float in_mul,
                                   float in_add, void* stream) {
    CN_CHECK_ARG(x && y, "cn_image_preprocess: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0 && oh > 0 && ow > 0, "cn_image_preprocess: bad extents");
    CN_CHECK_ARG(x_dt == CN_F32 || x_dt == CN_U8, "cn_image_preprocess: input must be CN_F32 or CN_U8 (got %d)", x_dt);
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)n * oh * ow * c;
    const long blocks = (total + 255) / 256;
    CN_CHECK_ARG(blocks < 0x7fffffffL, "cn_image_preprocess: tensor too large");
    if (x_dt == CN_U8)
        hipLaunchKernelGGL(image_preprocess_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)x, y, h, wd, c, oh, ow,
                           in_mul, in_add, total);
    else
        hipLaunchKernelGGL(image_preprocess_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)x, y, h, wd, c, oh, ow,
                           in_mul, in_add, total);
    CN_LAUNCH_CHECK();
    return CN_OK;
}
