// depthwise.hip -- the kernels of the CelebA attribute classifier (metrics/mobilenet_v2.py) that no other file covers:
// the depthwise 3x3 convolution of keras MobileNetV2 (DepthwiseConv2D, depth_multiplier 1, with the folded BatchNormalization
// as a per-channel bias and ReLU6 in the epilogue) and the one-pass image preprocessing in front of it (cv2.resize INTER_LINEAR +
// keras.applications.mobilenet_v2.preprocess_input); for training, the depthwise convolution's input and filter gradients.
#include <type_traits>
#include "chan_slices.h"

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

// The geometry of one call by the padding rule above: output extents and low pads (the three launchers and the slices query).
struct DwGeom {
    int n, h, wd, c, oh, ow, ph, pw;
};

DwGeom dw_geom(int n, int h, int wd, int c, int stride) {
    const int oh = (h + stride - 1) / stride, ow = (wd + stride - 1) / stride;
    return {n, h, wd, c, oh, ow, ((oh - 1) * stride + 3 - h) / 2, ((ow - 1) * stride + 3 - wd) / 2};     // total >= 1 for k = 3, s <= 2
}

// f(S, V) as compile-time constants for stride 1 / 2 and 4 channels per lane or 1: the one place an entry point's (stride, vector
// width) becomes an instantiation.
template <int I>
using Int = std::integral_constant<int, I>;

template <typename F>
int dw_instance(int stride, bool v4, F f) {
    if (stride == 1) return v4 ? f(Int<1>{}, Int<4>{}) : f(Int<1>{}, Int<1>{});
    return v4 ? f(Int<2>{}, Int<4>{}) : f(Int<2>{}, Int<1>{});
}

template <int S, int V, int OPX, int OPY>
int launch_dw(const DwGeom& g, const float* x, const float* w, const float* bias, float* y, int act, float slope, hipStream_t s) {
    const int nxb = cn_cdiv(g.ow, OPX), nyb = cn_cdiv(g.oh, OPY);
    const long total = (long)g.n * nyb * nxb * (g.c / V);
    const int threads = 256;
    const long blocks = (total + threads - 1) / threads;
    CN_CHECK_ARG(blocks < 0x7fffffffL, "cn_dwconv3x3_fwd: tensor too large");
    hipLaunchKernelGGL((dwconv3x3_kernel<S, V, OPX, OPY>), dim3((unsigned)blocks), dim3(threads), 0, s, x, w, bias, y, g.h, g.wd, g.c, g.oh,
                       g.ow, g.ph, g.pw, nxb, nyb, total, act, slope);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

// ---- depthwise 3x3: input gradient -------------------------------------------------------------------------------------------
// gx[b, iy, ix, ch] = sum_{ky, kx} gy[b, oy, ox, ch] w[ky, kx, ch] over the (oy, ox) with oy S - ph + ky = iy: a gather over gy with
// the forward's work split (a lane owns V channels and an IPY x IPX block of INPUT pixels, the taps in registers, every gy row
// of the block loaded once).  In padded coordinates u = iy + ph the tap is ky = u - oy S; a block starts at a multiple of S there
// (at stride 2 the first block of an odd extent begins one pixel outside the image), so the parity of u -- which decides whether
// the taps {0, 2} or the tap {1} contribute at stride 2 -- is the parity of the position inside the block and every ky / kx test
// below folds at compile time: with oy = u0 / S - 2 / S + rr, ky = i + 2 - S rr for position i and gy row rr.
// 24 float4 loads for 8 gradients at stride 1, 6 for 8 at stride 2.
template <int S, int V, int IPX, int IPY>
__global__ __launch_bounds__(256) void dwconv3x3_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                              float* __restrict__ gx, int h, int wd, int c, int oh, int ow, int ph, int pw,
                                                              int nxb, int nyb, long total) {
    static_assert(IPX % S == 0 && IPY % S == 0, "a block starts at a multiple of the stride");
    constexpr int LO = 2 / S;                       // gy rows before u0 / S that reach into the block
    constexpr int NC = (IPX - 1) / S + LO + 1;      // gy columns of one row of the block
    constexpr int NR = (IPY - 1) / S + LO + 1;      // gy rows of the block
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
    const int u0 = yb * IPY + (S == 1 ? ph : 0), v0 = xb * IPX + (S == 1 ? pw : 0);     // padded coordinates of the block
    const int iy0 = u0 - ph, ix0 = v0 - pw;
    const int oyb = u0 / S - LO, oxb = v0 / S - LO;

    float wt[9][V];
#pragma unroll
    for (int k = 0; k < 9; ++k) VecIO<V>::ld(w + (long)k * c + ch, wt[k]);
    float acc[IPY][IPX][V];
#pragma unroll
    for (int i = 0; i < IPY; ++i)
#pragma unroll
        for (int j = 0; j < IPX; ++j)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[i][j][v] = 0.f;

    const float* gb_ = gy + (long)b * oh * ow * c + ch;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        const int oy = oyb + rr;
        if (oy < 0 || oy >= oh) continue;
        float col[NC][V];
        const float* row = gb_ + (long)oy * ow * c;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int ox = oxb + q;
            if (ox >= 0 && ox < ow) {
                VecIO<V>::ld(row + (long)ox * c, col[q]);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) col[q][v] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < IPY; ++i) {
            const int ky = i + 2 - S * rr;             // (compile-time after unrolling, as kx below)
            if (ky < 0 || ky > 2) continue;
#pragma unroll
            for (int j = 0; j < IPX; ++j)
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const int kx = j + 2 - S * q;
                    if (kx < 0 || kx > 2) continue;
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[i][j][v] = fmaf(col[q][v], wt[ky * 3 + kx][v], acc[i][j][v]);
                }
        }
    }

    float* xb_ = gx + (long)b * h * wd * c + ch;
#pragma unroll
    for (int i = 0; i < IPY; ++i) {
        const int iy = iy0 + i;
        if (iy < 0 || iy >= h) continue;
#pragma unroll
        for (int j = 0; j < IPX; ++j) {
            const int ix = ix0 + j;
            if (ix < 0 || ix >= wd) continue;
            VecIO<V>::st(xb_ + ((long)iy * wd + ix) * c, acc[i][j]);
        }
    }
}

template <int S, int V, int IPX, int IPY>
int launch_dw_dgrad(const DwGeom& g, const float* gy, const float* w, float* gx, hipStream_t s) {
    const int nxb = cn_cdiv(g.wd + (S == 1 ? 0 : g.pw), IPX), nyb = cn_cdiv(g.h + (S == 1 ? 0 : g.ph), IPY);
    const long total = (long)g.n * nyb * nxb * (g.c / V);
    const long blocks = (total + 255) / 256;
    CN_CHECK_ARG(blocks < 0x7fffffffL, "cn_dwconv3x3_dgrad: tensor too large");
    hipLaunchKernelGGL((dwconv3x3_dgrad_kernel<S, V, IPX, IPY>), dim3((unsigned)blocks), dim3(256), 0, s, gy, w, gx, g.h, g.wd, g.c, g.oh,
                       g.ow, g.ph, g.pw, nxb, nyb, total);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

// ---- depthwise 3x3: filter gradient ------------------------------------------------------------------------------------------
// gw[ky, kx, ch] = sum_{b, oy, ox} gy[b, oy, ox, ch] x[b, oy S - ph + ky, ox S - pw + kx, ch]: N OH OW terms into 9 C numbers, as a
// per-channel reduction over slices of the output pixels (chan_slices.h: the work split, the slice rule with a floor of 64 pixels
// per slice, the lane combine): a lane keeps 9 x V accumulators, the workgroup leaves 9 x C partials, no atomics anywhere.
constexpr long DW_WGRAD_MIN_ROWS = 64;

template <int S, int V>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                              float* __restrict__ part, int h, int wd, int c, int oh, int ow, int ph, int pw,
                                                              int pixels, int per_slice, int TX, int TY) {
    __shared__ float red[9 * 256 * V];
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
    const int cg = blockIdx.x * TX + tx;
    const int ch = cg * V;
    float acc[9][V];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[k][v] = 0.f;
    if (ch < c) {
        const int p0 = blockIdx.y * per_slice, p1 = min(pixels, p0 + per_slice);
        for (int p = p0 + ty; p < p1; p += TY) {
            const int ox = p % ow, q = p / ow;
            const int oy = q % oh, b = q / oh;
            float g[V];
            VecIO<V>::ld(gy + (long)p * c + ch, g);
            const int iy0 = oy * S - ph, ix0 = ox * S - pw;
            const float* xb_ = x + (long)b * h * wd * c + ch;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = iy0 + ky;
                if (iy < 0 || iy >= h) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ix0 + kx;
                    if (ix < 0 || ix >= wd) continue;
                    float xv[V];
                    VecIO<V>::ld(xb_ + ((long)iy * wd + ix) * c, xv);
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[ky * 3 + kx][v] = fmaf(g[v], xv[v], acc[ky * 3 + kx][v]);
                }
            }
        }
    }
    chan_lanes_sum<9, V>(acc, red, part, c, TX, TY);
}

template <int S, int V>
int launch_dw_wgrad(const DwGeom& g, const float* x, const float* gy, float* part, int slices, hipStream_t s) {
    const long pixels = (long)g.n * g.oh * g.ow;
    CN_CHECK_ARG(pixels < 0x7fffffffL, "cn_dwconv3x3_wgrad: tensor too large");       // (so the plan's per_slice fits the kernel's int)
    const ChanSlicesPlan p = chan_slices_plan(pixels, g.c / V, DW_WGRAD_MIN_ROWS);
    CN_CHECK_ARG(slices == p.slices, "cn_dwconv3x3_wgrad: %d slices given, the plan has %d (cn_dwconv3x3_wgrad_slices)", slices, p.slices);
    hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<S, V>), dim3(p.cb, p.slices), dim3(256), 0, s, x, gy, part, g.h, g.wd, g.c, g.oh, g.ow, g.ph,
                       g.pw, (int)pixels, (int)p.per_slice, p.TX, p.TY);
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
    const DwGeom g = dw_geom(n, h, wd, c, stride);
    // operands that are not 16-byte aligned take the scalar walk (a NULL bias counts as aligned); 4 x 2 outputs per lane at stride 1, 2 x 2 at 2
    return dw_instance(stride, c % 4 == 0 && aligned16(x, w, y, bias), [&](auto S, auto V) {
        return launch_dw<S.value, V.value, S.value == 1 ? 4 : 2, 2>(g, x, w, bias, y, act, slope, s);
    });
}

extern "C" int cn_dwconv3x3_dgrad(const float* gy, const float* w, float* gx, int n, int h, int wd, int c, int stride, void* stream) {
    CN_CHECK_ARG(gy && w && gx, "cn_dwconv3x3_dgrad: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0, "cn_dwconv3x3_dgrad: bad extents n %d h %d w %d c %d", n, h, wd, c);
    CN_CHECK_ARG(stride == 1 || stride == 2, "cn_dwconv3x3_dgrad: stride must be 1 or 2 (got %d)", stride);
    hipStream_t s = (hipStream_t)stream;
    const DwGeom g = dw_geom(n, h, wd, c, stride);
    return dw_instance(stride, c % 4 == 0 && aligned16(gy, w, gx), [&](auto S, auto V) {      // (misaligned: the scalar walk, as the forward)
        return launch_dw_dgrad<S.value, V.value, 4, 2>(g, gy, w, gx, s);
    });
}

extern "C" int cn_dwconv3x3_wgrad_slices(int n, int h, int wd, int c, int stride) {
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0 && (stride == 1 || stride == 2), "cn_dwconv3x3_wgrad_slices: bad extents");
    const DwGeom g = dw_geom(n, h, wd, c, stride);
    return chan_slices_plan((long)n * g.oh * g.ow, c % 4 == 0 ? c / 4 : c, DW_WGRAD_MIN_ROWS).slices;
}

extern "C" int cn_dwconv3x3_wgrad(const float* x, const float* gy, float* part, int slices, int n, int h, int wd, int c, int stride,
                                  void* stream) {
    CN_CHECK_ARG(x && gy && part, "cn_dwconv3x3_wgrad: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0, "cn_dwconv3x3_wgrad: bad extents n %d h %d w %d c %d", n, h, wd, c);
    CN_CHECK_ARG(stride == 1 || stride == 2, "cn_dwconv3x3_wgrad: stride must be 1 or 2 (got %d)", stride);
    hipStream_t s = (hipStream_t)stream;
    // Unlike the forward and the input gradient, misaligned operands are refused, not walked as scalars: the slice plan -- and with it
    // the count the caller sized `part` by, cn_dwconv3x3_wgrad_slices -- follows c alone, so the float4 walk is not optional here.
    CN_CHECK_ARG(c % 4 != 0 || aligned16(x, gy), "cn_dwconv3x3_wgrad: x and gy must be 16-byte aligned when c %% 4 == 0");
    const DwGeom g = dw_geom(n, h, wd, c, stride);
    return dw_instance(stride, c % 4 == 0, [&](auto S, auto V) { return launch_dw_wgrad<S.value, V.value>(g, x, gy, part, slices, s); });
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
