// depthwise.hip -- the kernels of the CelebA attribute classifier (metrics/mobilenet_v2.py) that no other file covers:
// the depthwise 3x3 convolution of keras MobileNetV2 (DepthwiseConv2D, depth_multiplier 1, with the folded BatchNormalization
// as a per-channel bias and ReLU6 in the epilogue) and the one-pass image preprocessing in front of it (cv2.resize INTER_LINEAR +
// keras.applications.mobilenet_v2.preprocess_input); for training, the depthwise convolution's input and filter gradients.
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
int launch_dw_dgrad(const float* gy, const float* w, float* gx, int n, int h, int wd, int c, hipStream_t s) {
    const int oh = (h + S - 1) / S, ow = (wd + S - 1) / S;
    const int ph = ((oh - 1) * S + 3 - h) / 2, pw = ((ow - 1) * S + 3 - wd) / 2;
    const int nxb = cn_cdiv(wd + (S == 1 ? 0 : pw), IPX), nyb = cn_cdiv(h + (S == 1 ? 0 : ph), IPY);
    const long total = (long)n * nyb * nxb * (c / V);
    const long blocks = (total + 255) / 256;
    CN_CHECK_ARG(blocks < 0x7fffffffL, "cn_dwconv3x3_dgrad: tensor too large");
    hipLaunchKernelGGL((dwconv3x3_dgrad_kernel<S, V, IPX, IPY>), dim3((unsigned)blocks), dim3(256), 0, s, gy, w, gx, h, wd, c, oh, ow, ph,
                       pw, nxb, nyb, total);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

// ---- depthwise 3x3: filter gradient ------------------------------------------------------------------------------------------
// gw[ky, kx, ch] = sum_{b, oy, ox} gy[b, oy, ox, ch] x[b, oy S - ph + ky, ox S - pw + kx, ch]: N OH OW terms into 9 C numbers.
// 256 threads as TX channel groups x TY pixel lanes (TX = the channel groups rounded up to a power of two, 64 at most: lanes of a
// wave on consecutive channel groups, coalesced NHWC rows as in the forward); a workgroup owns a SLICE of consecutive output
// pixels, lane ty walks the pixels ty, ty + TY, ... of it with 9 x V accumulators in registers.  The TY lanes of a channel group
// then combine in LDS: every lane stores its accumulators as red[k][ty][tx] (consecutive lanes -> consecutive float4: ds_write_b128
// without bank conflicts), and after the barrier thread o sums the TY entries of output (k, channel) = o with consecutive threads on
// consecutive dwords (conflict-free again), in ty order.  The workgroup leaves 9 x C partials with plain stores; the caller adds
// the slices in slice order (cn_sum_rows_into, or the grouped reduction at the join of a backward pass).  No atomics anywhere: the
// result has the same bits in every mode.
// Slices (dw_wgrad_plan).  A slice costs 9 C floats written and read again next to 2 per_slice C floats of operands, so it holds at
// least 64 pixels (<= 7 % extra traffic) and at least 4 pixels per lane; as many slices as that allows, up to 1024 workgroups
// (4 per compute unit).  Batch 32: the 7 x 7 x 960 layer (1568 pixels, TX 64, TY 4, 4 channel blocks) gets 25 slices of 64 pixels,
// 100 workgroups of 16 pixels per lane; the 128 x 128 x 32 layer (524 288 pixels, TX 8, TY 32, one channel block) gets 1024 slices
// of 512 pixels.
struct DwWgradPlan {
    int TX, TY, cb, slices, per_slice;
};

DwWgradPlan dw_wgrad_plan(long pixels, int cgs) {
    DwWgradPlan p;
    p.TX = 1;
    while (p.TX < cgs && p.TX < 64) p.TX *= 2;
    p.TY = 256 / p.TX;
    p.cb = cn_cdiv(cgs, p.TX);
    const long min_px = 4L * p.TY > 64 ? 4L * p.TY : 64;
    long slices = (pixels + min_px - 1) / min_px;
    const long cap = 1024 / p.cb > 1 ? 1024 / p.cb : 1;
    if (slices > cap) slices = cap;
    p.per_slice = (int)((pixels + slices - 1) / slices);
    p.slices = (int)((pixels + p.per_slice - 1) / p.per_slice);
    return p;
}

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
#pragma unroll
    for (int k = 0; k < 9; ++k) VecIO<V>::st(red + ((long)k * 256 + threadIdx.x) * V, acc[k]);
    __syncthreads();
    const int W = TX * V;                              // channels of this workgroup
    for (int o = threadIdx.x; o < 9 * W; o += 256) {
        const int k = o / W, cl = o - k * W;
        float s = 0.f;
        for (int y = 0; y < TY; ++y) s += red[(k * TY + y) * W + cl];
        const int co = blockIdx.x * W + cl;
        if (co < c) part[((long)blockIdx.y * 9 + k) * c + co] = s;
    }
}

template <int S, int V>
int launch_dw_wgrad(const float* x, const float* gy, float* part, int slices, int n, int h, int wd, int c, hipStream_t s) {
    const int oh = (h + S - 1) / S, ow = (wd + S - 1) / S;
    const int ph = ((oh - 1) * S + 3 - h) / 2, pw = ((ow - 1) * S + 3 - wd) / 2;
    const long pixels = (long)n * oh * ow;
    CN_CHECK_ARG(pixels < 0x7fffffffL, "cn_dwconv3x3_wgrad: tensor too large");
    const DwWgradPlan p = dw_wgrad_plan(pixels, c / V);
    CN_CHECK_ARG(slices == p.slices, "cn_dwconv3x3_wgrad: %d slices given, the plan has %d (cn_dwconv3x3_wgrad_slices)", slices, p.slices);
    hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<S, V>), dim3(p.cb, p.slices), dim3(256), 0, s, x, gy, part, h, wd, c, oh, ow, ph, pw,
                       (int)pixels, p.per_slice, p.TX, p.TY);
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

extern "C" int cn_dwconv3x3_dgrad(const float* gy, const float* w, float* gx, int n, int h, int wd, int c, int stride, void* stream) {
    CN_CHECK_ARG(gy && w && gx, "cn_dwconv3x3_dgrad: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0, "cn_dwconv3x3_dgrad: bad extents n %d h %d w %d c %d", n, h, wd, c);
    CN_CHECK_ARG(stride == 1 || stride == 2, "cn_dwconv3x3_dgrad: stride must be 1 or 2 (got %d)", stride);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = c % 4 == 0 && ((uintptr_t)gy | (uintptr_t)w | (uintptr_t)gx) % 16 == 0;
    if (stride == 1) return v4 ? launch_dw_dgrad<1, 4, 4, 2>(gy, w, gx, n, h, wd, c, s) : launch_dw_dgrad<1, 1, 4, 2>(gy, w, gx, n, h, wd, c, s);
    return v4 ? launch_dw_dgrad<2, 4, 4, 2>(gy, w, gx, n, h, wd, c, s) : launch_dw_dgrad<2, 1, 4, 2>(gy, w, gx, n, h, wd, c, s);
}

extern "C" int cn_dwconv3x3_wgrad_slices(int n, int h, int wd, int c, int stride) {
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0 && (stride == 1 || stride == 2), "cn_dwconv3x3_wgrad_slices: bad extents");
    const long pixels = (long)n * ((h + stride - 1) / stride) * ((wd + stride - 1) / stride);
    return dw_wgrad_plan(pixels, c % 4 == 0 ? c / 4 : c).slices;
}

extern "C" int cn_dwconv3x3_wgrad(const float* x, const float* gy, float* part, int slices, int n, int h, int wd, int c, int stride,
                                  void* stream) {
    CN_CHECK_ARG(x && gy && part, "cn_dwconv3x3_wgrad: NULL");
    CN_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0, "cn_dwconv3x3_wgrad: bad extents n %d h %d w %d c %d", n, h, wd, c);
    CN_CHECK_ARG(stride == 1 || stride == 2, "cn_dwconv3x3_wgrad: stride must be 1 or 2 (got %d)", stride);
    hipStream_t s = (hipStream_t)stream;
    if (c % 4 == 0) {                                  // (the slice plan follows c alone, so the float4 walk is not optional here)
        CN_CHECK_ARG(((uintptr_t)x | (uintptr_t)gy) % 16 == 0, "cn_dwconv3x3_wgrad: x and gy must be 16-byte aligned when c %% 4 == 0");
        return stride == 1 ? launch_dw_wgrad<1, 4>(x, gy, part, slices, n, h, wd, c, s) : launch_dw_wgrad<2, 4>(x, gy, part, slices, n, h, wd, c, s);
    }
    return stride == 1 ? launch_dw_wgrad<1, 1>(x, gy, part, slices, n, h, wd, c, s) : launch_dw_wgrad<2, 1>(x, gy, part, slices, n, h, wd, c, s);
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
