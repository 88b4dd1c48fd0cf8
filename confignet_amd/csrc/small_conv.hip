// small_conv.hip -- the convolutions whose output or input is too thin for the implicit-GEMM tiles (igemm_conv.hip, fwd2.hip):
// thin-output direct convolutions (cout <= 4), the image-side first layers (3x3 and 7x7 convolutions of the 3-channel image) and
// their data gradients into the image, map_final of the generator; plus two small helpers of the same family (the tap-flipped
// filter copy and the backward of the folded x2 upsample).  Which of them a geometry gets is conv_dispatch.hip's decision
// (ConvRoute); cn_small_conv at the end of this file is the one place they are launched from.
#include "common.h"

#include "mma_tile.h"
#include "typed.h"
#include "conv_geom.h"

namespace {

// ---------------------------------------------------------------------------------------------
// thin-output direct convolution (cout <= 4): HBM-bound, one thread per output position.
// Used for map_final (32->3, hologan_generator.py:101), the 1x1 3->3 from-RGB conv
// (hologan_discriminator.py:20) and the data-gradient of every 3-channel-input conv.
// ---------------------------------------------------------------------------------------------
template <int CO, bool VEC>
__global__ __launch_bounds__(256) void thin_conv_kernel(CnConvGeom g, const float* __restrict__ X,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        float* __restrict__ Y, int act, float slope, int par) {
    extern __shared__ __attribute__((aligned(16))) float wsh[];     // [taps*cin][4] filter, broadcast reads
    const int M = g.n * g.out_d * g.out_h * g.out_w;
    const int Ktot = g.k_d * g.k_h * g.k_w * g.cin;
    for (int i = threadIdx.x; i < Ktot; i += 256) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wsh[i * 4 + c] = c < CO ? W[(long)i * CO + c] : 0.f;
    }
    __syncthreads();
    int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    if (par) {
        int cls;
        m = par_row(g, m, M, cls);
    }
    const RowInfo r = decode_row(g, m, M);
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = bias ? bias[c] : 0.f;
    int tap = 0;
    for (int kd = 0; kd < g.k_d; ++kd)
        for (int kh = 0; kh < g.k_h; ++kh)
            for (int kw = 0; kw < g.k_w; ++kw, ++tap) {
                const int off = src_off(g, r, kd, kh, kw);
                if (off < 0) continue;
                const float4* wp = reinterpret_cast<const float4*>(wsh) + tap * g.cin;
                if (VEC) {
                    for (int ci = 0; ci < g.cin; ci += 4) {
                        const float4 xv = *reinterpret_cast<const float4*>(X + off + ci);
                        const float4 w0 = wp[ci], w1 = wp[ci + 1], w2 = wp[ci + 2], w3 = wp[ci + 3];
                        const float wv[4][4] = {{w0.x, w0.y, w0.z, w0.w}, {w1.x, w1.y, w1.z, w1.w},
                                                {w2.x, w2.y, w2.z, w2.w}, {w3.x, w3.y, w3.z, w3.w}};
#pragma unroll
                        for (int c = 0; c < CO; ++c)
                            acc[c] += xv.x * wv[0][c] + xv.y * wv[1][c] + xv.z * wv[2][c] + xv.w * wv[3][c];
                    }
                } else {
                    for (int ci = 0; ci < g.cin; ++ci) {
                        const float xv = X[off + ci];
                        const float4 w0 = wp[ci];
                        const float wv[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
                        for (int c = 0; c < CO; ++c) acc[c] += xv * wv[c];
                    }
                }
            }
#pragma unroll
    for (int c = 0; c < CO; ++c) Y[(long)m * CO + c] = cn_apply_act(acc[c], act, slope);
}

// Cooperative thin-output convolution: G (= 8 or 16) lanes share one output pixel, lane c4 owning input
// channels [4*c4, 4*c4+4), so every global load instruction is a run of fully used 16-byte pieces
// (G*16 contiguous bytes per pixel), each thread carries PX pixels per filter read (4 broadcast-ish LDS
// reads feed 4*CO*PX FMAs), and the partial sums are combined with G-lane shuffles.  In parity-ordered
// mode (data-gradient of a stride-2 convolution into the 3-channel image) the per-class tap validity and
// coordinate shifts come from a small LDS table instead of per-thread integer divisions.
template <int CO, int G, int PX>
__global__ __launch_bounds__(256) void thin_conv_coop_kernel(CnConvGeom g, const float* __restrict__ X,
                                                             const float* __restrict__ W, const float* __restrict__ bias,
                                                             float* __restrict__ Y, int act, float slope, int par) {
    extern __shared__ __attribute__((aligned(16))) float wsh[];     // [taps*cin][4] filter
    __shared__ int tab[8][32];                                      // par: class x tap -> packed shifts / -1
    constexpr int PPB = 256 / G;                                    // pixel slots per block per step
    const int M = g.n * g.out_d * g.out_h * g.out_w;
    const int T = g.k_d * g.k_h * g.k_w;
    const int Ktot = T * g.cin;
    const int CL = g.cin / 4;
    for (int i = threadIdx.x; i < Ktot; i += 256) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wsh[i * 4 + c] = c < CO ? W[(long)i * CO + c] : 0.f;
    }
    if (par && threadIdx.x < 8 * 32) {
        const int cls = threadIdx.x >> 5, tap = threadIdx.x & 31;
        int e = -1;
        if (cls < g.dl_d * g.dl_h * g.dl_w && tap < T) {
            const int cw = cls % g.dl_w, ch = (cls / g.dl_w) % g.dl_h, cd = cls / (g.dl_w * g.dl_h);
            int kd, kh, kw;
            tap_decode(g, tap, kd, kh, kw);
            const int vd = cd - g.p_d + kd, vh = ch - g.p_h + kh, vw = cw - g.p_w + kw;
            if (vd % g.dl_d == 0 && vh % g.dl_h == 0 && vw % g.dl_w == 0)
                e = ((vd / g.dl_d + 8) << 8) | ((vh / g.dl_h + 8) << 4) | (vw / g.dl_w + 8);   // shifts in [-8, 7]
        }
        tab[cls][tap] = e;
    }
    __syncthreads();
    const int slot = threadIdx.x / G, c4 = threadIdx.x % G;
    const bool lane_on = c4 < CL;
    const int qd_ext = g.out_d / g.dl_d, qh_ext = g.out_h / g.dl_h, qw_ext = g.out_w / g.dl_w;
    const int per = g.n * qd_ext * qh_ext * qw_ext;
    int nb[PX], xd[PX], xh[PX], xw[PX], cls[PX], mrow[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const int mp = (blockIdx.x * PX + p) * PPB + slot;
        cls[p] = -1;
        mrow[p] = -1;
        nb[p] = xd[p] = xh[p] = xw[p] = 0;
        if (mp >= M) continue;
        if (par) {
            const int c = mp / per;
            int rem = mp - c * per;
            const int cw = c % g.dl_w, chh = (c / g.dl_w) % g.dl_h, cd = c / (g.dl_w * g.dl_h);
            xw[p] = rem % qw_ext; rem /= qw_ext;
            xh[p] = rem % qh_ext; rem /= qh_ext;
            xd[p] = rem % qd_ext;
            const int n = rem / qd_ext;
            nb[p] = n * g.in_d;
            cls[p] = c;
            mrow[p] = ((n * g.out_d + xd[p] * g.dl_d + cd) * g.out_h + xh[p] * g.dl_h + chh) * g.out_w + xw[p] * g.dl_w + cw;
        } else {
            int m = mp;
            int ow, oh, od, nn;
            divmod_pos(m, g.out_w, m, ow);
            divmod_pos(m, g.out_h, m, oh);
            divmod_pos(m, g.out_d, nn, od);
            nb[p] = nn * g.in_d;
            xd[p] = od * g.s_d - g.p_d; xh[p] = oh * g.s_h - g.p_h; xw[p] = ow * g.s_w - g.p_w;
            cls[p] = 0;
            mrow[p] = mp;
        }
    }
    float acc[PX][CO];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int c = 0; c < CO; ++c) acc[p][c] = 0.f;
    const int ed = g.in_d << g.up, eh = g.in_h << g.up, ew = g.in_w << g.up;
    int tap = 0;
    for (int kd = 0; kd < g.k_d; ++kd)
        for (int kh = 0; kh < g.k_h; ++kh)
            for (int kw = 0; kw < g.k_w; ++kw, ++tap) {
                float4 xv[PX];
                bool any = false;
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    xv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (cls[p] < 0 || !lane_on) continue;
                    int qd, qh, qw;
                    if (par) {
                        const int e = tab[cls[p]][tap];
                        if (e < 0) continue;
                        qd = xd[p] + ((e >> 8) & 15) - 8; qh = xh[p] + ((e >> 4) & 15) - 8; qw = xw[p] + (e & 15) - 8;
                        if (qd < 0 || qd >= g.in_d || qh < 0 || qh >= g.in_h || qw < 0 || qw >= g.in_w) continue;
                    } else {
                        qd = xd[p] + kd; qh = xh[p] + kh; qw = xw[p] + kw;
                        if (qd < 0 || qd >= ed || qh < 0 || qh >= eh || qw < 0 || qw >= ew) continue;
                        qd >>= g.up; qh >>= g.up; qw >>= g.up;
                    }
                    const long off = ((((long)nb[p] + qd) * g.in_h + qh) * g.in_w + qw) * g.cin + c4 * 4;
                    xv[p] = *reinterpret_cast<const float4*>(X + off);
                    any = true;
                }
                if (!any) continue;
                const float4* wp = reinterpret_cast<const float4*>(wsh) + (tap * g.cin + c4 * 4);
                const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
                const float wv[4][4] = {{w0.x, w0.y, w0.z, w0.w}, {w1.x, w1.y, w1.z, w1.w},
                                        {w2.x, w2.y, w2.z, w2.w}, {w3.x, w3.y, w3.z, w3.w}};
#pragma unroll
                for (int p = 0; p < PX; ++p)
#pragma unroll
                    for (int c = 0; c < CO; ++c)
                        acc[p][c] += xv[p].x * wv[0][c] + xv[p].y * wv[1][c] + xv[p].z * wv[2][c] + xv[p].w * wv[3][c];
            }
#pragma unroll
    for (int p = 0; p < PX; ++p) {
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            float v = acc[p][c];
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            acc[p][c] = v;
        }
        if (c4 == 0 && mrow[p] >= 0) {
#pragma unroll
            for (int c = 0; c < CO; ++c)
                Y[(long)mrow[p] * CO + c] = cn_apply_act(acc[p][c] + (bias ? bias[c] : 0.f), act, slope);
        }
    }
}

__global__ void weight_tflip_kernel(const float* __restrict__ W, float* __restrict__ Wt, int T, int cin, int cout) {
    const long total = (long)T * cin * cout;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        // i indexes Wt[t'][co][ci]
        const int ci = (int)(i % cin);
        const long r = i / cin;
        const int co = (int)(r % cout);
        const int tp = (int)(r / cout);
        Wt[i] = W[((long)(T - 1 - tp) * cin + ci) * cout + co];
    }
}

template <int ND, typename T>
__global__ void sumpool2_kernel(const T* __restrict__ GU, T* __restrict__ GX, int n, int d, int h, int w, int c4) {
    const long total = (long)n * d * h * w * c4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cc = (int)(i % c4);
    long t = i / c4;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    t /= h;
    const int z = (int)(t % d);
    const int b = (int)(t / d);
    const int H2 = 2 * h, W2 = 2 * w, D2 = ND == 3 ? 2 * d : 1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int dz = 0; dz < (ND == 3 ? 2 : 1); ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int zz = ND == 3 ? 2 * z + dz : 0;
                const float4 v = ld4<T>(GU + 4 * (((((long)b * D2 + zz) * H2 + 2 * y + dy) * W2 + 2 * x + dx) * c4 + cc));
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
    st4<T>(GX + 4 * i, s);
}

// ---------------------------------------------------------------------------------------------
// Data gradient of a 3x3 stride-2 convolution INTO a 3-channel image (first DiscrBlock of the discriminators and
// of the latent regressor: 29 launches per second-stage iteration).  As a gather -- one output pixel = <= 4 live
// taps x C channels x 3 outputs -- the 32-column MFMA tile spends 10x the useful work on padding.  Transposed,
// every INPUT pixel owns one small dense product
//     P[pixel][tap*3 + co] = sum_c gy[pixel][c] * wt[tap][c][co]        (C x 27, one 32-column MFMA block)
// and each output pixel is the sum of the <= 4 entries of P that land on it (col2im).  One workgroup: (TH+1) x (TW+1)
// input pixels (one halo row/column, on the side the padding fixes) -> P in LDS -> its 2TH x 2TW output pixels.
// No atomics, gy is read once (+ halo), K order is permuted so that a lane's A operand is one float4 load.
template <int NG, typename TI = float>   // C = 8 * NG; TI: storage type of gy (fp32 / bf16)
__global__ __launch_bounds__(256) void s2_image_dgrad_kernel(CnConvGeom g, const TI* __restrict__ GY,
                                                             const float* __restrict__ WT, float* __restrict__ Y) {
    constexpr int TH = 8, TW = 32, RW = TW + 1, R = (TH + 1) * RW, MT = (R + 31) / 32, PS = 28, C = 8 * NG;
    __shared__ float P[MT * 32][PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles_w = (g.in_w + TW - 1) / TW, tiles_h = (g.in_h + TH - 1) / TH;
    int b = blockIdx.x;
    const int tj = b % tiles_w; b /= tiles_w;
    const int ti = b % tiles_h;
    const int n = b / tiles_h;
    const int i0 = ti * TH, j0 = tj * TW;
    // output row y = 2i + p - kh (kh = 0..2): rows [2 i0, 2 i0 + 2 TH) are fed by input rows [i0 + off, i0 + off + TH]
    const int offh = g.p_h == 2 ? -1 : 0, offw = g.p_w == 2 ? -1 : 0;

    // B operand (K x 32 slice of wt, K permuted as below), resident in registers for the whole workgroup
    float breg[NG][4];
#pragma unroll
    for (int jg = 0; jg < NG; ++jg)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 8 * jg + 4 * half + q;
            breg[jg][q] = l31 < 27 ? WT[((l31 / 3) * C + k) * 3 + l31 % 3] : 0.f;
        }

    for (int mt = wave; mt < MT; mt += 4) {
        const int r = mt * 32 + l31;
        const int ri = r / RW, rj = r - ri * RW;
        const int ii = i0 + offh + ri, jj = j0 + offw + rj;
        const bool inb = r < R && ii >= 0 && ii < g.in_h && jj >= 0 && jj < g.in_w;
        // lane (row, half) holds channels 8 jg + 4 half + {0..3}: MFMA step (jg, q) contracts channel pair
        // {8 jg + q, 8 jg + 4 + q} -- any K order is fine as long as A and B agree
        const TI* src = GY + (((long)n * g.in_h + ii) * g.in_w + jj) * C + 4 * half;
        float4 a[NG];
#pragma unroll
        for (int jg = 0; jg < NG; ++jg)
            a[jg] = inb ? ld4<TI>(src + 8 * jg) : make_float4(0.f, 0.f, 0.f, 0.f);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int jg = 0; jg < NG; ++jg) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].x, breg[jg][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].y, breg[jg][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].z, breg[jg][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].w, breg[jg][3], acc, 0, 0, 0);
        }
        if (l31 < PS) {
#pragma unroll
            for (int q = 0; q < 16; ++q) P[mt * 32 + 4 * half + (q & 3) + 8 * (q >> 2)][l31] = acc[q];
        }
    }
    __syncthreads();

    // col2im: 2TH x 2TW output pixels, 4 per thread
#pragma unroll
    for (int q = 0; q < (2 * TH * 2 * TW) / 256; ++q) {
        const int px = threadIdx.x + 256 * q;
        const int ly = px / (2 * TW), lx = px - ly * (2 * TW);
        const int y = 2 * i0 + ly, x = 2 * j0 + lx;
        if (y >= g.out_h || x >= g.out_w) continue;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int vy = y - g.p_h + kh;
            if (vy < 0 || (vy & 1) || (vy >> 1) >= g.in_h) continue;
            const int ri = (vy >> 1) - (i0 + offh);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int vx = x - g.p_w + kw;
                if (vx < 0 || (vx & 1) || (vx >> 1) >= g.in_w) continue;
                const float* pr = &P[ri * RW + (vx >> 1) - (j0 + offw)][(kh * 3 + kw) * 3];
                s0 += pr[0];
                s1 += pr[1];
                s2 += pr[2];
            }
        }
        float* dst = Y + (((long)n * g.out_h + y) * g.out_w + x) * 3;
        dst[0] = s0;
        dst[1] = s1;
        dst[2] = s2;
    }
}

// Data gradient of a 3x3 stride-1 convolution INTO a 3-channel image (VGG conv1_1 under the perceptual loss, twice per
// generator step).  Same transposition as s2_image_dgrad_kernel: P[pixel][tap*3 + co] = sum_c gy[pixel][c] wt[tap][c][co]
// for the (TH+2) x (TW+2) input pixels around a TH x TW output tile (one 32-column MFMA block per 32 pixels, gy read once
// + halo), then every output pixel sums its 9 entries of P.
template <int NG, typename TI = float>   // C = 8 * NG
__global__ __launch_bounds__(256) void s1_image_dgrad_kernel(CnConvGeom g, const TI* __restrict__ GY,
                                                             const float* __restrict__ WT, float* __restrict__ Y) {
    constexpr int TH = 8, TW = 32, RW = TW + 2, R = (TH + 2) * RW, MT = (R + 31) / 32, PS = 29, C = 8 * NG;
    __shared__ float P[MT * 32][PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles_w = (g.out_w + TW - 1) / TW, tiles_h = (g.out_h + TH - 1) / TH;
    int b = blockIdx.x;
    const int tj = b % tiles_w; b /= tiles_w;
    const int ti = b % tiles_h;
    const int n = b / tiles_h;
    const int i0 = ti * TH - g.p_h, j0 = tj * TW - g.p_w;          // first input row / column of the patch

    float breg[NG][4];
#pragma unroll
    for (int jg = 0; jg < NG; ++jg)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 8 * jg + 4 * half + q;
            breg[jg][q] = l31 < 27 ? WT[((l31 / 3) * C + k) * 3 + l31 % 3] : 0.f;
        }

    for (int mt = wave; mt < MT; mt += 4) {
        const int r = mt * 32 + l31;
        const int ri = r / RW, rj = r - ri * RW;
        const int ii = i0 + ri, jj = j0 + rj;
        const bool inb = r < R && ii >= 0 && ii < g.in_h && jj >= 0 && jj < g.in_w;
        const TI* src = GY + (((long)n * g.in_h + ii) * g.in_w + jj) * C + 4 * half;
        float4 a[NG];
#pragma unroll
        for (int jg = 0; jg < NG; ++jg)
            a[jg] = inb ? ld4<TI>(src + 8 * jg) : make_float4(0.f, 0.f, 0.f, 0.f);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int jg = 0; jg < NG; ++jg) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].x, breg[jg][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].y, breg[jg][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].z, breg[jg][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jg].w, breg[jg][3], acc, 0, 0, 0);
        }
        if (l31 < 27) {
#pragma unroll
            for (int q = 0; q < 16; ++q) P[mt * 32 + 4 * half + (q & 3) + 8 * (q >> 2)][l31] = acc[q];
        }
    }
    __syncthreads();

    const int ly = threadIdx.x / TW, lx = threadIdx.x - ly * TW;
    const int y = ti * TH + ly, x = tj * TW + lx;
    if (y >= g.out_h || x >= g.out_w) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const float* pr = &P[(ly + kh) * RW + lx + kw][(kh * 3 + kw) * 3];   // out-of-image pixels hold zeros
            s0 += pr[0];
            s1 += pr[1];
            s2 += pr[2];
        }
    float* dst = Y + (((long)n * g.out_h + y) * g.out_w + x) * 3;
    dst[0] = s0;
    dst[1] = s1;
    dst[2] = s2;
}

// ---------------------------------------------------------------------------------------------
// Epilogue of the image-side forward kernels below: one wave's 32 output pixels (one row segment) x cout channels, accumulators
// in the 32 x 32 MFMA layout (lane = channel, register = pixel), -> bias, activation, store.  yrow: the segment's first pixel;
// pix: pixels of it that exist (>= 32: all).
// staged: the 32 pixels x cout values are one contiguous run of the NHWC output: pass them through LDS, 16 pixels at a time
// ([pixel][channel] = the run's own layout; st: 16 * 32 NB floats of this wave's), and write the run with 16-byte stores -- lane c
// writes bytes 16 c .. of it.  (Straight from the accumulators a lane owns ONE channel of 16 pixels: 4-byte -- in bf16 2-byte --
// stores, 64 of them per row; the bf16 variant took longer than the fp32 one.)  Needs cout % (16 / sizeof(TO)) == 0 and a
// 16-byte aligned tensor; otherwise the element-wise form.
template <int NB, typename TO>
__device__ __forceinline__ void image_row_epilogue(const f32x16 (&acc)[NB], float* st, bool staged, TO* yrow, int pix, int cout,
                                                   const float* __restrict__ bias, int act, float slope) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
    if (staged) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int col = nb * 32 + l31;
                if (col < cout) {
                    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
                    for (int qq = 0; qq < 8; ++qq)
                        st[(4 * half + (qq & 3) + 8 * (qq >> 2)) * cout + col] = cn_apply_act(acc[nb][8 * ph + qq] + bv, act, slope);
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            constexpr int CH = 16 / (int)sizeof(TO);                    // channels per 16-byte chunk
            const int cpp = cout / CH, nch = 16 * cpp;
            const int pix_left = pix - 16 * ph;                         // pixels of this half that exist (>= 16: all)
            for (int c = lane; c < nch; c += 64) {
                if (pix_left < 16 && c / cpp >= pix_left) continue;
                const float4 v0 = *reinterpret_cast<const float4*>(st + c * CH);
                if constexpr (sizeof(TO) == 4) {
                    *reinterpret_cast<float4*>(reinterpret_cast<float*>(yrow) + 16 * ph * cout + c * 4) = v0;
                } else {
                    const float4 v1 = *reinterpret_cast<const float4*>(st + c * CH + 4);
                    uint4 o;
                    o.x = (unsigned)f32_to_bf16(v0.x) | ((unsigned)f32_to_bf16(v0.y) << 16);
                    o.y = (unsigned)f32_to_bf16(v0.z) | ((unsigned)f32_to_bf16(v0.w) << 16);
                    o.z = (unsigned)f32_to_bf16(v1.x) | ((unsigned)f32_to_bf16(v1.y) << 16);
                    o.w = (unsigned)f32_to_bf16(v1.z) | ((unsigned)f32_to_bf16(v1.w) << 16);
                    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(yrow) + 16 * ph * cout + c * 8) = o;
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
        return;
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = nb * 32 + l31;
        if (col >= cout) continue;
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int px = 4 * half + (q & 3) + 8 * (q >> 2);
            if (px < pix) stf<TO>(yrow + (long)px * cout + col, cn_apply_act(acc[nb][q] + bv, act, slope));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// First layers: 3x3 convolution of a 3-channel image (DiscrBlock 0 of both discriminators and the latent regressor,
// VGG conv1_1): K = 27.  The generic kernel gathers those 27 values with per-element integer division (cin = 3 is not
// a float4).  Here a workgroup stages the input patch of an 8 x 32 output tile in LDS once (coalesced rows), the K
// axis is padded to 28 = 14 MFMA steps, rows = output pixels and the whole filter sits in registers.
// (A matching filter-gradient kernel -- rows = the 27 filter rows, K' = pixels -- was tried and dropped: with a
// 27 x cout output every workgroup ends in the same 1296 atomics, and ~75 ns per same-address atomic put it at
// 70-90 us against the generic kernel's 65.)
template <int S, int NB, typename TO = float>   // TO: storage type of the output (fp32 / bf16)
__global__ __launch_bounds__(256) void c3_fwd_kernel(CnConvGeom g, const float* __restrict__ X, const float* __restrict__ W,
                                                     const float* __restrict__ bias, TO* __restrict__ Y, int act, float slope) {
    constexpr int TH = 8, TW = 32, PR = (TH - 1) * S + 3, PC = ((TW - 1) * S + 3) * 3, PCP = PC + 1;
    __shared__ float patch[PR * PCP];
    __shared__ __attribute__((aligned(16))) float stage[4][16 * NB * 32];      // per wave: 16 pixels x cout of the epilogue
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles_w = (g.out_w + TW - 1) / TW, tiles_h = (g.out_h + TH - 1) / TH;
    int b = blockIdx.x;
    const int tj = b % tiles_w; b /= tiles_w;
    const int ti = b % tiles_h;
    const int n = b / tiles_h;
    const int oy0 = ti * TH, ox0 = tj * TW, iy0 = oy0 * S - g.p_h, ix0 = ox0 * S - g.p_w;
    // 16-byte stores need whole chunks per pixel and an aligned tensor (else: the element-wise epilogue)
    const bool staged = g.cout % (16 / (int)sizeof(TO)) == 0 && ((uintptr_t)Y & 15) == 0;
    float breg[14][NB];
    int aoff[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) {
        const int k = 2 * q + half;
        const int kh = k / 9, kw = (k - kh * 9) / 3, ci = k - kh * 9 - kw * 3;
        aoff[q] = k < 27 ? kh * PCP + kw * 3 + ci : 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 32 + l31;
            breg[q][nb] = (k < 27 && col < g.cout) ? W[k * g.cout + col] : 0.f;
        }
    }
    {
        // patch rows: a thread owns one column of the patch (PC <= 256 / RPP floats per row) and every RPP-th row; ALL its loads
        // are issued before the first LDS store (a load -> wait -> store loop serialises PR x PC / 256 memory round trips per
        // workgroup: that loop, not the MFMA work or the stores, was what the kernel's time consisted of)
        constexpr int PCC = PC <= 128 ? 128 : 256, RPP = 256 / PCC, NR = (PR + RPP - 1) / RPP;
        static_assert(PC <= 256, "patch row wider than the workgroup");
        const int c = threadIdx.x % PCC, rs = threadIdx.x / PCC;
        const int ix = ix0 + c / 3;
        const bool cok = c < PC, xin = cok && ix >= 0 && ix < g.in_w;
        // (branch-free: an out-of-image element loads X[0] and is zeroed afterwards.  As `ok ? X[...] : 0` hipcc put each guarded
        // load in its own exec-mask region and, in the <2, 2, float> instance, waited for it there: seven round trips were left.)
        const long xb = ((long)n * g.in_h * g.in_w + ix0) * 3 + c;
        float pv[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int r = rs + RPP * i, iy = iy0 + r;
            const bool ok = xin && r < PR && iy >= 0 && iy < g.in_h;
            const float v = X[ok ? xb + (long)iy * g.in_w * 3 : 0L];
            pv[i] = ok ? v : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int r = rs + RPP * i;
            if (cok && r < PR) patch[r * PCP + c] = pv[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = wave * 2 + rr;
        const int base = r * S * PCP + l31 * S * 3;
        f32x16 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[nb][q] = 0.f;
#pragma unroll
        for (int q = 0; q < 14; ++q) {
            const float a = patch[base + aoff[q]];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, breg[q][nb], acc[nb], 0, 0, 0);
        }
        const int oy = oy0 + r;
        if (oy >= g.out_h) continue;
        image_row_epilogue<NB, TO>(acc, stage[wave], staged, Y + (((long)n * g.out_h + oy) * g.out_w + ox0) * g.cout, g.out_w - ox0, g.cout,
                                   bias, act, slope);
    }
}

// ---------------------------------------------------------------------------------------------
// ResNet-50 conv1 (real_encoder.py:13, keras ResNet50: ZeroPadding2D(3) + 7x7 stride-2 convolution of the 3-channel image): K = 147.
// The generic kernel gathered those with per-element integer division (190 us on 16 images at 256^2 against ~32 us of MFMA work);
// here, as in c3_fwd_kernel, a workgroup stages the 21 x 69-pixel patch of its 8 x 32 output tile once (every load in flight before
// the first LDS store), and walks the filter one kernel row (21 values = 11 MFMA steps, the last half-empty) at a time: the next
// row's filter slice is loaded while this row's MFMAs run, and both of a wave's output rows use it.
template <int NB, typename TO = float, int RPW = 2>      // RPW: output rows per wave (tile = 4 RPW rows x 32 pixels; 1: 96 -> 87 us at 1024 tiles, 39 -> 44 at 512)
__global__ __launch_bounds__(256) void c7s2_fwd_kernel(CnConvGeom g, const float* __restrict__ X, const float* __restrict__ W,
                                                       const float* __restrict__ bias, TO* __restrict__ Y, int act, float slope) {
    constexpr int S = 2, KS = 7, TH = 4 * RPW, TW = 32, PR = (TH - 1) * S + KS, PC = ((TW - 1) * S + KS) * 3, PCP = PC + 1;
    constexpr int KR = KS * 3, NQ = (KR + 1) / 2;
    static_assert(PC <= 256, "patch row wider than the workgroup");
    __shared__ float patch[PR * PCP];
    __shared__ __attribute__((aligned(16))) float stage[4][16 * NB * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles_w = (g.out_w + TW - 1) / TW, tiles_h = (g.out_h + TH - 1) / TH;
    int b = blockIdx.x;
    const int tj = b % tiles_w; b /= tiles_w;
    const int ti = b % tiles_h;
    const int n = b / tiles_h;
    const int oy0 = ti * TH, ox0 = tj * TW, iy0 = oy0 * S - g.p_h, ix0 = ox0 * S - g.p_w;
    const bool staged = g.cout % (16 / (int)sizeof(TO)) == 0 && ((uintptr_t)Y & 15) == 0;
    float bq[2][NQ][NB];
    auto load_b = [&](int kh, float (*dst)[NB]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int k = 2 * q + half;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int col = nb * 32 + l31;
                dst[q][nb] = (k < KR && col < g.cout) ? W[(kh * KR + k) * g.cout + col] : 0.f;
            }
        }
    };
    load_b(0, bq[0]);
    {
        const int c = threadIdx.x;
        const int ix = ix0 + c / 3;
        const bool cok = c < PC, xin = cok && ix >= 0 && ix < g.in_w;
        const long xb = ((long)n * g.in_h * g.in_w + ix0) * 3 + c;      // (branch-free loads: see c3_fwd_kernel)
        float pv[PR];
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            const int iy = iy0 + r;
            const bool ok = xin && iy >= 0 && iy < g.in_h;
            const float v = X[ok ? xb + (long)iy * g.in_w * 3 : 0L];
            pv[r] = ok ? v : 0.f;
        }
#pragma unroll
        for (int r = 0; r < PR; ++r)
            if (cok) patch[r * PCP + c] = pv[r];
    }
    __syncthreads();
    f32x16 acc[RPW][NB];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[rr][nb][q] = 0.f;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh) {
        if (kh + 1 < KS) load_b(kh + 1, bq[(kh + 1) & 1]);
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int base = ((wave * RPW + rr) * S + kh) * PCP + l31 * S * 3;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = 2 * q + half;
                const float a = patch[base + (k < KR ? k : 0)];           // (k = 21: its filter value is 0, the address stays inside the row)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[rr][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq[kh & 1][q][nb], acc[rr][nb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int oy = oy0 + wave * RPW + rr;
        if (oy >= g.out_h) continue;
        image_row_epilogue<NB, TO>(acc[rr], stage[wave], staged, Y + (((long)n * g.out_h + oy) * g.out_w + ox0) * g.cout, g.out_w - ox0, g.cout,
                                   bias, act, slope);
    }
}

// ---------------------------------------------------------------------------------------------
// map_final of the generator: x2 nearest upsample folded into a 4x4 convolution from C (= 32) channels to the 3-channel
// image, + bias + tanh.  Same transposition as s2_image_dgrad_kernel: every INPUT pixel owns
//     P[pixel][tap*3 + co] = sum_c x[pixel][c] * w[tap][c][co]                 (C x 48: two 32-column MFMA blocks)
// and an output pixel (y, x) adds the 16 entries P[((y+kh-p)>>1, (x+kw-p)>>1)][kh*4+kw] that land on it.  One workgroup:
// (TH+2) x (TW+2) input pixels -> P in LDS -> its 2TH x 2TW output pixels.  The VALU kernel it replaces spent 240 us
// on 16 images at 256^2 (3.2 GFLOP of lane-serial FMAs); here the contraction is 1 GFLOP of MFMA and the pass is
// bounded by reading the input once.
template <int NG>   // C = 8 * NG
__global__ __launch_bounds__(256) void up2k4_rgb_fwd_kernel(CnConvGeom g, const float* __restrict__ X, const float* __restrict__ W,
                                                            const float* __restrict__ bias, float* __restrict__ Y, int act,
                                                            float slope) {
    constexpr int TH = 8, TW = 16, RW = TW + 2, R = (TH + 2) * RW, MT = (R + 31) / 32, PS = 49, C = 8 * NG;
    __shared__ float P[MT * 32 * PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles_w = (g.in_w + TW - 1) / TW, tiles_h = (g.in_h + TH - 1) / TH;
    int b = blockIdx.x;
    const int tj = b % tiles_w; b /= tiles_w;
    const int ti = b % tiles_h;
    const int n = b / tiles_h;
    const int i0 = ti * TH - 1, j0 = tj * TW - 1;          // first input row / column of the patch (may be -1)
    float breg[NG * 4][2];
#pragma unroll
    for (int q = 0; q < NG * 4; ++q) {
        const int k = 8 * (q >> 2) + 4 * half + (q & 3);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int col = nb * 32 + l31;                 // = tap * 3 + co
            breg[q][nb] = col < 48 ? W[((col / 3) * C + k) * 3 + col % 3] : 0.f;
        }
    }
    for (int mt = wave; mt < MT; mt += 4) {
        const int r = mt * 32 + l31;
        const int ri = r / RW, rj = r - ri * RW;
        const int ii = i0 + ri, jj = j0 + rj;
        const bool inb = r < R && ii >= 0 && ii < g.in_h && jj >= 0 && jj < g.in_w;
        const float* src = X + (((long)n * g.in_h + ii) * g.in_w + jj) * C + 4 * half;
        float4 a[NG];
#pragma unroll
        for (int jg = 0; jg < NG; ++jg)
            a[jg] = inb ? *reinterpret_cast<const float4*>(src + 8 * jg) : make_float4(0.f, 0.f, 0.f, 0.f);
        f32x16 acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[nb][q] = 0.f;
#pragma unroll
        for (int jg = 0; jg < NG; ++jg) {
            const float av[4] = {a[jg].x, a[jg].y, a[jg].z, a[jg].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], breg[jg * 4 + e][nb], acc[nb], 0, 0, 0);
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int col = nb * 32 + l31;
            if (col < 48) {
#pragma unroll
                for (int q = 0; q < 16; ++q) P[(mt * 32 + 4 * half + (q & 3) + 8 * (q >> 2)) * PS + col] = acc[nb][q];
            }
        }
    }
    __syncthreads();
    const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f, b2 = bias ? bias[2] : 0.f;
#pragma unroll
    for (int q = 0; q < (2 * TH * 2 * TW) / 256; ++q) {
        const int px = threadIdx.x + 256 * q;
        const int ly = px / (2 * TW), lx = px - ly * (2 * TW);
        const int y = 2 * (i0 + 1) + ly, x = 2 * (j0 + 1) + lx;
        if (y >= g.out_h || x >= g.out_w) continue;
        float s0 = b0, s1 = b1, s2 = b2;
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
            const int uy = y + kh - g.p_h;                 // row of the upsampled image
            if (uy < 0 || uy >= 2 * g.in_h) continue;
            const int ri = (uy >> 1) - i0;
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                const int ux = x + kw - g.p_w;
                if (ux < 0 || ux >= 2 * g.in_w) continue;
                const float* pr = &P[(ri * RW + (ux >> 1) - j0) * PS + (kh * 4 + kw) * 3];
                s0 += pr[0];
                s1 += pr[1];
                s2 += pr[2];
            }
        }
        float* dst = Y + (((long)n * g.out_h + y) * g.out_w + x) * 3;
        dst[0] = cn_apply_act(s0, act, slope);
        dst[1] = cn_apply_act(s1, act, slope);
        dst[2] = cn_apply_act(s2, act, slope);
    }
}

}  // namespace

// One launch of the route's kernel (conv_dispatch.hip: plan_conv_fwd chose route and grid; vec / par as planned).  x_dt / y_dt: the
// mixed storage types of the bf16 path's first / last layers (cn_conv_fwd_dt), CN_F32 otherwise.  No profile bracket, no launch
// check: both are the caller's.
void cn_small_conv(int route, unsigned grid_x, const CnConvGeom& g, bool vec, int par, const void* xv, int x_dt, const float* w,
                   const float* bias, void* yv, int y_dt, int act, float slope, hipStream_t s) {
    const float* x = (const float*)xv;
    float* y = (float*)yv;
    bf16_t* yb = (bf16_t*)yv;
    const bool ybf = y_dt == CN_BF16;
    const size_t lds = sizeof(float) * 4 * (size_t)g.k_d * g.k_h * g.k_w * g.cin;      // the thin kernels' filter stage
    constexpr int PX = CN_THIN_COOP_PX;
#define LAUNCH(kernel, dyn, ...) hipLaunchKernelGGL(kernel, dim3(grid_x), dim3(256), dyn, s, g, __VA_ARGS__)
#define THIN(CO)                                                                        \
    if (vec) LAUNCH((thin_conv_kernel<CO, true>), lds, x, w, bias, y, act, slope, par); \
    else LAUNCH((thin_conv_kernel<CO, false>), lds, x, w, bias, y, act, slope, par)
#define C3F(S_, NB_)                                                                    \
    if (ybf) LAUNCH((c3_fwd_kernel<S_, NB_, bf16_t>), 0, x, w, bias, yb, act, slope);   \
    else LAUNCH((c3_fwd_kernel<S_, NB_>), 0, x, w, bias, y, act, slope)
#define C7F(NB_)                                                                        \
    if (ybf) LAUNCH((c7s2_fwd_kernel<NB_, bf16_t>), 0, x, w, bias, yb, act, slope);     \
    else LAUNCH((c7s2_fwd_kernel<NB_>), 0, x, w, bias, y, act, slope)
    switch (route) {
        case CN_ROUTE_UP2K4_RGB: LAUNCH((up2k4_rgb_fwd_kernel<4>), 0, x, w, bias, y, act, slope); break;
        case CN_ROUTE_S2_IMAGE_DGRAD:
            if (x_dt == CN_BF16) LAUNCH((s2_image_dgrad_kernel<6, bf16_t>), 0, (const bf16_t*)xv, w, y);
            else LAUNCH((s2_image_dgrad_kernel<6>), 0, x, w, y);
            break;
        case CN_ROUTE_S1_IMAGE_DGRAD: LAUNCH((s1_image_dgrad_kernel<8>), 0, x, w, y); break;
        case CN_ROUTE_THIN_COOP:
            if (g.cin / 4 <= 8) LAUNCH((thin_conv_coop_kernel<3, 8, PX>), lds, x, w, bias, y, act, slope, par);
            else LAUNCH((thin_conv_coop_kernel<3, 16, PX>), lds, x, w, bias, y, act, slope, par);
            break;
        case CN_ROUTE_THIN:
            switch (g.cout) {
                case 1: THIN(1); break;
                case 2: THIN(2); break;
                case 3: THIN(3); break;
                default: THIN(4); break;
            }
            break;
        case CN_ROUTE_C3:
            if (g.s_h == 1) { if (g.cout <= 32) { C3F(1, 1); } else { C3F(1, 2); } }
            else { if (g.cout <= 32) { C3F(2, 1); } else { C3F(2, 2); } }
            break;
        case CN_ROUTE_C7S2:
            if (g.cout <= 32) { C7F(1); } else { C7F(2); }
            break;
        default: break;          // (not a route of this file: run_conv_fwd never passes one)
    }
#undef C7F
#undef C3F
#undef THIN
#undef LAUNCH
}

extern "C" int cn_conv_weight_tflip(const float* w, float* wt, int taps, int cin, int cout, void* stream) {
    CN_CHECK_ARG(w && wt && taps > 0 && cin > 0 && cout > 0, "bad tflip args");
    const long total = (long)taps * cin * cout;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(weight_tflip_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, wt, taps, cin, cout);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_sumpool2(const void* gu, void* gx, int nd, int n, int d, int h, int w, int c, int dt, void* stream) {
    CN_CHECK_ARG(gu && gx && (nd == 2 || nd == 3) && c % 4 == 0 && (dt == CN_F32 || dt == CN_BF16), "sumpool2: bad args (c must be a multiple of 4)");
    if (nd == 2) d = 1;
    const long total = (long)n * d * h * w * (c / 4);
    CN_DISPATCH_DT(dt, {
        if (nd == 3)
            hipLaunchKernelGGL((sumpool2_kernel<3, T>), dim3(cn_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)gu, (T*)gx, n, d, h, w, c / 4);
        else
            hipLaunchKernelGGL((sumpool2_kernel<2, T>), dim3(cn_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)gu, (T*)gx, n, d, h, w, c / 4);
    });
    CN_LAUNCH_CHECK();
    return CN_OK;
}
