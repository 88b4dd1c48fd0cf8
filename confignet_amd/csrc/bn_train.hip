// bn_train.hip -- training-mode BatchNormalization of the attribute classifier's MobileNetV2 (keras BatchNormalization(eps 1e-3,
// momentum 0.99) behind every bias-free convolution, with ReLU(6.) or nothing behind it) over the rows of an (m, c) view of an
// NHWC tensor, m = N H W.
//
// Forward: the per-channel sums are cn_nc_reduce's (one pass); cn_bn_train_coef turns them into a / b and the moving statistics;
// cn_bn_train_apply is the second pass y = act(a x + b).  Backward: cn_bn_train_bwd_reduce is the one reduce pass (sum g and
// sum g xh with the ReLU6 mask taken from y), cn_bn_train_bwd_apply the one apply pass.
// What the existing launches did not cover, and why these four exist: cn_nc_lin2 has ReLU but no ReLU6 behind its affine map;
// act_deriv (cn_bn_act_bwd, cn_nc_reduce_dact) knows no two-sided mask, and those sum g x with the RAW x, which cancels for a
// channel with |mean| >> sigma where sum g (x - mean) r does not; cn_norm_apply's grid is sized per sample and the view has one.
#include "chan_slices.h"

namespace {

__device__ __forceinline__ float relu6_mask(float y, int act) { return act == CN_ACT_RELU6 ? ((y > 0.f && y < 6.f) ? 1.f : 0.f) : 1.f; }

// One workgroup per channel.  mean / var from the one-pass sums; where mean^2 > 1000 (var + eps) the fp32 sums leave an error in
// var that is no longer small under the root (cn_norm_coef_fwd's rule), and the workgroup walks the channel once more for
// sum (x - mean) and sum (x - mean)^2, reduced in a fixed order.
__global__ __launch_bounds__(256) void bn_train_coef_kernel(const float* __restrict__ s1, const float* __restrict__ s2,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ x, float* __restrict__ mean_o, float* __restrict__ var_o,
                                                            float* __restrict__ r_o, float* __restrict__ a_o, float* __restrict__ b_o,
                                                            float* __restrict__ mov_mean, float* __restrict__ mov_var, long m, int c, float eps,
                                                            float decay, int bessel) {
    __shared__ float red[2][256];
    const int ch = blockIdx.x;
    const float inv = 1.f / (float)m;
    float mu = s1[ch] * inv;
    float var = s2[ch] * inv - mu * mu;
    if (x && mu * mu > 1000.f * (var + eps)) {          // (the same value in every thread: a uniform branch)
        float d1 = 0.f, d2 = 0.f;
        for (long i = threadIdx.x; i < m; i += 256) {
            const float d = x[i * c + ch] - mu;
            d1 += d;
            d2 = fmaf(d, d, d2);
        }
        red[0][threadIdx.x] = d1;
        red[1][threadIdx.x] = d2;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                red[0][threadIdx.x] += red[0][threadIdx.x + w];
                red[1][threadIdx.x] += red[1][threadIdx.x + w];
            }
            __syncthreads();
        }
        const float e = red[0][0] * inv;
        mu += e;
        var = red[1][0] * inv - e * e;
    }
    if (threadIdx.x != 0) return;
    var = fmaxf(var, 0.f);
    const float r = rsqrtf(var + eps);
    const float a = gamma[ch] * r;
    mean_o[ch] = mu;
    var_o[ch] = var;
    r_o[ch] = r;
    a_o[ch] = a;
    b_o[ch] = beta[ch] - mu * a;
    if (mov_mean) mov_mean[ch] -= (mov_mean[ch] - mu) * decay;
    if (mov_var) {
        const float v = (bessel && m > 1) ? var * ((float)m / (float)(m - 1)) : var;
        mov_var[ch] -= (mov_var[ch] - v) * decay;
    }
}

template <int V>
__global__ __launch_bounds__(256) void bn_train_apply_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                             const float* __restrict__ b, float* __restrict__ y, long total_g, int c,
                                                             int act) {
    const int cgs = c / V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_g; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % cgs) * V;
        if (V == 4) {
            const float4 xv = *reinterpret_cast<const float4*>(x + i * 4);
            const float4 av = *reinterpret_cast<const float4*>(a + ch), bv = *reinterpret_cast<const float4*>(b + ch);
            float4 o = make_float4(av.x * xv.x + bv.x, av.y * xv.y + bv.y, av.z * xv.z + bv.z, av.w * xv.w + bv.w);
            if (act == CN_ACT_RELU6) o = make_float4(fminf(fmaxf(o.x, 0.f), 6.f), fminf(fmaxf(o.y, 0.f), 6.f), fminf(fmaxf(o.z, 0.f), 6.f), fminf(fmaxf(o.w, 0.f), 6.f));
            *reinterpret_cast<float4*>(y + i * 4) = o;
        } else {
            float o = a[ch] * x[i] + b[ch];
            if (act == CN_ACT_RELU6) o = fminf(fmaxf(o, 0.f), 6.f);
            y[i] = o;
        }
    }
}

// The backward reduce pass: a per-channel reduction over slices of the rows (chan_slices.h: the work split, the slice rule, the
// lane combine), per-slice partials [sum g | sum g xh] left with plain stores and added by the caller in slice order.
template <int V>
__global__ __launch_bounds__(256) void bn_train_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                                  const float* __restrict__ x, const float* __restrict__ mean,
                                                                  const float* __restrict__ r, float* __restrict__ part, long m, int c,
                                                                  long per_slice, int TX, int TY, int act) {
    __shared__ float red[2 * 256 * V];
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
    const int ch = (blockIdx.x * TX + tx) * V;
    float acc[2][V];                                   // sum g | sum g xh
#pragma unroll
    for (int e = 0; e < V; ++e) acc[0][e] = acc[1][e] = 0.f;
    if (ch < c) {
        float mu[V], rs[V];
        VecIO<V>::ld(mean + ch, mu);
        VecIO<V>::ld(r + ch, rs);
        const long r0 = blockIdx.y * per_slice, r1 = r0 + per_slice < m ? r0 + per_slice : m;
        for (long i = r0 + ty; i < r1; i += TY) {
            float g[V], xv[V], yv[V];
            VecIO<V>::ld(gy + i * c + ch, g);
            VecIO<V>::ld(x + i * c + ch, xv);
            if (act == CN_ACT_RELU6) {
                VecIO<V>::ld(y + i * c + ch, yv);
#pragma unroll
                for (int e = 0; e < V; ++e) g[e] *= relu6_mask(yv[e], act);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                acc[0][e] += g[e];
                acc[1][e] = fmaf(g[e], (xv[e] - mu[e]) * rs[e], acc[1][e]);
            }
        }
    }
    chan_lanes_sum<2, V>(acc, red, part, c, TX, TY);
}

template <int V>
__global__ __launch_bounds__(256) void bn_train_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                                 const float* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ r, const float* __restrict__ a,
                                                                 const float* __restrict__ sums, float* __restrict__ gx, long total_g, int c,
                                                                 float inv_m, int act) {
    const int cgs = c / V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total_g; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % cgs) * V;
        float g[V], xv[V], yv[V], mu[V], rs[V], av[V], db[V], dg[V], o[V];
        VecIO<V>::ld(gy + i * V, g);
        VecIO<V>::ld(x + i * V, xv);
        VecIO<V>::ld(mean + ch, mu);
        VecIO<V>::ld(r + ch, rs);
        VecIO<V>::ld(a + ch, av);
        VecIO<V>::ld(sums + ch, db);
        VecIO<V>::ld(sums + c + ch, dg);
        if (act == CN_ACT_RELU6) {
            VecIO<V>::ld(y + i * V, yv);
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] *= relu6_mask(yv[e], act);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = av[e] * (g[e] - (db[e] + (xv[e] - mu[e]) * rs[e] * dg[e]) * inv_m);
        VecIO<V>::st(gx + i * V, o);
    }
}

// The launch of an elementwise pass over (m, c): float4 groups where c % 4 == 0 and every operand is 16-byte aligned, else scalars;
// total_g groups, a grid-stride loop of at most 8192 workgroups.
struct EwShape {
    bool v4;
    long total_g;
    unsigned blocks;
};

template <typename... P>
EwShape ew_shape(long m, int c, const P*... operands) {
    const bool v4 = c % 4 == 0 && aligned16(operands...);
    const long total_g = m * (v4 ? c / 4 : c), b = (total_g + 255) / 256;
    return {v4, total_g, (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b))};
}

}  // namespace

extern "C" int cn_bn_train_coef(const float* s1, const float* s2, const float* gamma, const float* beta, const float* x, float* mean,
                                float* var, float* r, float* a, float* b, float* moving_mean, float* moving_var, long long m, int c,
                                float eps, double momentum, int bessel, void* stream) {
    CN_CHECK_ARG(s1 && s2 && gamma && beta && mean && var && r && a && b, "cn_bn_train_coef: NULL");
    CN_CHECK_ARG(m > 0 && c > 0, "cn_bn_train_coef: bad extents m %lld c %d", m, c);
    hipLaunchKernelGGL(bn_train_coef_kernel, dim3(c), dim3(256), 0, (hipStream_t)stream, s1, s2, gamma, beta, x, mean, var, r, a, b,
                       moving_mean, moving_var, (long)m, c, eps, (float)(1.0 - momentum), bessel);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_bn_train_apply(const float* x, const float* a, const float* b, float* y, long long m, int c, int act, void* stream) {
    CN_CHECK_ARG(x && a && b && y, "cn_bn_train_apply: NULL");
    CN_CHECK_ARG(m > 0 && c > 0, "cn_bn_train_apply: bad extents m %lld c %d", m, c);
    CN_CHECK_ARG(act == CN_ACT_NONE || act == CN_ACT_RELU6, "cn_bn_train_apply: activation %d", act);
    hipStream_t s = (hipStream_t)stream;
    const EwShape e = ew_shape((long)m, c, x, a, b, y);
    if (e.v4) hipLaunchKernelGGL(bn_train_apply_kernel<4>, dim3(e.blocks), dim3(256), 0, s, x, a, b, y, e.total_g, c, act);
    else hipLaunchKernelGGL(bn_train_apply_kernel<1>, dim3(e.blocks), dim3(256), 0, s, x, a, b, y, e.total_g, c, act);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_bn_train_bwd_slices(long long m, int c) {
    CN_CHECK_ARG(m > 0 && c > 0, "cn_bn_train_bwd_slices: bad extents");
    return chan_slices_plan((long)m, c % 4 == 0 ? c / 4 : c, 0).slices;
}

extern "C" int cn_chan_slices_plan(long long rows, int c, int min_rows, int* out5) {
    CN_CHECK_ARG(rows > 0 && c > 0 && min_rows >= 0 && out5, "cn_chan_slices_plan: bad args");
    const ChanSlicesPlan p = chan_slices_plan((long)rows, c % 4 == 0 ? c / 4 : c, min_rows);
    CN_CHECK_ARG(p.per_slice <= 0x7fffffffL, "cn_chan_slices_plan: %ld rows per slice do not fit the report", p.per_slice);
    const int v[5] = {p.TX, p.TY, p.cb, p.slices, (int)p.per_slice};
    for (int i = 0; i < 5; ++i) out5[i] = v[i];
    return CN_OK;
}

extern "C" int cn_bn_train_bwd_reduce(const float* gy, const float* y, const float* x, const float* mean, const float* r, float* part,
                                      int slices, long long m, int c, int act, void* stream) {
    CN_CHECK_ARG(gy && x && mean && r && part, "cn_bn_train_bwd_reduce: NULL");
    CN_CHECK_ARG(m > 0 && c > 0, "cn_bn_train_bwd_reduce: bad extents m %lld c %d", m, c);
    CN_CHECK_ARG(act == CN_ACT_NONE || (act == CN_ACT_RELU6 && y), "cn_bn_train_bwd_reduce: activation %d (ReLU6 needs y)", act);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = c % 4 == 0;
    const ChanSlicesPlan p = chan_slices_plan((long)m, v4 ? c / 4 : c, 0);
    CN_CHECK_ARG(slices == p.slices, "cn_bn_train_bwd_reduce: %d slices given, the plan has %d (cn_bn_train_bwd_slices)", slices, p.slices);
    if (v4) {
        CN_CHECK_ARG(aligned16(gy, x, y, mean, r),
                     "cn_bn_train_bwd_reduce: operands must be 16-byte aligned when c %% 4 == 0");
        hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<4>, dim3(p.cb, p.slices), dim3(256), 0, s, gy, y, x, mean, r, part, (long)m, c,
                           p.per_slice, p.TX, p.TY, act);
    } else {
        hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<1>, dim3(p.cb, p.slices), dim3(256), 0, s, gy, y, x, mean, r, part, (long)m, c,
                           p.per_slice, p.TX, p.TY, act);
    }
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_bn_train_bwd_apply(const float* gy, const float* y, const float* x, const float* mean, const float* r, const float* a,
                                     const float* sums, float* gx, long long m, int c, int act, void* stream) {
    CN_CHECK_ARG(gy && x && mean && r && a && sums && gx, "cn_bn_train_bwd_apply: NULL");
    CN_CHECK_ARG(m > 0 && c > 0, "cn_bn_train_bwd_apply: bad extents m %lld c %d", m, c);
    CN_CHECK_ARG(act == CN_ACT_NONE || (act == CN_ACT_RELU6 && y), "cn_bn_train_bwd_apply: activation %d (ReLU6 needs y)", act);
    hipStream_t s = (hipStream_t)stream;
    const float inv_m = 1.f / (float)m;
    const EwShape e = ew_shape((long)m, c, gy, y, x, mean, r, a, sums, gx);
    if (e.v4) hipLaunchKernelGGL(bn_train_bwd_apply_kernel<4>, dim3(e.blocks), dim3(256), 0, s, gy, y, x, mean, r, a, sums, gx, e.total_g, c, inv_m, act);
    else hipLaunchKernelGGL(bn_train_bwd_apply_kernel<1>, dim3(e.blocks), dim3(256), 0, s, gy, y, x, mean, r, a, sums, gx, e.total_g, c, inv_m, act);
    CN_LAUNCH_CHECK();
    return CN_OK;
}
