// typed.h -- storage-type helpers: activations live in HBM as fp32 (CN_F32) or bf16 (CN_BF16); arithmetic,
// statistics, coefficients, loss sums, gradients of parameters and optimizer state are always fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned short bf16_t;                  // raw bfloat16 bits

__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ bf16_t f32_to_bf16(float x) {       // round to nearest even (NaN stays NaN)
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40u);
    return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    return (unsigned)f32_to_bf16(lo) | ((unsigned)f32_to_bf16(hi) << 16);
}

// scalar / 4-wide loads and stores of a tensor stored as T (float or bf16_t); the 4-wide forms need
// 4*sizeof(T)-byte alignment
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }

template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }

template <typename T> __device__ __forceinline__ float4 ld4(const T* p);
template <> __device__ __forceinline__ float4 ld4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 ld4<bf16_t>(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}

template <typename T> __device__ __forceinline__ void st4(T* p, float4 v);
template <> __device__ __forceinline__ void st4<float>(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
template <> __device__ __forceinline__ void st4<bf16_t>(bf16_t* p, float4 v) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}

// AdaIn's variance where the one-pass form fails.  s2 / S - mu^2 from fp32 sums carries an absolute error of ~2e-6 mu^2 (measured:
// 2.2e-5 at mu = 3.7, S = 4096) whatever produced the sums (cn_nc_reduce or a convolution epilogue); AdaIn adds eps under the
// root, so that error matters once it is no longer small against var + eps -- an almost constant channel with a large mean.
// cn_adain_refine() says when: mu^2 > 1000 (var + eps), a mean above ~31 standard deviations; below it the residue stays under
// 2e-3 of var + eps, i.e. 1e-3 of r = rsqrt(var + eps).  cn_var_two_pass() then takes mean((x - mu)^2) of one (sample, channel)
// again from the tensor, one thread, fixed order: both users (norm_coef_fwd_kernel, norm_apply_rows_kernel) get the same bits.
// A thread that meets the condition walks S strided elements.
__device__ __forceinline__ bool cn_adain_refine(float mu, float var, float eps) { return mu * mu > 1000.f * (var + eps); }
template <typename T>
__device__ __forceinline__ float cn_var_two_pass(const T* __restrict__ x, int S, int C, float mu, float invS) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 3 < S; s += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float d = ldf<T>(x + (long)(s + u) * C) - mu;
            acc[u] = fmaf(d, d, acc[u]);
        }
    }
    for (; s < S; ++s) {
        const float d = ldf<T>(x + (long)s * C) - mu;
        acc[0] = fmaf(d, d, acc[0]);
    }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) * invS;
}

// runtime dispatch on the dtype code of the C ABI
#define CN_DISPATCH_DT(dt, ...)                                     \
    do {                                                            \
        if ((dt) == CN_BF16) { typedef bf16_t T; __VA_ARGS__; }     \
        else { typedef float T; __VA_ARGS__; }                      \
    } while (0)
