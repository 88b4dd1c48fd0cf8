// chan_slices.h -- what the per-channel training reductions share (depthwise.hip: dwconv3x3_wgrad_kernel, bn_train.hip:
// bn_train_bwd_reduce_kernel): the rows of an (rows, c) NHWC view summed into K numbers per channel, without atomics.
// 256 threads as TX channel groups x TY row lanes (TX = the channel groups rounded up to a power of two, 64 at most: lanes of a wave
// on consecutive channel groups, coalesced rows); a workgroup owns a SLICE of consecutive rows, lane ty walks the rows ty, ty + TY, ...
// of it with K x V accumulators in registers and the workgroup leaves K x C partials (chan_lanes_sum).  The caller adds the slices in
// slice order (cn_sum_rows_into, or the grouped reduction at the join of a backward pass): the same bits in every mode.
#pragma once
#include "common.h"

// V consecutive floats as one access (V = 4: a float4, the pointer 16-byte aligned) or a scalar
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

template <typename... P>
inline bool aligned16(const P*... p) { return (((uintptr_t)p | ...) % 16) == 0; }       // (NULL counts as aligned)

// The slice rule.  A slice costs K C floats written and read again next to its rows of operands, so one slice per min_rows rows
// (the depthwise filter gradient: 64, about 7 % extra traffic for its 9 C floats; BatchNormalization: no floor of its own) and per
// 4 rows of every lane, whichever is more rows; at most 1024 workgroups (4 per compute unit); the rows then evened out over the
// slices.  Batch 32, depthwise: the 7 x 7 x 960 layer (1568 pixels, TX 64, TY 4, 4 channel blocks) gets 25 slices of 63 pixels, 100
// workgroups of 16 pixels per lane; the 128 x 128 x 32 layer (524 288 pixels, TX 8, TY 32, one channel block) gets 1024 slices of 512.
struct ChanSlicesPlan {
    int TX, TY, cb, slices;        // cb: channel blocks of TX groups; the grid is (cb, slices)
    long per_slice;                // rows of a slice (the last one may hold fewer)
};

inline ChanSlicesPlan chan_slices_plan(long rows, int cgs, long min_rows) {
    ChanSlicesPlan p;
    p.TX = 1;
    while (p.TX < cgs && p.TX < 64) p.TX *= 2;
    p.TY = 256 / p.TX;
    p.cb = cn_cdiv(cgs, p.TX);
    const long least = 4L * p.TY > min_rows ? 4L * p.TY : min_rows;
    long slices = (rows + least - 1) / least;
    const long cap = 1024 / p.cb > 1 ? 1024 / p.cb : 1;
    if (slices > cap) slices = cap;
    p.per_slice = (rows + slices - 1) / slices;
    p.slices = (int)((rows + p.per_slice - 1) / p.per_slice);
    return p;
}

// The lane combine at the end of such a kernel (every thread calls it; red: K * 256 * V floats of LDS).  Every lane stores its
// accumulators as red[k][ty][tx] (consecutive lanes -> consecutive float4: ds_write_b128 without bank conflicts); after the barrier thread
// o sums the TY entries of output (k, channel) = o in ty order (consecutive threads on consecutive dwords) into part[slice][k][channel].
template <int K, int V>
__device__ __forceinline__ void chan_lanes_sum(const float (&acc)[K][V], float* red, float* part, int c, int TX, int TY) {
#pragma unroll
    for (int k = 0; k < K; ++k) VecIO<V>::st(red + ((long)k * 256 + threadIdx.x) * V, acc[k]);
    __syncthreads();
    const int W = TX * V;                              // channels of this workgroup
    for (int o = threadIdx.x; o < K * W; o += 256) {
        const int k = o / W, cl = o - k * W;
        float s = 0.f;
        for (int q = 0; q < TY; ++q) s += red[(k * TY + q) * W + cl];
        const int co = blockIdx.x * W + cl;
        if (co < c) part[((long)blockIdx.y * K + k) * c + co] = s;
    }
}
