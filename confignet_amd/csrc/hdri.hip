// hdri.hip -- the image side of the HDRI environment-map PCA encoding (confignet_amd/hdri.py; reference: hdri_encoding/
// hdri_pca_model.py): log2(x + 1), a rotation about the vertical axis (np.roll along the columns by a whole number of
// columns) and cv2.resize(INTER_AREA) to the model's shape, for many (image, rotation) samples drawn from a small pool of images.
//
// The roll only moves columns, so the vertical half of the area resize does not depend on the rotation:
//   cn_hdri_rows_v   once per POOL image:  v[p][o][j]    = sum_t wy[o][t] log2f(x[p][y0[o] + t][j] + 1),   j over the W 3 floats of a row
//   cn_hdri_rows_h   once per SAMPLE:      r[n][o][q][c] = sum_t wx[q][t] v[idx[n]][o][(x0[q] + t - shift[n]) mod W][c]  (- mean[o][q][c])
// For 1024 x 2048 -> 64 x 128 that reads each 25 MB image once and then 1.5 MB per sample instead of 25 MB per sample.  Both kernels
// are plain streaming code (HBM / L2 bound, a handful of flops per float); the sums run over t in index order with one fused
// multiply-add per term, so equal weights on equal values give bit-identical results whatever the shift.
//
// The area tables (first source index and T weights per output index, overlap / scale, zero padded) come from the host
// (hdri.py: area_table).  A term whose weight is zero or whose source index falls outside the image is skipped, so no table
// content can make a kernel read out of bounds.
#include "common.h"

namespace {

// One thread: 4 consecutive floats of one output row.  VEC: W 3 is a multiple of 4 and both base pointers are 16-byte aligned,
// so every row starts on a 16-byte boundary -> float4 loads and stores.  Otherwise the rows of an image sit at different
// offsets modulo 16 bytes and no column group is aligned in all of them: scalar loads (still coalesced), the last group of a row
// guarded element by element.
template <bool VEC>
__global__ __launch_bounds__(256) void hdri_rows_v_kernel(const float* __restrict__ x, float* __restrict__ v, const int* __restrict__ y0,
                                                          const float* __restrict__ wy, int h, int w3, int oh, int t_len) {
    const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= w3) return;
    const int o = blockIdx.y;
    const int64_t p = blockIdx.z;
    const float* src = x + p * h * (int64_t)w3 + j;
    const int first = y0[o];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < t_len; ++t) {
        const float wt = wy[o * t_len + t];
        const int y = first + t;
        if (wt == 0.f || y < 0 || y >= h) continue;
        const float* row = src + (int64_t)y * w3;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 q = *reinterpret_cast<const float4*>(row);
            a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < w3) a[e] = row[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(wt, log2f(a[e] + 1.f), acc[e]);
    }
    float* dst = v + (p * oh + o) * (int64_t)w3 + j;
    if (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < w3) dst[e] = acc[e];
    }
}

// One thread: one output float (sample n = blockIdx.z, output row o = blockIdx.y, q 3 + c along x).
__global__ __launch_bounds__(256) void hdri_rows_h_kernel(const float* __restrict__ v, float* __restrict__ out, const int* __restrict__ idx,
                                                          const int* __restrict__ shift, const int* __restrict__ x0,
                                                          const float* __restrict__ wx, const float* __restrict__ mean, int pool, int w,
                                                          int oh, int ow, int t_len) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ow * 3) return;
    const int q = e / 3, c = e - q * 3;
    const int o = blockIdx.y;
    const int64_t n = blockIdx.z;
    float* dst = out + (n * oh + o) * (int64_t)ow * 3 + e;
    const int p = idx[n];
    if (p < 0 || p >= pool) {          // no image to read: mark the sample instead of reading out of bounds
        *dst = __builtin_nanf("");
        return;
    }
    int s = shift[n] % w;              // C remainder: sign of the dividend; |s| < w afterwards
    if (s < 0) s += w;
    const float* row = v + ((int64_t)p * oh + o) * (int64_t)w * 3 + c;
    const int first = x0[q];
    float acc = 0.f;
    for (int t = 0; t < t_len; ++t) {
        const float wt = wx[q * t_len + t];
        const int xs = first + t;      // column of the ROTATED image; np.roll: rotated[x] = image[(x - shift) mod w]
        if (wt == 0.f || xs < 0 || xs >= w) continue;
        int col = xs - s;
        if (col < 0) col += w;
        acc = fmaf(wt, row[(int64_t)col * 3], acc);
    }
    if (mean) acc -= mean[((int64_t)o * ow) * 3 + e];
    *dst = acc;
}

__global__ __launch_bounds__(256) void exp2m1_kernel(const float* __restrict__ x, float* __restrict__ y, size_t numel) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < numel) y[i] = exp2f(x[i]) - 1.f;
}

// T weights per output index cover every source cell an interval of length in / out can touch: ceil(in / out) + 1
bool table_len_ok(int in, int out, int t_len) { return t_len >= (in + out - 1) / out + 1; }

}  // namespace

extern "C" int cn_hdri_rows_v(const float* x, float* v, const int* y0, const float* wy, int pool, int h, int w, int oh, int t_len,
                              void* stream) {
    CN_CHECK_ARG(x && v && y0 && wy, "cn_hdri_rows_v: NULL");
    CN_CHECK_ARG(pool > 0 && h > 0 && w > 0 && oh > 0 && t_len > 0, "cn_hdri_rows_v: bad extents");
    CN_CHECK_ARG(oh <= h, "cn_hdri_rows_v: %d -> %d rows enlarges (area resize only shrinks)", h, oh);
    CN_CHECK_ARG(table_len_ok(h, oh, t_len), "cn_hdri_rows_v: %d weights per row are too few for %d -> %d", t_len, h, oh);
    CN_CHECK_ARG(pool <= 65535 && oh <= 65535 && (long)w * 3 < 0x7fffffffL, "cn_hdri_rows_v: extents exceed the launch grid");
    const int w3 = w * 3;
    const dim3 grid(cn_cdiv(cn_cdiv(w3, 4), 256), oh, pool);
    const bool vec = w3 % 4 == 0 && ((uintptr_t)x | (uintptr_t)v) % 16 == 0;
    if (vec) hipLaunchKernelGGL(hdri_rows_v_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, v, y0, wy, h, w3, oh, t_len);
    else hipLaunchKernelGGL(hdri_rows_v_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, v, y0, wy, h, w3, oh, t_len);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_hdri_rows_h(const float* v, float* out, const int* idx, const int* shift, const int* x0, const float* wx,
                              const float* mean, int n, int pool, int w, int oh, int ow, int t_len, void* stream) {
    CN_CHECK_ARG(v && out && idx && shift && x0 && wx, "cn_hdri_rows_h: NULL");
    CN_CHECK_ARG(n > 0 && pool > 0 && w > 0 && oh > 0 && ow > 0 && t_len > 0, "cn_hdri_rows_h: bad extents");
    CN_CHECK_ARG(ow <= w, "cn_hdri_rows_h: %d -> %d columns enlarges (area resize only shrinks)", w, ow);
    CN_CHECK_ARG(table_len_ok(w, ow, t_len), "cn_hdri_rows_h: %d weights per column are too few for %d -> %d", t_len, w, ow);
    CN_CHECK_ARG(n <= 65535 && oh <= 65535 && (long)w * 3 < 0x7fffffffL, "cn_hdri_rows_h: extents exceed the launch grid");
    const dim3 grid(cn_cdiv((long)ow * 3, 256), oh, n);
    hipLaunchKernelGGL(hdri_rows_h_kernel, grid, dim3(256), 0, (hipStream_t)stream, v, out, idx, shift, x0, wx, mean, pool, w, oh, ow,
                       t_len);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_exp2m1(const float* x, float* y, size_t numel, void* stream) {
    CN_CHECK_ARG(x && y, "cn_exp2m1: NULL");
    if (numel == 0) return CN_OK;
    const size_t blocks = (numel + 255) / 256;
    CN_CHECK_ARG(blocks < 0x7fffffffUL, "cn_exp2m1: tensor too large");
    hipLaunchKernelGGL(exp2m1_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, numel);
    CN_LAUNCH_CHECK();
    return CN_OK;
}
