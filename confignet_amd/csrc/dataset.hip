// dataset.hip -- the image side of dataset creation (confignet_amd/face_image_normalizer.py, neural_renderer_dataset.py; reference:
// confignet/face_image_normalizer.py:113-126, neural_renderer_dataset.py:241-255): cv2.warpAffine of uint8 pictures (bilinear,
// BORDER_CONSTANT 0) and of float32 UV maps (INTER_NEAREST), and the eye-region mask of a warped UV map.
//
// cv2 does the coordinate arithmetic of warpAffine in double on the host and keeps it as int32 tables with 10 fractional bits: per
// output column adelta[x] = rint(M0 x 1024), bdelta[x] = rint(M3 x 1024), per output row X0[y] = rint((M1 y + M2) 1024) + delta,
// Y0[y] likewise (delta 16 for bilinear, 512 for nearest).  face_image_normalizer.py: affine_tables builds the same tables, one set per
// image, so the kernels below are integer-only (the nearest one a pure gather) and equal the numpy statement bit for bit:
//   bilinear  X = (X0[y] + adelta[x]) >> 5; sx = X >> 5, ax = X & 31 (likewise Y, sy, ay); the four taps (sy, sx) .. (sy + 1, sx + 1) with
//             the weights 32 (32 - ax)(32 - ay), 32 ax (32 - ay), 32 (32 - ax) ay, 32 ax ay (they sum to 32768); (sum + 16384) >> 15
//   nearest   sx = (X0[y] + adelta[x]) >> 10, sy likewise; the source value, 0.0 outside
// The sum of two table entries is taken in 64 bits and every tap is tested against the source extents, so no table content (INT32_MAX,
// INT32_MIN) overflows or reads outside the source.  Plain streaming code: one thread per output pixel, consecutive lanes write
// consecutive pixels of a row; the reads are a gather whose neighbours in a row are neighbours in the source for any similarity.
// 4-channel pixels move as one dword; 3-channel pixels as bytes, the wave's stores still contiguous: 64 pictures 1024^2 -> 1024^2 take
// 0.49 ms (0.8 TB/s of pixels read once and written once), 250 times the rate at which 16 threads decode the files they come from
// (profiles/dataset_creation.txt), so nothing wider is attempted.  18 - 26 VGPRs, no scratch, 8 waves per SIMD.
// That covers the uint8 kernel.  The nearest-neighbour kernel walks a runtime channel count with one dword store per channel, so for
// 3 channels a wave's stores are strided by 12 bytes (each cache line is still written whole by the wave); at 3 000 UV maps per second
// with its copies, against 300 decoded per second, it bounds nothing either and is left plain.
#include "common.h"

namespace {

struct Tables {
    const int* x0;      // (n, oh)
    const int* y0;      // (n, oh)
    const int* adelta;  // (n, ow)
    const int* bdelta;  // (n, ow)
};

// C interleaved uint8 channels of one tap; 0 outside the source.  C == 4: one aligned dword load.
template <int C>
__device__ __forceinline__ void load_tap(const uint8_t* __restrict__ img, int sh, int sw, long long sy, long long sx, int p[C]) {
    if (sx < 0 || sx >= sw || sy < 0 || sy >= sh) {
#pragma unroll
        for (int k = 0; k < C; ++k) p[k] = 0;
        return;
    }
    const uint8_t* q = img + ((int64_t)sy * sw + sx) * C;
    if constexpr (C == 4) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(q);
        p[0] = v & 255; p[1] = (v >> 8) & 255; p[2] = (v >> 16) & 255; p[3] = v >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) p[k] = q[k];
    }
}

template <int C>
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, Tables t, int sh,
                                                             int sw, int oh, int ow) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= ow) return;
    const int y = blockIdx.y;
    const int64_t n = blockIdx.z;
    const long long X = ((long long)t.x0[n * oh + y] + t.adelta[n * ow + x]) >> 5;
    const long long Y = ((long long)t.y0[n * oh + y] + t.bdelta[n * ow + x]) >> 5;
    const long long sx = X >> 5, sy = Y >> 5;
    const int ax = (int)(X & 31), ay = (int)(Y & 31);
    const uint8_t* img = src + n * sh * (int64_t)sw * C;
    int p00[C], p01[C], p10[C], p11[C];
    load_tap<C>(img, sh, sw, sy, sx, p00);
    load_tap<C>(img, sh, sw, sy, sx + 1, p01);
    load_tap<C>(img, sh, sw, sy + 1, sx, p10);
    load_tap<C>(img, sh, sw, sy + 1, sx + 1, p11);
    const int w00 = 32 * (32 - ax) * (32 - ay), w01 = 32 * ax * (32 - ay), w10 = 32 * (32 - ax) * ay, w11 = 32 * ax * ay;
    int r[C];
#pragma unroll
    for (int k = 0; k < C; ++k) r[k] = (w00 * p00[k] + w01 * p01[k] + w10 * p10[k] + w11 * p11[k] + 16384) >> 15;   // <= 255
    uint8_t* o = dst + ((n * oh + y) * (int64_t)ow + x) * C;
    if constexpr (C == 4) {
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = (uint8_t)r[k];
    }
}

__global__ __launch_bounds__(256) void warp_nearest_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, Tables t, int sh, int sw,
                                                               int oh, int ow, int c) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= ow) return;
    const int y = blockIdx.y;
    const int64_t n = blockIdx.z;
    const long long sx = ((long long)t.x0[n * oh + y] + t.adelta[n * ow + x]) >> 10;
    const long long sy = ((long long)t.y0[n * oh + y] + t.bdelta[n * ow + x]) >> 10;
    const bool inside = sx >= 0 && sx < sw && sy >= 0 && sy < sh;
    const float* q = src + ((n * sh + (inside ? sy : 0)) * (int64_t)sw + (inside ? sx : 0)) * c;
    float* o = dst + ((n * oh + y) * (int64_t)ow + x) * c;
    for (int k = 0; k < c; ++k) o[k] = inside ? q[k] : 0.f;
}

// mask = 1 where (u, v) = the first two channels of a pixel lie strictly inside the left or the right eye rectangle
__global__ __launch_bounds__(256) void eye_mask_kernel(const float* __restrict__ uv, uint8_t* __restrict__ mask, size_t pixels, int c,
                                                       float l_min, float l_max, float r_min, float r_max, float y_min, float y_max) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const float u = uv[i * c], v = uv[i * c + 1];
    const bool in_y = v < y_max && v > y_min;
    const bool left = u < l_max && u > l_min, right = u < r_max && u > r_min;
    mask[i] = (in_y && (left || right)) ? 1 : 0;
}

bool extents_ok(int n, int sh, int sw, int oh, int ow) {
    // cv2 keeps source coordinates as int16: a source beyond 32767 would behave differently there
    return n > 0 && sh > 0 && sw > 0 && oh > 0 && ow > 0 && n <= 65535 && oh <= 65535 && sh <= 32767 && sw <= 32767;
}

}  // namespace

extern "C" int cn_warp_affine_u8(const uint8_t* src, uint8_t* dst, const int* x0, const int* y0, const int* adelta, const int* bdelta,
                                 int n, int sh, int sw, int c, int oh, int ow, void* stream) {
    CN_CHECK_ARG(src && dst && x0 && y0 && adelta && bdelta, "cn_warp_affine_u8: NULL");
    CN_CHECK_ARG(extents_ok(n, sh, sw, oh, ow), "cn_warp_affine_u8: bad extents %d x (%d, %d) -> (%d, %d)", n, sh, sw, oh, ow);
    CN_CHECK_ARG(c >= 1 && c <= 4, "cn_warp_affine_u8: %d channels (1 .. 4)", c);
    const Tables t{x0, y0, adelta, bdelta};
    const dim3 grid(cn_cdiv(ow, 256), oh, n);
    const hipStream_t s = (hipStream_t)stream;
    // 4 channels move as one dword per pixel: the images must sit on 4-byte boundaries (any tensor allocation does)
    CN_CHECK_ARG(c != 4 || ((uintptr_t)src | (uintptr_t)dst) % 4 == 0, "cn_warp_affine_u8: 4-channel images must be 4-byte aligned");
    if (c == 4) hipLaunchKernelGGL(warp_affine_u8_kernel<4>, grid, dim3(256), 0, s, src, dst, t, sh, sw, oh, ow);
    else if (c == 3) hipLaunchKernelGGL(warp_affine_u8_kernel<3>, grid, dim3(256), 0, s, src, dst, t, sh, sw, oh, ow);
    else if (c == 2) hipLaunchKernelGGL(warp_affine_u8_kernel<2>, grid, dim3(256), 0, s, src, dst, t, sh, sw, oh, ow);
    else hipLaunchKernelGGL(warp_affine_u8_kernel<1>, grid, dim3(256), 0, s, src, dst, t, sh, sw, oh, ow);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_warp_nearest_f32(const float* src, float* dst, const int* x0, const int* y0, const int* adelta, const int* bdelta,
                                   int n, int sh, int sw, int c, int oh, int ow, void* stream) {
    CN_CHECK_ARG(src && dst && x0 && y0 && adelta && bdelta, "cn_warp_nearest_f32: NULL");
    CN_CHECK_ARG(extents_ok(n, sh, sw, oh, ow), "cn_warp_nearest_f32: bad extents %d x (%d, %d) -> (%d, %d)", n, sh, sw, oh, ow);
    CN_CHECK_ARG(c >= 1 && c <= 4, "cn_warp_nearest_f32: %d channels (1 .. 4)", c);
    const Tables t{x0, y0, adelta, bdelta};
    hipLaunchKernelGGL(warp_nearest_f32_kernel, dim3(cn_cdiv(ow, 256), oh, n), dim3(256), 0, (hipStream_t)stream, src, dst, t, sh, sw, oh,
                       ow, c);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

extern "C" int cn_eye_mask(const float* uv, uint8_t* mask, size_t pixels, int c, float l_min, float l_max, float r_min, float r_max,
                           float y_min, float y_max, void* stream) {
    CN_CHECK_ARG(uv && mask, "cn_eye_mask: NULL");
    CN_CHECK_ARG(c >= 2, "cn_eye_mask: %d channels (the test reads the first two)", c);
    if (pixels == 0) return CN_OK;
    const size_t blocks = (pixels + 255) / 256;
    CN_CHECK_ARG(blocks < 0x7fffffffUL, "cn_eye_mask: tensor too large");
    hipLaunchKernelGGL(eye_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, uv, mask, pixels, c, l_min, l_max,
                       r_min, r_max, y_min, y_max);
    CN_LAUNCH_CHECK();
    return CN_OK;
}
