// gemm.hip -- dense GEMM  C = act(op(A) op(B) + bias)  for the Keras Dense layers of the path
// (AdaIN MLPs, discriminator heads, latent regressor head, latent discriminator, synthetic
// encoder, RealEncoder heads, LatentGAN).  Arbitrary M/N/K/ld (e.g. latent_dim = 145), so the
// loaders are guarded scalar loads; the multiply is the same 32x32x2 f32 MFMA tile as the
// convolutions (64x64 tile, 4 waves).  Skinny problems with a long K (32768 -> 148 at M = batch)
// are split over K across workgroups and combined with fp32 atomics.
#include "common.h"
#include "mma_tile.h"
#include <stdlib.h>

namespace {

__global__ __launch_bounds__(256) void gemm_kernel(int ta, int tb, int M, int N, int K, const float* __restrict__ A,
                                                   int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
                                                   int ldc, const float* __restrict__ bias, int act, float slope,
                                                   int k_per_split, int splitk, float* __restrict__ parts = nullptr) {
    constexpr int BM = 64, BN = 64, LDA = BM + 4, LDB = BN + 4;
    __shared__ float As[2][BK][LDA];
    __shared__ float Bs[2][BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kbeg = blockIdx.z * k_per_split, kend = min(K, kbeg + k_per_split);
    if (kbeg >= kend) return;

    f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    float ra[4], rb[4];
    const int q4 = tid & 3, r64 = tid >> 2;      // (4 consecutive k, row) mapping
    const int q16 = tid & 15, r16 = tid >> 4;    // (4 consecutive m/n, k row) mapping

    auto load_tiles = [&](int k0) {
        if (!ta) {
            const int m = m0 + r64;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + q4 * 4 + e;
                ra[e] = (m < M && k < kend) ? A[(long)m * lda + k] : 0.f;
            }
        } else {
            const int k = k0 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + q16 * 4 + e;
                ra[e] = (m < M && k < kend) ? A[(long)k * lda + m] : 0.f;
            }
        }
        if (!tb) {
            const int k = k0 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = n0 + q16 * 4 + e;
                rb[e] = (n < N && k < kend) ? B[(long)k * ldb + n] : 0.f;
            }
        } else {
            const int n = n0 + r64;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + q4 * 4 + e;
                rb[e] = (n < N && k < kend) ? B[(long)n * ldb + k] : 0.f;
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!ta) As[buf][q4 * 4 + e][r64] = ra[e];
            else As[buf][r16][q16 * 4 + e] = ra[e];
            if (!tb) Bs[buf][r16][q16 * 4 + e] = rb[e];
            else Bs[buf][q4 * 4 + e][r64] = rb[e];
        }
    };

    const int nks = (kend - kbeg + BK - 1) / BK;
    load_tiles(kbeg);
    store_tiles(0);
    __syncthreads();
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nks) load_tiles(kbeg + (ks + 1) * BK);
        mma_step<1, 1, LDA, LDB>(As[buf], Bs[buf], acc, wm * 32 + l31, wn * 32 + l31, half);
        if (ks + 1 < nks) store_tiles(buf ^ 1);
        __syncthreads();
    }

    const int col = n0 + wn * 32 + l31;
    if (col >= N) return;
    const float bv = (bias && blockIdx.z == 0) ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + 4 * half + (r & 3) + 8 * (r >> 2);
        if (row >= M) continue;
        const float v = acc[0][0][r] + bv;
        if (parts) parts[((long)blockIdx.z * M + row) * N + col] = v;      // deterministic mode: per-split slabs, added in order afterwards
        else if (splitk > 1) unsafeAtomicAdd(&C[(long)row * ldc + col], v);
        else C[(long)row * ldc + col] = cn_apply_act(v, act, slope);
    }
}

// Dense layers with <= 4 outputs and few rows (discriminator / rotation heads: M = batch, N = 1 or 3, K up to 32768): a
// 64x64 MFMA tile would walk the whole K in ONE workgroup (120 us for K = 2048).  One workgroup per (row, K slice)
// instead: 256 lanes stride K, wave shuffles + LDS combine.  bias/act need the full sum, so slices > 1 only without act.
__global__ __launch_bounds__(256) void thin_gemm_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                        const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                                        const float* __restrict__ bias, int act, float slope, int kps) {
    const int m = blockIdx.x;
    const int kbeg = blockIdx.y * kps, kend = min(K, kbeg + kps);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* ar = A + (long)m * lda;
    for (int k = kbeg + threadIdx.x; k < kend; k += 256) {
        const float av = ar[k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < N) acc[j] += av * B[(long)k * ldb + j];
    }
    __shared__ float red[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = acc[j];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int j = threadIdx.x;
        const float v = red[0][j] + red[1][j] + red[2][j] + red[3][j];
        if (gridDim.y > 1) unsafeAtomicAdd(&C[(long)m * ldc + j], v + ((bias && blockIdx.y == 0) ? bias[j] : 0.f));
        else C[(long)m * ldc + j] = cn_apply_act(v + (bias ? bias[j] : 0.f), act, slope);
    }
}

// ---------------------------------------------------------------------------------------------
// Small dense layers (round 3).  The path's Dense layers run at M = batch (8 / 16 rows): AdaIN MLPs 145 -> 128 -> 2C, the
// synthetic encoder's 24 per-input layers, the latent discriminator, heads.  ~360 launches per training iteration went
// through the 64 x 64 MFMA tile above, which walks K in 16-deep stages with one global round trip per stage: 10 us for a
// 16 x 145 x 128 product whose arithmetic is nothing.  These kernels issue every load up front instead.
//   row-skinny (M <= 32; C = A op(B)): the whole A block sits in LDS, a thread owns one output column and a quarter of K
//     (M accumulators), the four K quarters are combined through LDS;
//   depth-skinny (K <= 32; C (+)= A^T B, the weight gradient x^T gy of such a layer): a thread owns 4 rows x 1 column.
// ---------------------------------------------------------------------------------------------
template <int MT, bool TB>
__global__ __launch_bounds__(256) void gemm_rows_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                        const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                                        const float* __restrict__ bias, int act, float slope) {
    extern __shared__ float sm[];                 // A block [MT][K] (rows >= M are zero), then the partial sums [3][MT][64]
    float* As = sm;
    float* red = sm + MT * K;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    for (int i = tid; i < MT * K; i += 256) {
        const int m = i / K, k = i - m * K;
        As[i] = m < M ? A[(long)m * lda + k] : 0.f;
    }
    __syncthreads();
    const int n = blockIdx.x * 64 + c;
    const int kq = (K + 3) / 4, kbeg = q * kq, kend = min(K, kbeg + kq);
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    if (n < N) {
#pragma unroll 4
        for (int k = kbeg; k < kend; ++k) {
            const float b = TB ? B[(long)n * ldb + k] : B[(long)k * ldb + n];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] += As[m * K + k] * b;
        }
    }
    if (q > 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) red[((q - 1) * MT + m) * 64 + c] = acc[m];
    }
    __syncthreads();
    if (q == 0 && n < N) {
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float v = acc[m] + red[(0 * MT + m) * 64 + c] + red[(1 * MT + m) * 64 + c] + red[(2 * MT + m) * 64 + c] + bv;
            if (m < M) C[(long)m * ldc + n] = cn_apply_act(v, act, slope);
        }
    }
}

__global__ __launch_bounds__(256) void gemm_depth_kernel(int M, int N, int K, const float* __restrict__ A, int lda,
                                                         const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                                         int accumulate) {
    // C[m][n] (+)= sum_k A[k][m] B[k][n], K <= 32.  Workgroup tile: 16 rows x 64 columns.
    __shared__ float As[32][16];
    __shared__ float Bs[32][64];
    const int tid = threadIdx.x, c = tid & 63, r = tid >> 6;
    const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 64;
    for (int i = tid; i < K * 16; i += 256) {
        const int k = i >> 4, m = i & 15;
        As[k][m] = (m0 + m < M) ? A[(long)k * lda + m0 + m] : 0.f;
    }
    for (int i = tid; i < K * 64; i += 256) {
        const int k = i >> 6, nn = i & 63;
        Bs[k][nn] = (n0 + nn < N) ? B[(long)k * ldb + n0 + nn] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        const float b = Bs[k][c];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += As[k][r * 4 + e] * b;
    }
    const int n = n0 + c;
    if (n >= N) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int m = m0 + r * 4 + e;
        if (m >= M) continue;
        if (accumulate) unsafeAtomicAdd(&C[(long)m * ldc + n], acc[e]);
        else C[(long)m * ldc + n] = acc[e];
    }
}

// ---- many shallow weight-gradient products in ONE launch (round 6): C_j += A_j^T B_j with K_j <= 32 rows -- the dense layers'
// weight gradients of a backward pass (batch <= 32 samples: the AdaIN MLPs, the encoders' and the regressor's dense layers) are
// leaves of the tape; the pass queues them and launches them together at its join.  Per job exactly gemm_depth_kernel's arithmetic.
constexpr int CN_DEPTH_GROUP = 64;
struct DepthJobs {
    const float* a[CN_DEPTH_GROUP];
    const float* b[CN_DEPTH_GROUP];
    float* c[CN_DEPTH_GROUP];
    int m[CN_DEPTH_GROUP], n[CN_DEPTH_GROUP], k[CN_DEPTH_GROUP], lda[CN_DEPTH_GROUP], ldb[CN_DEPTH_GROUP], ldc[CN_DEPTH_GROUP];
    int blk0[CN_DEPTH_GROUP + 1];
    int count;
};

__global__ __launch_bounds__(256) void gemm_depth_grouped_kernel(DepthJobs J) {
    __shared__ float As[32][16];
    __shared__ float Bs[32][64];
    const int bid = blockIdx.x;
    int lo = 0, hi = J.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.blk0[mid] <= bid) lo = mid;
        else hi = mid;
    }
    const int j = __builtin_amdgcn_readfirstlane(lo), lb = bid - J.blk0[j];
    const int M = J.m[j], N = J.n[j], K = J.k[j], lda = J.lda[j], ldb = J.ldb[j], ldc = J.ldc[j];
    const float* __restrict__ A = J.a[j];
    const float* __restrict__ B = J.b[j];
    float* __restrict__ C = J.c[j];
    const int tx = (M + 15) / 16;
    const int tid = threadIdx.x, c = tid & 63, r = tid >> 6;
    const int m0 = (lb % tx) * 16, n0 = (lb / tx) * 64;
    for (int i = tid; i < K * 16; i += 256) {
        const int k = i >> 4, m = i & 15;
        As[k][m] = (m0 + m < M) ? A[(long)k * lda + m0 + m] : 0.f;
    }
    for (int i = tid; i < K * 64; i += 256) {
        const int k = i >> 6, nn = i & 63;
        Bs[k][nn] = (n0 + nn < N) ? B[(long)k * ldb + n0 + nn] : 0.f;
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        const float b = Bs[k][c];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += As[k][r * 4 + e] * b;
    }
    const int n = n0 + c;
    if (n >= N) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int m = m0 + r * 4 + e;
        if (m >= M) continue;
        unsafeAtomicAdd(&C[(long)m * ldc + n], acc[e]);
    }
}

// ---- many row-skinny dense layers in ONE launch (round 6): C_j = epi(A_j op(B_j) + bias_j) with M_j <= 32 rows -- the six AdaIN
// MLPs of a generator pass layer by layer (hologan_generator.py:119-124), forward and data-gradient side.  Per job exactly
// gemm_rows_kernel's arithmetic (K quarters combined in the same order); epi = activation, or (mask != NULL) the product with
// act'(mask) -- the hidden layer's LeakyReLU derivative taken from its stored output --, or (accumulate) an atomic add into C.
constexpr int CN_ROWS_GROUP = 16;
struct RowsJobs {
    const float* a[CN_ROWS_GROUP];
    const float* b[CN_ROWS_GROUP];
    float* c[CN_ROWS_GROUP];
    const float* bias[CN_ROWS_GROUP];
    const float* mask[CN_ROWS_GROUP];
    int m[CN_ROWS_GROUP], n[CN_ROWS_GROUP], k[CN_ROWS_GROUP], lda[CN_ROWS_GROUP], ldb[CN_ROWS_GROUP], ldc[CN_ROWS_GROUP];
    int tb[CN_ROWS_GROUP], act[CN_ROWS_GROUP], accumulate[CN_ROWS_GROUP];
    float slope[CN_ROWS_GROUP];
    int blk0[CN_ROWS_GROUP + 1];
    int count;
};

template <int MT>
__global__ __launch_bounds__(256) void gemm_rows_grouped_kernel(RowsJobs J) {
    extern __shared__ float sm[];                 // A block [MT][K] (rows >= M are zero), then the partial sums [3][MT][64]
    const int bid = blockIdx.x;
    int lo = 0, hi = J.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.blk0[mid] <= bid) lo = mid;
        else hi = mid;
    }
    const int j = __builtin_amdgcn_readfirstlane(lo);
    const int M = J.m[j], N = J.n[j], K = J.k[j], lda = J.lda[j], ldb = J.ldb[j], ldc = J.ldc[j], tb = J.tb[j];
    const float* __restrict__ A = J.a[j];
    const float* __restrict__ B = J.b[j];
    float* __restrict__ C = J.c[j];
    float* As = sm;
    float* red = sm + MT * K;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    for (int i = tid; i < MT * K; i += 256) {
        const int m = i / K, k = i - m * K;
        As[i] = m < M ? A[(long)m * lda + k] : 0.f;
    }
    __syncthreads();
    const int n = (bid - J.blk0[j]) * 64 + c;
    const int kq = (K + 3) / 4, kbeg = q * kq, kend = min(K, kbeg + kq);
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    if (n < N) {
        if (tb) {
#pragma unroll 4
            for (int k = kbeg; k < kend; ++k) {
                const float b = B[(long)n * ldb + k];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] += As[m * K + k] * b;
            }
        } else {
#pragma unroll 4
            for (int k = kbeg; k < kend; ++k) {
                const float b = B[(long)k * ldb + n];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] += As[m * K + k] * b;
            }
        }
    }
    if (q > 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) red[((q - 1) * MT + m) * 64 + c] = acc[m];
    }
    __syncthreads();
    if (q == 0 && n < N) {
        const float bv = J.bias[j] ? J.bias[j][n] : 0.f;
        const float* __restrict__ mask = J.mask[j];
        const int act = J.act[j];
        const float slope = J.slope[j];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float v = acc[m] + red[(0 * MT + m) * 64 + c] + red[(1 * MT + m) * 64 + c] + red[(2 * MT + m) * 64 + c] + bv;
            if (m >= M) continue;
            float* dst = C + (long)m * ldc + n;
            if (mask) {
                const float y = mask[(long)m * ldc + n];          // act'(.) from the stored activation output (sign(y) = sign(x))
                const float d = act == CN_ACT_LRELU ? (y > 0.f ? 1.f : slope) : act == CN_ACT_RELU ? (y > 0.f ? 1.f : 0.f)
                                : act == CN_ACT_TANH ? 1.f - y * y : 1.f;
                *dst = v * d;
            } else if (J.accumulate[j]) {
                unsafeAtomicAdd(dst, v);
            } else {
                *dst = cn_apply_act(v, act, slope);
            }
        }
    }
}

// ---- the same launch for any K: the A block is staged in chunks of KC = 8192 / MT columns (the LDS block of the kernel above at
// its limit), wave q walks quarter q of every chunk and keeps its sums in registers from chunk to chunk, so the K quarters are
// still combined once, in the same order, after the last chunk.  A job with K <= KC takes one chunk: the multiply-adds of
// gemm_rows_grouped_kernel in its order (measured: the same bits in rows 0..29; in rows 30 and 31 of MT = 32 hipcc fuses the
// multiply-add of one kernel and not of the other, one rounding apart -- tests/test_gemm_rows_ksteps_gpu.py).  Launches that fit
// the whole block never come here (plan_rows_group).  The chunk count comes from the job alone (j is wave- and workgroup-uniform), so every barrier of the
// loop is reached by all 256 threads; the n < N guard sits inside, around the loads of B only.
template <int MT>
__global__ __launch_bounds__(256) void gemm_rows_grouped_ksteps_kernel(RowsJobs J) {
    constexpr int KC = 8192 / MT;
    extern __shared__ float sm[];                 // A chunk [MT][len <= KC] (rows >= M are zero); at MT * KC the partial sums [3][MT][64]
    const int bid = blockIdx.x;
    int lo = 0, hi = J.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.blk0[mid] <= bid) lo = mid;
        else hi = mid;
    }
    const int j = __builtin_amdgcn_readfirstlane(lo);
    const int M = J.m[j], N = J.n[j], K = J.k[j], lda = J.lda[j], ldb = J.ldb[j], ldc = J.ldc[j], tb = J.tb[j];
    const float* __restrict__ A = J.a[j];
    const float* __restrict__ B = J.b[j];
    float* __restrict__ C = J.c[j];
    float* As = sm;
    float* red = sm + MT * KC;
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    const int n = (bid - J.blk0[j]) * 64 + c;
    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.f;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int len = min(KC, K - k0);
        if (k0 > 0) __syncthreads();              // every wave has finished with the previous chunk
        for (int i = tid; i < MT * len; i += 256) {
            const int m = i / len, k = i - m * len;
            As[i] = m < M ? A[(long)m * lda + k0 + k] : 0.f;
        }
        __syncthreads();
        const int kq = (len + 3) / 4, kbeg = q * kq, kend = min(len, kbeg + kq);
        if (n < N) {
            if (tb) {
                const float* __restrict__ Bn = B + (long)n * ldb + k0;
#pragma unroll 4
                for (int k = kbeg; k < kend; ++k) {
                    const float b = Bn[k];
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m] += As[m * len + k] * b;
                }
            } else {
                const float* __restrict__ Bn = B + (long)k0 * ldb + n;
#pragma unroll 4
                for (int k = kbeg; k < kend; ++k) {
                    const float b = Bn[(long)k * ldb];
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[m] += As[m * len + k] * b;
                }
            }
        }
    }
    if (q > 0) {
#pragma unroll
        for (int m = 0; m < MT; ++m) red[((q - 1) * MT + m) * 64 + c] = acc[m];
    }
    __syncthreads();
    if (q == 0 && n < N) {
        const float bv = J.bias[j] ? J.bias[j][n] : 0.f;
        const float* __restrict__ mask = J.mask[j];
        const int act = J.act[j];
        const float slope = J.slope[j];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float v = acc[m] + red[(0 * MT + m) * 64 + c] + red[(1 * MT + m) * 64 + c] + red[(2 * MT + m) * 64 + c] + bv;
            if (m >= M) continue;
            float* dst = C + (long)m * ldc + n;
            if (mask) {
                const float y = mask[(long)m * ldc + n];          // act'(.) from the stored activation output (sign(y) = sign(x))
                const float d = act == CN_ACT_LRELU ? (y > 0.f ? 1.f : slope) : act == CN_ACT_RELU ? (y > 0.f ? 1.f : 0.f)
                                : act == CN_ACT_TANH ? 1.f - y * y : 1.f;
                *dst = v * d;
            } else if (J.accumulate[j]) {
                unsafeAtomicAdd(dst, v);
            } else {
                *dst = cn_apply_act(v, act, slope);
            }
        }
    }
}

__global__ void zero_rows_kernel(float* C, int M, int N, int ldc) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)M * N) C[(i / N) * ldc + i % N] = 0.f;
}

}  // namespace

// ---- the launch of a dense product: decided here, performed by gemm_launch ----
enum { GEMM_ROWS = 0, GEMM_DEPTH, GEMM_THIN, GEMM_TILE };
struct GemmPlan {
    int route;                // GEMM_ROWS / GEMM_DEPTH / GEMM_THIN / GEMM_TILE
    int mt;                   // rows: the row count the kernel is instantiated for (8 / 16 / 32); else 0
    int gx, gy, gz;           // grid
    int kps;                  // K per slice (thin: grid y slices, tile: grid z slices; rows / depth: k)
    int zero_first;           // the slices add with atomics: clear C before the launch
    long parts_floats;        // deterministic mode: the per-slice slabs [gz][m][n] of the stream's workspace, added in order afterwards
    size_t lds;               // dynamic LDS bytes (rows: the A block [mt][k], then the partial sums [3][mt][64])
};

// the rows kernels' instantiation for m rows and their LDS block; mt * k <= 8192 floats is what they take
static inline int gemm_rows_mt(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : 32; }
static inline size_t gemm_rows_lds(int mt, int k) { return sizeof(float) * ((size_t)mt * k + 3 * mt * 64); }

// Pure.  The order of the tests matters: rows before depth before thin, the 64x64 tile takes what is left.
static GemmPlan plan_gemm(int ta, int tb, int m, int n, int k, int ldc, bool has_bias, int act, bool accumulate, bool det) {
    GemmPlan p{};
    p.gx = p.gy = p.gz = 1;
    p.kps = k;
    if (!accumulate && !ta && m <= 32 && n > 4 && (long)gemm_rows_mt(m) * k <= 8192) {
        p.route = GEMM_ROWS;
        p.mt = gemm_rows_mt(m);
        p.lds = gemm_rows_lds(p.mt, k);
        p.gx = cn_cdiv(n, 64);
        return p;
    }
    if (ta && !tb && k <= 32 && !has_bias && act == CN_ACT_NONE) {
        p.route = GEMM_DEPTH;
        p.gx = cn_cdiv(m, 16);
        p.gy = cn_cdiv(n, 64);
        return p;
    }
    if (!accumulate && !ta && !tb && n <= 4 && m <= 256 && k >= 128) {
        int slices = 1;
        if (act == CN_ACT_NONE && k >= 8192 && !det) slices = k / 4096;      // (deterministic mode: no K slices, no atomics)
        const int kps = (k + slices - 1) / slices;
        slices = (k + kps - 1) / kps;
        p.route = GEMM_THIN;
        p.gx = m;
        p.gy = slices;
        p.kps = kps;
        p.zero_first = slices > 1;
        return p;
    }
    const long tiles = (long)cn_cdiv(m, 64) * cn_cdiv(n, 64);
    int splitk = 1;
    if (act == CN_ACT_NONE && tiles < 128 && k >= 1024 && !(det && (accumulate || ldc != n))) {
        splitk = (int)((256 + tiles - 1) / tiles);
        if (splitk > k / 256) splitk = k / 256;
        if (splitk < 1) splitk = 1;
    }
    int kps = (k + splitk - 1) / splitk;
    kps = (kps + BK - 1) / BK * BK;
    splitk = (k + kps - 1) / kps;
    if (det && splitk > 1) {
        // deterministic mode: K slices into per-split slabs of the stream's workspace, added in split order by a second launch.
        // The cap never binds: splitting needs tiles < 128, so m * n <= 4096 * tiles and cap >= 4096 / tiles, while the split asked
        // for is at most ceil(256 / tiles) (tests/test_gemm_plan_cpu.py sweeps it); it stays as the guard of the workspace size.
        const long cap = (long)(CN_DET_WS_FLOATS / ((size_t)m * n));
        if (splitk > cap) splitk = (int)(cap < 1 ? 1 : cap);
        kps = (k + splitk - 1) / splitk;
        kps = (kps + BK - 1) / BK * BK;
        splitk = (k + kps - 1) / kps;
        if (splitk > 1) p.parts_floats = (long)splitk * m * n;
    }
    p.route = GEMM_TILE;
    p.gx = cn_cdiv(m, 64);
    p.gy = cn_cdiv(n, 64);
    p.gz = splitk;
    p.kps = kps;
    p.zero_first = splitk > 1 && !accumulate && !p.parts_floats;
    return p;
}

/* out = {route (0 rows, 1 depth, 2 thin, 3 tile), MT of the rows kernel (else 0), grid x, y, z, K per slice, C cleared first (0 / 1),
 * floats of the deterministic workspace, dynamic LDS bytes} */
extern "C" int cn_gemm_plan(int ta, int tb, int m, int n, int k, int ldc, int has_bias, int act, int accumulate, int deterministic,
                            int out[9]) {
    CN_CHECK_ARG(m > 0 && n > 0 && k > 0 && ldc >= n && out, "gemm_plan: bad args m=%d n=%d k=%d ldc=%d", m, n, k, ldc);
    const GemmPlan p = plan_gemm(ta, tb, m, n, k, ldc, has_bias != 0, act, accumulate != 0, deterministic != 0);
    const int v[9] = {p.route, p.mt, p.gx, p.gy, p.gz, p.kps, p.zero_first, (int)p.parts_floats, (int)p.lds};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return CN_OK;
}

// Performs the plan: deterministic workspace, zero pass, the launch, the ordered sum of the slabs.
static int gemm_launch(int ta, int tb, int m, int n, int k, const float* a, int lda, const float* b, int ldb, float* c,
                       int ldc, const float* bias, int act, float slope, int accumulate, void* stream) {
    CN_CHECK_ARG(m > 0 && n > 0 && k > 0 && a && b && c, "gemm: bad args m=%d n=%d k=%d", m, n, k);
    CN_CHECK_ARG(lda >= (ta ? m : k) && ldb >= (tb ? k : n) && ldc >= n, "gemm: leading dimension too small");
    hipStream_t s = (hipStream_t)stream;
    const GemmPlan p = plan_gemm(ta, tb, m, n, k, ldc, bias != nullptr, act, accumulate != 0, cn_det() != 0);
    float* parts = nullptr;
    if (p.parts_floats) {
        parts = cn_det_ws(s, (size_t)p.parts_floats);
        if (!parts) return CN_EINVAL;
    }
    if (p.zero_first) {
        hipLaunchKernelGGL(zero_rows_kernel, dim3(cn_cdiv((long)m * n, 256)), dim3(256), 0, s, c, m, n, ldc);
        CN_LAUNCH_CHECK();
    }
    const dim3 grid(p.gx, p.gy, p.gz);
    switch (p.route) {
        case GEMM_ROWS:
#define ROWS(MT_, TB_) hipLaunchKernelGGL((gemm_rows_kernel<MT_, TB_>), grid, dim3(256), p.lds, s, m, n, k, a, lda, b, ldb, c, ldc, bias, act, slope)
            if (p.mt == 8) { if (tb) ROWS(8, true); else ROWS(8, false); }
            else if (p.mt == 16) { if (tb) ROWS(16, true); else ROWS(16, false); }
            else { if (tb) ROWS(32, true); else ROWS(32, false); }
#undef ROWS
            break;
        case GEMM_DEPTH:
            hipLaunchKernelGGL(gemm_depth_kernel, grid, dim3(256), 0, s, m, n, k, a, lda, b, ldb, c, ldc, accumulate);
            break;
        case GEMM_THIN:
            hipLaunchKernelGGL(thin_gemm_kernel, grid, dim3(256), 0, s, m, n, k, a, lda, b, ldb, c, ldc, bias, act, slope, p.kps);
            break;
        default:
            // (the kernel adds with atomics whenever its last but one argument is > 1: split-K, or accumulation into the caller's C)
            hipLaunchKernelGGL(gemm_kernel, grid, dim3(256), 0, s, ta, tb, m, n, k, a, lda, b, ldb, c, ldc, bias, act, slope, p.kps,
                               accumulate ? 2 : p.gz, parts);
    }
    CN_LAUNCH_CHECK();
    if (parts) return cn_sum_parts(parts, c, p.gz, (long)m * n, 0, 1.f, s);
    return CN_OK;
}

extern "C" int cn_gemm(int ta, int tb, int m, int n, int k, const float* a, int lda, const float* b, int ldb, float* c,
                       int ldc, const float* bias, int act, float slope, void* stream) {
    return gemm_launch(ta, tb, m, n, k, a, lda, b, ldb, c, ldc, bias, act, slope, 0, stream);
}

// C += op(A) op(B): the weight gradient of a Dense layer added straight into its slot of the network's gradient arena
extern "C" int cn_gemm_acc(int ta, int tb, int m, int n, int k, const float* a, int lda, const float* b, int ldb, float* c,
                           int ldc, void* stream) {
    return gemm_launch(ta, tb, m, n, k, a, lda, b, ldb, c, ldc, nullptr, CN_ACT_NONE, 0.f, 1, stream);
}

// C_j = epi(A_j op(B_j) + bias_j), m_j <= 32 rows, for every job in one launch per 16 jobs; `jobs` is a HOST array.
extern "C" int cn_gemm_rows_grouped(const CnRowsJob* jobs, int njobs, void* stream) {
    CN_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs), "cn_gemm_rows_grouped: bad arguments");
    for (int first = 0; first < njobs; first += CN_ROWS_GROUP) {
        RowsJobs J{};
        const int cnt = njobs - first < CN_ROWS_GROUP ? njobs - first : CN_ROWS_GROUP;
        long blocks = 0;
        int mmax = 0, kmax = 0;
        for (int q = 0; q < cnt; ++q) {
            const CnRowsJob& d = jobs[first + q];
            CN_CHECK_ARG(d.a && d.b && d.c && d.m > 0 && d.m <= 32 && d.n > 0 && d.k > 0 && d.lda >= d.k && d.ldb >= (d.tb ? d.k : d.n) && d.ldc >= d.n,
                         "cn_gemm_rows_grouped: job %d: m=%d n=%d k=%d (m <= 32)", first + q, d.m, d.n, d.k);
            CN_CHECK_ARG(!(d.mask && d.accumulate) && !(d.accumulate && (d.bias || d.act != CN_ACT_NONE)),
                         "cn_gemm_rows_grouped: job %d: accumulate excludes mask / bias / activation", first + q);
            J.a[q] = d.a; J.b[q] = d.b; J.c[q] = d.c; J.bias[q] = d.bias; J.mask[q] = d.mask;
            J.m[q] = d.m; J.n[q] = d.n; J.k[q] = d.k; J.lda[q] = d.lda; J.ldb[q] = d.ldb; J.ldc[q] = d.ldc;
            J.tb[q] = d.tb; J.act[q] = d.act; J.accumulate[q] = d.accumulate; J.slope[q] = d.slope;
            J.blk0[q] = (int)blocks;
            blocks += cn_cdiv(d.n, 64);
            mmax = d.m > mmax ? d.m : mmax;
            kmax = d.k > kmax ? d.k : kmax;
        }
        J.blk0[cnt] = (int)blocks;
        J.count = cnt;
        const int mt = gemm_rows_mt(mmax);
        CN_CHECK_ARG((long)mt * kmax <= 8192, "cn_gemm_rows_grouped: %d rows x k = %d do not fit the LDS block", mt, kmax);
        const size_t lds = gemm_rows_lds(mt, kmax);
        if (mt == 8) hipLaunchKernelGGL((gemm_rows_grouped_kernel<8>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, J);
        else if (mt == 16) hipLaunchKernelGGL((gemm_rows_grouped_kernel<16>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, J);
        else hipLaunchKernelGGL((gemm_rows_grouped_kernel<32>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, J);
        CN_LAUNCH_CHECK();
    }
    return CN_OK;
}

// ---- the grouped rows product for any k: decided by plan_rows_group, performed by cn_gemm_rows_grouped_k ----
struct RowsGroupPlan {
    int first, count;         // the run of jobs of this launch (at most CN_ROWS_GROUP)
    int mt;                   // instantiation, from the largest m of the run
    int kc;                   // columns of A per chunk: 8192 / mt
    int chunks;               // chunks the largest k of the run takes
    int grid;                 // workgroups: sum of cdiv(n, 64)
    size_t lds;               // dynamic LDS bytes
    int ksteps;               // 0: the whole A block fits (mt * kmax <= 8192): gemm_rows_grouped_kernel, the launch of cn_gemm_rows_grouped;
                              // 1: gemm_rows_grouped_ksteps_kernel
};

// Pure: the launch of the run of jobs that starts at `first`; looks at m, n and k only.
static RowsGroupPlan plan_rows_group(const CnRowsJob* jobs, int njobs, int first) {
    RowsGroupPlan p{};
    p.first = first;
    p.count = njobs - first < CN_ROWS_GROUP ? njobs - first : CN_ROWS_GROUP;
    int mmax = 0, kmax = 0;
    for (int q = 0; q < p.count; ++q) {
        const CnRowsJob& d = jobs[first + q];
        p.grid += cn_cdiv(d.n, 64);
        mmax = d.m > mmax ? d.m : mmax;
        kmax = d.k > kmax ? d.k : kmax;
    }
    p.mt = gemm_rows_mt(mmax);
    p.kc = 8192 / p.mt;
    p.chunks = cn_cdiv(kmax, p.kc);
    p.ksteps = (long)p.mt * kmax <= 8192 ? 0 : 1;
    p.lds = p.ksteps ? gemm_rows_lds(p.mt, p.kc) : gemm_rows_lds(p.mt, kmax);
    return p;
}

// the argument checks of cn_gemm_rows_grouped, job by job (the plan query does not look at the pointers)
static int rows_jobs_check(const char* who, const CnRowsJob* jobs, int njobs, bool pointers) {
    CN_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs), "%s: bad arguments", who);
    for (int q = 0; q < njobs; ++q) {
        const CnRowsJob& d = jobs[q];
        CN_CHECK_ARG((!pointers || (d.a && d.b && d.c)) && d.m > 0 && d.m <= 32 && d.n > 0 && d.k > 0 && d.lda >= d.k && d.ldb >= (d.tb ? d.k : d.n) && d.ldc >= d.n,
                     "%s: job %d: m=%d n=%d k=%d (m <= 32)", who, q, d.m, d.n, d.k);
        CN_CHECK_ARG(!(d.mask && d.accumulate) && !(d.accumulate && (d.bias || d.act != CN_ACT_NONE)),
                     "%s: job %d: accumulate excludes mask / bias / activation", who, q);
    }
    return CN_OK;
}

/* out = per launch {first job, jobs, MT, KC, chunks of the largest k, grid, dynamic LDS bytes, ksteps (0: gemm_rows_grouped_kernel,
 * 1: gemm_rows_grouped_ksteps_kernel)} */
extern "C" int cn_gemm_rows_grouped_plan(const CnRowsJob* jobs, int njobs, int* out, int cap, int* nlaunches) {
    const int rc = rows_jobs_check("cn_gemm_rows_grouped_plan", jobs, njobs, false);
    if (rc != CN_OK) return rc;
    const int launches = cn_cdiv(njobs, CN_ROWS_GROUP);
    CN_CHECK_ARG(out && nlaunches && cap >= 8 * launches, "cn_gemm_rows_grouped_plan: %d launches need %d ints (cap = %d)", launches, 8 * launches, cap);
    for (int l = 0; l < launches; ++l) {
        const RowsGroupPlan p = plan_rows_group(jobs, njobs, l * CN_ROWS_GROUP);
        const int v[8] = {p.first, p.count, p.mt, p.kc, p.chunks, p.grid, (int)p.lds, p.ksteps};
        for (int i = 0; i < 8; ++i) out[8 * l + i] = v[i];
    }
    *nlaunches = launches;
    return CN_OK;
}

// cn_gemm_rows_grouped without its LDS refusal: every job is checked before the first launch, then one launch per plan.
extern "C" int cn_gemm_rows_grouped_k(const CnRowsJob* jobs, int njobs, void* stream) {
    const int rc = rows_jobs_check("cn_gemm_rows_grouped_k", jobs, njobs, true);
    if (rc != CN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    for (int first = 0; first < njobs; first += CN_ROWS_GROUP) {
        const RowsGroupPlan p = plan_rows_group(jobs, njobs, first);
        RowsJobs J{};
        int blocks = 0;
        for (int q = 0; q < p.count; ++q) {
            const CnRowsJob& d = jobs[first + q];
            J.a[q] = d.a; J.b[q] = d.b; J.c[q] = d.c; J.bias[q] = d.bias; J.mask[q] = d.mask;
            J.m[q] = d.m; J.n[q] = d.n; J.k[q] = d.k; J.lda[q] = d.lda; J.ldb[q] = d.ldb; J.ldc[q] = d.ldc;
            J.tb[q] = d.tb; J.act[q] = d.act; J.accumulate[q] = d.accumulate; J.slope[q] = d.slope;
            J.blk0[q] = blocks;
            blocks += cn_cdiv(d.n, 64);
        }
        J.blk0[p.count] = blocks;
        J.count = p.count;
        const dim3 grid((unsigned)p.grid);
#define ROWS_GROUP(MT_) do { \
            if (p.ksteps) hipLaunchKernelGGL((gemm_rows_grouped_ksteps_kernel<MT_>), grid, dim3(256), p.lds, s, J); \
            else hipLaunchKernelGGL((gemm_rows_grouped_kernel<MT_>), grid, dim3(256), p.lds, s, J); } while (0)
        if (p.mt == 8) ROWS_GROUP(8);
        else if (p.mt == 16) ROWS_GROUP(16);
        else ROWS_GROUP(32);
#undef ROWS_GROUP
        CN_LAUNCH_CHECK();
    }
    return CN_OK;
}

// C_j += A_j^T B_j (A_j: k x m, B_j: k x n, row-major, k <= 32) for every job in one launch per 64 jobs; `jobs` is a HOST array.
extern "C" int cn_gemm_depth_grouped(const CnDepthJob* jobs, int njobs, void* stream) {
    CN_CHECK_ARG(njobs >= 0 && (njobs == 0 || jobs), "cn_gemm_depth_grouped: bad arguments");
    for (int first = 0; first < njobs; first += CN_DEPTH_GROUP) {
        DepthJobs J{};
        const int cnt = njobs - first < CN_DEPTH_GROUP ? njobs - first : CN_DEPTH_GROUP;
        long blocks = 0;
        for (int q = 0; q < cnt; ++q) {
            const CnDepthJob& d = jobs[first + q];
            CN_CHECK_ARG(d.a && d.b && d.c && d.m > 0 && d.n > 0 && d.k > 0 && d.k <= 32 && d.lda >= d.m && d.ldb >= d.n && d.ldc >= d.n,
                         "cn_gemm_depth_grouped: job %d: m=%d n=%d k=%d (k <= 32)", first + q, d.m, d.n, d.k);
            J.a[q] = d.a; J.b[q] = d.b; J.c[q] = d.c;
            J.m[q] = d.m; J.n[q] = d.n; J.k[q] = d.k; J.lda[q] = d.lda; J.ldb[q] = d.ldb; J.ldc[q] = d.ldc;
            J.blk0[q] = (int)blocks;
            blocks += (long)cn_cdiv(d.m, 16) * cn_cdiv(d.n, 64);
        }
        J.blk0[cnt] = (int)blocks;
        J.count = cnt;
        hipLaunchKernelGGL(gemm_depth_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, J);
        CN_LAUNCH_CHECK();
    }
    return CN_OK;
}
