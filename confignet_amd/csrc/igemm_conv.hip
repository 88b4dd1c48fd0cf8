// igemm_conv.hip -- N-d convolution family as implicit GEMM on the CDNA4 matrix cores.
//
// fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (exact f32, 157 TF peak on MI355X).
// One 256-thread workgroup (4 wave64, 2x2) owns a (64*TM) x (64*TN) output tile; each wave
// owns TM x TN 32x32 MFMA tiles.  K is walked in steps of 16: the gathered activation tile
// and the filter tile are prefetched from HBM/L2 into registers while the previous step is
// multiplied out of LDS (two LDS buffers, one barrier per step).  Both LDS tiles are
// "k-major" ([k][m] / [k][n], row pitch +4 floats) so every MFMA operand read is a
// conflict-free ds_read_b32 of 32 consecutive floats per half-wave.
//
// Layouts: activations channels-last (N,[D,]H,W,C); filters Keras (kd,kh,kw,cin,cout) ==
// row-major [K = taps*cin][cout], i.e. already the B matrix of the GEMM.  The x2 nearest
// upsample that precedes most generator convolutions (hologan_generator.py:139-170) is folded
// into the gather (index >> 1); SAME padding ([TF-2.1] asymmetric, low = total//2) and the
// zero-stuffing of strided data-gradients are predicates of the gather.
//
// This file: the register-staged forward / data-gradient kernel, the row-split filter-gradient kernel (plus the two from-RGB
// reductions), their launchers and the host entry points of common.h.  Which layer gets which of them -- or the LDS-DMA loops of
// fwd2.hip / wgrad2.hip, or a kernel of small_conv.hip -- is decided in conv_dispatch.hip.
#include "common.h"

#include "mma_tile.h"
#include "typed.h"
#include "conv_geom.h"

namespace {

// ---------------------------------------------------------------------------------------------
// forward / data-gradient:  Y[m, co] = act( sum_{t,ci} X[src(m,t), ci] * W[t, ci, co] + bias[co] )
// ---------------------------------------------------------------------------------------------
template <int WM, int WN, int TM, int TN, bool VEC, bool BVEC = true>
__global__ __launch_bounds__(256) void igemm_fwd_kernel(CnConvGeom g, const float* __restrict__ X,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        float* __restrict__ Y, int act, float slope, int par,
                                                        int xcd_swizzle, int ntiles_m, int ntiles_n, int bt = 0,
                                                        long part_stride = 0, const float* __restrict__ res = nullptr) {
    // res (unsplit launches only): a tensor of Y's shape added before the activation (residual branch of a ResNet block)
    // bt: W is the ORIGINAL filter [t][n = output channel here][k = reduction channel here] of the convolution whose data
    // gradient this launch computes (tap order reversed, the two channel axes swapped): the B tile is then loaded like the
    // gathered A tile (16-byte pieces along k, transposed on the way into LDS) -- no tap-flipped, channel-transposed copy of
    // every trainable filter per step (cn_conv_weight_tflip: 80 launches per iteration)
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN, LDA = BM + 4, LDB = BN + 4;
    constexpr int KQ = BK / 4;                          // float4 pieces per A row per K step
    constexpr int RPP = 256 / KQ;                       // A rows loaded per pass of the workgroup
    constexpr int AP = BM / RPP, BP = (BK * BN / 4 + 255) / 256;   // float4 loads per thread per K step
    __shared__ float As[2][BK][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];
    __shared__ int rowmap[BM];                          // tile row -> output row (or -1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, half = lane >> 5, l31 = lane & 31;
    const int M = g.n * g.out_d * g.out_h * g.out_w;
    const int T = g.k_d * g.k_h * g.k_w;
    const int Ktot = T * g.cin;
    // XCD-aware tile order: workgroup b runs on XCD b % 8 (observed dispatch order); give each XCD a contiguous
    // run of M tiles so that neighbouring tiles (shared input halo rows) hit the same 4 MiB L2.  Bijective for
    // any grid size; placement only affects speed, never results.
    int bx = blockIdx.x, by = blockIdx.y;
    if ((xcd_swizzle & 3) == 2) {
        // 1-D launch over all (M tile, cout tile) pairs: XCD = id % 8 gets a contiguous run of M tiles and, within it, the
        // cout tiles of one M tile in consecutive slots -- they read the same input rows, which then come from that XCD's
        // L2 instead of being fetched once per cout tile
        const int nt = ntiles_n, nmt = ntiles_m;
        const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
        const int q = nmt >> 3, r = nmt & 7;                              // M tiles per XCD: q (+1 for the first r XCDs)
        const int mine = q + (xcd < r ? 1 : 0);
        int ml;
        divmod_pos(j, nt, ml, by);
        if (ml >= mine) return;                                           // padding slot of the rounded-up launch
        bx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + ml;
    } else if (xcd_swizzle && !par) {   // parity-ordered rows: classes have 1/2/2/4 live taps, keep them interleaved over XCDs
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bx & 7, idx = bx >> 3;
        bx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int m0 = bx * BM, n0 = by * BN;

    const int kq = tid % KQ, arow = tid / KQ;
    RowInfo ri[AP];
    unsigned long long tapmask = T >= 64 ? ~0ull : ((1ull << T) - 1ull);
#pragma unroll
    for (int i = 0; i < AP; ++i) {
        int mrow = m0 + arow + RPP * i;
        if (par) {
            int cls;
            mrow = par_row(g, mrow, M, cls);
        }
        ri[i] = decode_row(g, mrow, M);
        if (kq == 0) rowmap[arow + RPP * i] = ri[i].ok ? mrow : -1;
    }
    if (par) {
        int c0, c1;
        par_row(g, m0, M, c0);
        par_row(g, min(m0 + BM, M) - 1, M, c1);
        if (c0 == c1) tapmask = par_tap_mask(g, c0);   // whole tile in one parity class: skip dead taps
    }
    int aoff[AP];

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // two register sets: loads of K step s+2 are issued while step s is multiplied and step s+1 is still in flight, so a
    // gathered operand has two steps of MFMA time to arrive (small tiles give a workgroup only 512 MFMA cycles per step and
    // small problems only 1-2 workgroups per CU: one step did not cover the L2/HBM latency -- MFMA-busy 0.41 on the 64x64 tile)
    float4 ra0[AP], rb0[BP], ra1[AP], rb1[BP];
    const int cpb = VEC ? g.cin / BK : 1;
    const int nks_all = VEC ? __popcll(tapmask) * cpb : (Ktot + BK - 1) / BK;
    // split-K over gridDim.z (small-M problems): this workgroup walks K steps [ks_beg, ks_end)
    const int per_z = (nks_all + gridDim.z - 1) / gridDim.z;
    const int ks_beg = blockIdx.z * per_z, ks_end = min(nks_all, ks_beg + per_z);
    int cur_ord = -1, cur_tap = -1;                     // ordinal among live taps / tap index
    const bool tap_minor = VEC && xcd_swizzle >= 2 && !par && gridDim.z == 1 && T > 1 && T <= 9 && (xcd_swizzle & 4);
    extern __shared__ int offtab[];                     // tap-minor order: gather offset of every (tap, row of this thread)
    if (tap_minor) {
        for (int t = 0; t < T; ++t) {
            int kd, kh, kw;
            tap_decode(g, t, kd, kh, kw);
#pragma unroll
            for (int i = 0; i < AP; ++i) offtab[(t * AP + i) * 256 + tid] = src_off(g, ri[i], kd, kh, kw);
        }
    }

    // K order.  Tap-major (all channel chunks of a tap, then the next tap) recomputes the gather offsets once per tap.
    // Tap-minor (tap_minor != 0: all taps of a channel chunk, then the next chunk) recomputes them every step but keeps
    // the XCD's working set at (tiles in flight) x (rows) x BK channels, so the taps' shifted re-reads of a chunk hit
    // the 4 MiB L2 instead of going back to the fabric (stride-1 layers with many channels).
    auto load_tiles = [&](int ks, float4 (&ra)[AP], float4 (&rb)[BP], unsigned& amask) {
        if (VEC) {
            int c0;
            if (tap_minor) {
                const int chunk = ks / T;
                cur_tap = ks - chunk * T;
                c0 = chunk * BK;
#pragma unroll
                for (int i = 0; i < AP; ++i) aoff[i] = offtab[(cur_tap * AP + i) * 256 + tid];
            } else {
                const int ord = ks / cpb;
                c0 = (ks - ord * cpb) * BK;
                if (ord != cur_ord) {
                    while (cur_ord < ord) {
                        cur_tap += __ffsll((long long)(tapmask >> (cur_tap + 1)));
                        ++cur_ord;
                    }
                    int kd, kh, kw;
                    tap_decode(g, cur_tap, kd, kh, kw);
#pragma unroll
                    for (int i = 0; i < AP; ++i) aoff[i] = src_off(g, ri[i], kd, kh, kw);
                }
            }
            const int tap = cur_tap;
            // every load below is UNCONDITIONAL (dead rows / columns read a clamped, valid address and are zeroed on the way
            // into LDS): a load inside a branch makes the compiler's waitcnt insertion assume the branch was skipped, and it
            // then drains vmcnt to 0 before every LDS store -- the two-step lookahead of the register sets would be lost
            amask = 0;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                ra[i] = *reinterpret_cast<const float4*>(X + max(aoff[i], 0) + c0 + kq * 4);
                amask |= (aoff[i] >= 0 ? 1u : 0u) << i;
            }
            if (bt) {
#pragma unroll
                for (int j = 0; j < BP; ++j) {
                    const int idx = min(tid + 256 * j, BK * BN / 4 - 1);
                    const int nn = min(n0 + idx / KQ, g.cout - 1), kk = (idx % KQ) * 4;
                    rb[j] = *reinterpret_cast<const float4*>(W + ((long)(T - 1 - tap) * g.cout + nn) * g.cin + c0 + kk);
                }
            } else {
#pragma unroll
                for (int j = 0; j < BP; ++j) {
                    const int idx = BVEC ? min(tid + 256 * j, BK * BN / 4 - 1) : tid + 256 * j;
                    const int brow = idx / (BN / 4), col = n0 + (idx % (BN / 4)) * 4;
                    const long kg = (long)tap * g.cin + c0 + brow;
                    if (BVEC) {
                        rb[j] = *reinterpret_cast<const float4*>(W + kg * g.cout + min(col, g.cout - 4));
                    } else {   // thin cout (3-channel image gradients): guarded scalar filter loads
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (col + e < g.cout && idx < BK * BN / 4) ? W[kg * g.cout + col + e] : 0.f;
                        rb[j] = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
        } else {
            amask = ~0u;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = ks * BK + kq * 4 + e;
                    v[e] = 0.f;
                    if (k < Ktot) {
                        const int tap = k / g.cin, ci = k - tap * g.cin;
                        int kd, kh, kw;
                        tap_decode(g, tap, kd, kh, kw);
                        const int off = src_off(g, ri[i], kd, kh, kw);
                        if (off >= 0) v[e] = X[off + ci];
                    }
                }
                ra[i] = make_float4(v[0], v[1], v[2], v[3]);
            }
#pragma unroll
            for (int j = 0; j < BP; ++j) {
                const int idx = tid + 256 * j;
                const int brow = idx / (BN / 4), col = n0 + (idx % (BN / 4)) * 4;
                const long kg = (long)ks * BK + brow;
                rb[j] = (col < g.cout && kg < Ktot && idx < BK * BN / 4)
                            ? *reinterpret_cast<const float4*>(W + kg * g.cout + col)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto store_tiles = [&](int buf, const float4 (&ra)[AP], const float4 (&rb)[BP], unsigned amask) {
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const int r = arow + RPP * i;
            const bool live = (amask >> i) & 1u;     // padding taps / rows past the end: zeros (the load read a clamped address)
            As[buf][kq * 4 + 0][r] = live ? ra[i].x : 0.f;
            As[buf][kq * 4 + 1][r] = live ? ra[i].y : 0.f;
            As[buf][kq * 4 + 2][r] = live ? ra[i].z : 0.f;
            As[buf][kq * 4 + 3][r] = live ? ra[i].w : 0.f;
        }
        if (VEC && bt) {
#pragma unroll
            for (int j = 0; j < BP; ++j) {
                const int idx = tid + 256 * j;
                const int nn = idx / KQ, kk = (idx % KQ) * 4;
                if (idx < BK * BN / 4) {
                    Bs[buf][kk + 0][nn] = rb[j].x;
                    Bs[buf][kk + 1][nn] = rb[j].y;
                    Bs[buf][kk + 2][nn] = rb[j].z;
                    Bs[buf][kk + 3][nn] = rb[j].w;
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) {
            const int idx = tid + 256 * j;
            const int brow = idx / (BN / 4), bcol = (idx % (BN / 4)) * 4;
            if (idx < BK * BN / 4) *reinterpret_cast<float4*>(&Bs[buf][brow][bcol]) = rb[j];
        }
    };

    const int a_col = wm * 32 * TM + l31, b_col = wn * 32 * TN + l31;
    // The steps past the end re-load the last step (clamped index) and store it into the LDS buffer nobody reads again:
    // no branch around a load or a store in the loop (see load_tiles).  Dead filter columns (>= cout) carry whatever the
    // clamped address held: they only reach accumulator columns the epilogue never stores.
    unsigned am0 = 0, am1 = 0;
    if (ks_beg < ks_end) {
        const int ks_last = ks_end - 1;
        load_tiles(ks_beg, ra0, rb0, am0);
        store_tiles(0, ra0, rb0, am0);
        load_tiles(min(ks_beg + 1, ks_last), ra1, rb1, am1);
        __syncthreads();
        int ks = ks_beg;
        for (; ks + 1 < ks_end; ks += 2) {
            // even step: LDS buffer 0 holds step ks, set 1 holds step ks+1 (in flight), step ks+2 goes to set 0
            load_tiles(min(ks + 2, ks_last), ra0, rb0, am0);
            mma_step<TM, TN, LDA, LDB>(As[0], Bs[0], acc, a_col, b_col, half);
            store_tiles(1, ra1, rb1, am1);
            __syncthreads();
            // odd step: buffer 1 holds step ks+1, set 0 holds step ks+2, step ks+3 goes to set 1
            load_tiles(min(ks + 3, ks_last), ra1, rb1, am1);
            mma_step<TM, TN, LDA, LDB>(As[1], Bs[1], acc, a_col, b_col, half);
            store_tiles(0, ra0, rb0, am0);
            __syncthreads();
        }
        if (ks < ks_end) mma_step<TM, TN, LDA, LDB>(As[0], Bs[0], acc, a_col, b_col, half);   // odd number of steps: the last one
    } else {
        // no K step at all (an empty K split; a parity-ordered tile whose class has no live tap: three of the four classes of a 1x1
        // stride-2 data gradient): the epilogue below reads rowmap entries that OTHER waves wrote, and without the loop's barriers
        // nothing ordered those writes before the reads -- a wave that ran ahead stored its (zero) rows through whatever the LDS
        // held before (found with the real halves of the discriminator steps shifted under the generator tail: ResNet-50's
        // 64x64x256 <- 32x32x128 data gradient wrote through stale floats and faulted)
        __syncthreads();
    }

    // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * 32 * TN + 32 * j + l31;
        if (col >= g.cout) continue;
        const float bv = (bias && blockIdx.z == 0) ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rbase = wm * 32 * TM + 32 * i + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rowmap[rbase + (r & 3) + 8 * (r >> 2)];
                if (row < 0) continue;
                const float v = acc[i][j][r] + bv;
                // (deterministic mode: every K split stores its partial tile in its own slab; the slabs are added in order afterwards)
                if (part_stride) Y[(long)blockIdx.z * part_stride + (long)row * g.cout + col] = v;
                else if (split) unsafeAtomicAdd(&Y[(long)row * g.cout + col], v);
                else Y[(long)row * g.cout + col] = cn_apply_act(res ? v + res[(long)row * g.cout + col] : v, act, slope);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// filter gradient:  GW[(t,ci), co] = sum_m X[src(m,t), ci] * GY[m, co]   (split over m, fp32 atomics)
// ---------------------------------------------------------------------------------------------
template <int WM, int WN, int TM, int TN, bool VEC, bool BVEC>
__global__ __launch_bounds__(256) void igemm_wgrad_kernel(CnConvGeom g, const float* __restrict__ X,
                                                          const float* __restrict__ GY, float* __restrict__ GW,
                                                          int rows_per_split, float* __restrict__ parts = nullptr,
                                                          int tiles_x = 0, int tiles_y = 0, int nsplits = 0) {
    static_assert(WM * WN == 4, "4 waves per workgroup");
    constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN, LDA = BM + 4, LDB = BN + 4;
    constexpr int AP = BM / 64, BP = (BN + 63) / 64;
    // XCD-aware order (tiles_x != 0: 1-D launch).  Workgroup id runs on XCD id % 8 (observed dispatch order): every (tap, ci) /
    // cout tile of ONE row slice goes to the same XCD, so the slice of X and GY that all of them read is fetched into that
    // XCD's L2 once instead of once per tile on eight different XCDs (PMC: 4 - 5 x the algorithmic bytes at the fabric with the
    // 3-D grid order).  Placement only affects speed.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (tiles_x) {
        const int T = tiles_x * tiles_y, id = blockIdx.x;
        const int grp = id / (8 * T), r = id - grp * 8 * T;
        bz = grp * 8 + (r & 7);
        if (bz >= nsplits) return;
        const int t = r >> 3;
        by = t / tiles_x;
        bx = t - by * tiles_x;
    }
    __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, half = lane >> 5, l31 = lane & 31;
    const int M = g.n * g.out_d * g.out_h * g.out_w;
    const int T = g.k_d * g.k_h * g.k_w;
    const int Ktot = T * g.cin;
    const int i0 = bx * BM, n0 = by * BN;
    const int mbeg = bz * rows_per_split;
    const int mend = min(M, mbeg + rows_per_split);
    if (mbeg >= mend) return;

    // A loader: float4 along i = (tap, ci); fixed per thread across the whole m loop
    int a_krow[AP], a_col[AP], a_ci[AP][4], a_kd[AP][4], a_kh[AP][4], a_kw[AP][4];
    bool a_ok[AP][4];
#pragma unroll
    for (int ii = 0; ii < AP; ++ii) {
        const int idx = tid + 256 * ii;
        a_krow[ii] = idx / (BM / 4);
        a_col[ii] = (idx % (BM / 4)) * 4;
#pragma unroll
        for (int e = 0; e < (VEC ? 1 : 4); ++e) {
            const int i = i0 + a_col[ii] + e;
            a_ok[ii][e] = i < Ktot;
            const int tap = a_ok[ii][e] ? i / g.cin : 0;
            a_ci[ii][e] = a_ok[ii][e] ? i - tap * g.cin : 0;
            tap_decode(g, tap, a_kd[ii][e], a_kh[ii][e], a_kw[ii][e]);
        }
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float4 ra[AP], rb[BP];
    const int nks = (mend - mbeg + BK - 1) / BK;

    // output coordinates of this thread's gathered row, advanced by BK rows per K step with carries instead of
    // re-dividing the row index every step (load_tiles is called with ks = 0, 1, 2, ... in order)
    int p_m[AP], p_n[AP], p_d[AP], p_h[AP], p_w[AP];
#pragma unroll
    for (int ii = 0; ii < AP; ++ii) {
        int m = mbeg + a_krow[ii];
        p_m[ii] = m;
        divmod_pos(m, g.out_w, m, p_w[ii]);
        divmod_pos(m, g.out_h, m, p_h[ii]);
        divmod_pos(m, g.out_d, p_n[ii], p_d[ii]);
    }

    auto load_tiles = [&](int ks) {
#pragma unroll
        for (int ii = 0; ii < AP; ++ii) {
            RowInfo r;
            r.ok = p_m[ii] < mend;
            r.nbase = p_n[ii] * g.in_d;
            r.vd = p_d[ii] * g.s_d - g.p_d;
            r.vh = p_h[ii] * g.s_h - g.p_h;
            r.vw = p_w[ii] * g.s_w - g.p_w;
            p_m[ii] += BK;
            p_w[ii] += BK;
            while (p_w[ii] >= g.out_w) {
                p_w[ii] -= g.out_w;
                if (++p_h[ii] == g.out_h) {
                    p_h[ii] = 0;
                    if (++p_d[ii] == g.out_d) {
                        p_d[ii] = 0;
                        ++p_n[ii];
                    }
                }
            }
            if (VEC) {
                const int off = a_ok[ii][0] ? src_off(g, r, a_kd[ii][0], a_kh[ii][0], a_kw[ii][0]) : -1;
                ra[ii] = off >= 0 ? *reinterpret_cast<const float4*>(X + off + a_ci[ii][0])
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int off = a_ok[ii][e] ? src_off(g, r, a_kd[ii][e], a_kh[ii][e], a_kw[ii][e]) : -1;
                    v[e] = off >= 0 ? X[off + a_ci[ii][e]] : 0.f;
                }
                ra[ii] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
#pragma unroll
        for (int j = 0; j < BP; ++j) {
            const int idx = tid + 256 * j;
            const int krow = idx / (BN / 4), col = n0 + (idx % (BN / 4)) * 4;
            const int m = mbeg + ks * BK + krow;
            const bool ok = m < mend && idx < BK * BN / 4;
            if (BVEC) {
                rb[j] = (ok && col < g.cout) ? *reinterpret_cast<const float4*>(GY + (long)m * g.cout + col)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (ok && col + e < g.cout) ? GY[(long)m * g.cout + col + e] : 0.f;
                rb[j] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int ii = 0; ii < AP; ++ii) *reinterpret_cast<float4*>(&As[buf][a_krow[ii]][a_col[ii]]) = ra[ii];
#pragma unroll
        for (int j = 0; j < BP; ++j) {
            const int idx = tid + 256 * j;
            if (idx < BK * BN / 4) *reinterpret_cast<float4*>(&Bs[buf][idx / (BN / 4)][(idx % (BN / 4)) * 4]) = rb[j];
        }
    };

    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    const int ac = wm * 32 * TM + l31, bc = wn * 32 * TN + l31;
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nks) load_tiles(ks + 1);
        mma_step<TM, TN, LDA, LDB>(As[buf], Bs[buf], acc, ac, bc, half);
        if (ks + 1 < nks) store_tiles(buf ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * 32 * TN + 32 * j + l31;
        if (col >= g.cout) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rbase = i0 + wm * 32 * TM + 32 * i + 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2);
                if (row >= Ktot) continue;
                // deterministic mode: this split's partial filter goes to its own slab, the slabs are added in split order
                if (parts) parts[((long)bz * Ktot + row) * g.cout + col] = acc[i][j][r];
                else unsafeAtomicAdd(&GW[(long)row * g.cout + col], acc[i][j][r]);
            }
        }
    }
}

// from-RGB conv (3 -> 3): four pixels = three float4 per tensor per trip
__global__ __launch_bounds__(256) void tiny_wgrad_3x3_kernel(const float* __restrict__ X, const float* __restrict__ GY,
                                                             float* __restrict__ GW, long M, float* __restrict__ parts = nullptr) {
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    const long quads = M / 4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        const float4* xp = reinterpret_cast<const float4*>(X + q * 12);
        const float4* gp = reinterpret_cast<const float4*>(GY + q * 12);
        const float4 x0 = xp[0], x1 = xp[1], x2 = xp[2], g0 = gp[0], g1 = gp[1], g2 = gp[2];
        const float xv[12] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w};
        const float gv[12] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[i * 3 + j] += xv[p * 3 + i] * gv[p * 3 + j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long m = quads * 4; m < M; ++m)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) acc[i * 3 + j] += X[m * 3 + i] * GY[m * 3 + j];
    __shared__ float sh[4][9];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[w][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const float v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (parts) parts[blockIdx.x * 9 + threadIdx.x] = v;      // deterministic mode: added in block order afterwards
        else unsafeAtomicAdd(&GW[threadIdx.x], v);
    }
}

// filter gradient of a 1x1 convolution between thin tensors (cin, cout <= 4: the from-RGB conv,
// hologan_discriminator.py:20): a plain HBM-bound reduction gw[ci][co] = sum_m x[m][ci] gy[m][co]
__global__ __launch_bounds__(256) void tiny_wgrad_1x1_kernel(const float* __restrict__ X, const float* __restrict__ GY,
                                                             float* __restrict__ GW, long M, int cin, int cout,
                                                             float* __restrict__ parts = nullptr) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < cin; ++i) xv[i] = X[m * cin + i];
        for (int j = 0; j < cout; ++j) gv[j] = GY[m * cout + j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += xv[i] * gv[j];
    }
    __shared__ float sh[4][16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = acc[i][j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) sh[w][i * 4 + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
        if (i < cin && j < cout) {
            const float v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
            if (parts) parts[blockIdx.x * (cin * cout) + i * cout + j] = v;
            else unsafeAtomicAdd(&GW[i * cout + j], v);
        }
    }
}

// tile cfg of the implicit-GEMM numbering (0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 128x32, 4 = 128x96; anything else: 64x64)
struct Tile { int wm, wn, tm, tn; };
constexpr Tile tile_of(int cfg) {
    return cfg == 0 ? Tile{2, 2, 2, 2} : cfg == 1 ? Tile{2, 2, 2, 1} : cfg == 3 ? Tile{4, 1, 1, 1} : cfg == 4 ? Tile{4, 1, 1, 3} : Tile{2, 2, 1, 1};
}

// grid, tile order (the kernel's xcd_swizzle argument) and offset-table LDS of one igemm_fwd_kernel launch
struct FwdGrid { dim3 grid; int xcd, ntm, ntn; size_t dyn; };
FwdGrid fwd_grid(Tile t, const CnConvGeom& g, bool vec, int par, int splits) {
    const int bm = 32 * t.wm * t.tm, bn = 32 * t.wn * t.tn;
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    FwdGrid f;
    f.grid = dim3(cn_cdiv(M, bm), cn_cdiv(g.cout, bn), splits);
    f.xcd = 1;                                                         // XCD-aware workgroup order
    f.ntm = (int)f.grid.x;
    f.ntn = (int)f.grid.y;
    // cout tiles of one M tile grouped per XCD (several cout tiles), taps inside channel chunks (wide layers on the big tiles:
    // that is where the tap re-reads miss L2; the offset table costs LDS the small tiles' occupancy cannot spare)
    const bool wide = t.tm * t.tn >= 2 && g.cin >= 128;
    if (!par && splits == 1 && f.ntm >= 64 && (f.ntn > 1 || wide)) {
        f.xcd = 2 | (wide ? 4 : 0);
        const int per_xcd = (f.ntm + 7) / 8;
        f.grid = dim3((unsigned)(per_xcd * f.ntn * 8), 1, 1);
    }
    const int taps = g.k_d * g.k_h * g.k_w;
    if ((f.xcd & 4) && (taps < 2 || taps > 9 || !vec)) f.xcd &= ~4;     // (offset table: taps x AP x 1 KiB of LDS)
    f.dyn = (f.xcd & 4) ? sizeof(int) * taps * (bm / (256 / (BK / 4))) * 256 : 0;   // taps x AP x 256 threads
    return f;
}

template <int WM, int WN, int TM, int TN>
int launch_fwd(const CnConvGeom& g, bool vec, int par, int splits, const float* x, const float* w, const float* bias,
               float* y, int act, float slope, hipStream_t s, int bt = 0, long part_stride = 0, const float* res = nullptr) {
    const FwdGrid f = fwd_grid(Tile{WM, WN, TM, TN}, g, vec, par, splits);
    if (vec)
        hipLaunchKernelGGL((igemm_fwd_kernel<WM, WN, TM, TN, true>), f.grid, dim3(256), f.dyn, s, g, x, w, bias, y, act, slope, par, f.xcd, f.ntm, f.ntn, bt, part_stride, res);
    else
        hipLaunchKernelGGL((igemm_fwd_kernel<WM, WN, TM, TN, false>), f.grid, dim3(256), 0, s, g, x, w, bias, y, act, slope, par, f.xcd, f.ntm, f.ntn, 0, 0L, res);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

template <int WM, int WN, int TM, int TN>
void launch_wgrad(const CnConvGeom& g, const float* x, const float* gy, float* gw, int rows, float* parts, int tx, int ty, int splits,
                  dim3 grid, hipStream_t s) {
    const bool avec = g.cin % 4 == 0, bvec = g.cout % 4 == 0;
#define WG(A, B) hipLaunchKernelGGL((igemm_wgrad_kernel<WM, WN, TM, TN, A, B>), grid, dim3(256), 0, s, g, x, gy, gw, rows, parts, tx, ty, splits)
    if (avec && bvec) WG(true, true);
    else if (avec) WG(true, false);
    else if (bvec) WG(false, true);
    else WG(false, false);
#undef WG
}

}  // namespace

// The host entry points of this file (common.h); which of them a convolution gets is conv_dispatch.hip's decision.
int cn_igemm_fwd(int cfg, const CnConvGeom& g, bool vec, int par, int splits, const float* x, const float* w, const float* bias, float* y,
                 int act, float slope, hipStream_t s, int bt, long part_stride, const float* res) {
    switch (cfg) {
        case 3: return launch_fwd<4, 1, 1, 1>(g, vec, par, splits, x, w, bias, y, act, slope, s, bt, part_stride, res);   // 128 x 32
        case 4: return launch_fwd<4, 1, 1, 3>(g, vec, par, splits, x, w, bias, y, act, slope, s, bt, part_stride, res);   // 128 x 96
        case 0: return launch_fwd<2, 2, 2, 2>(g, vec, par, splits, x, w, bias, y, act, slope, s, bt, part_stride, res);   // 128 x 128
        case 1: return launch_fwd<2, 2, 2, 1>(g, vec, par, splits, x, w, bias, y, act, slope, s, bt, part_stride, res);   // 128 x 64
        default: return launch_fwd<2, 2, 1, 1>(g, vec, par, splits, x, w, bias, y, act, slope, s, bt, part_stride, res);  // 64 x 64
    }
}

void cn_igemm_fwd_grid(int cfg, const CnConvGeom& g, bool vec, int par, int splits, int grid[3]) {
    const FwdGrid f = fwd_grid(tile_of(cfg), g, vec, par, splits);
    grid[0] = (int)f.grid.x; grid[1] = (int)f.grid.y; grid[2] = (int)f.grid.z;
}

// zero-stuffed data gradient into a thin image (cout <= 4, parity-ordered rows): per pixel only ~taps/4 * cin MACs, the per-pixel
// bookkeeping of a VALU kernel dominates; the 128x32 MFMA tile with dead-tap skipping and guarded scalar filter loads is faster
int cn_igemm_fwd_thin(const CnConvGeom& g, const float* x, const float* w, const float* bias, float* y, int act, float slope, hipStream_t s) {
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    dim3 grid(cn_cdiv(M, 128), 1, 1);
    hipLaunchKernelGGL((igemm_fwd_kernel<4, 1, 1, 1, true, false>), grid, dim3(256), 0, s, g, x, w, bias, y, act, slope, 1, 1, 0, 0);
    CN_LAUNCH_CHECK();
    return CN_OK;
}

// One launch of the row-split filter gradient on tile cfg with the slices, rows per slice and grid of the plan (tx / ty != 0: the
// XCD-ordered 1-D grid); parts: per-slice partial filters instead of atomics (deterministic mode)
void cn_igemm_wgrad(int cfg, const CnConvGeom& g, const float* x, const float* gy, float* gw, int rows, float* parts, int tx, int ty,
                    int splits, dim3 grid, hipStream_t s) {
    switch (cfg) {
        case 3: return launch_wgrad<4, 1, 1, 1>(g, x, gy, gw, rows, parts, tx, ty, splits, grid, s);       // 128 (tap,ci) x 32 co
        case 4: return launch_wgrad<4, 1, 1, 3>(g, x, gy, gw, rows, parts, tx, ty, splits, grid, s);       // 128 x 96: cout 96 / 192 without column padding
        case 0: return launch_wgrad<2, 2, 2, 2>(g, x, gy, gw, rows, parts, tx, ty, splits, grid, s);       // 128 x 128
        default: return launch_wgrad<2, 2, 1, 1>(g, x, gy, gw, rows, parts, tx, ty, splits, grid, s);      // 64 x 64
    }
}

// filter gradient of the from-RGB shapes (1x1, cin and cout <= 4) on `blocks` workgroups; parts: per-workgroup partials instead of
// atomics.  Returns the workgroups launched (the 3 -> 3 kernel for 16-byte aligned operands runs on at most 512).
int cn_tiny_wgrad(const CnConvGeom& g, const float* x, const float* gy, float* gw, int blocks, float* parts, hipStream_t s) {
    const long M = (long)g.n * g.out_d * g.out_h * g.out_w;
    if (g.cin == 3 && g.cout == 3 && (((uintptr_t)x | (uintptr_t)gy) & 15) == 0) {
        const int nb = blocks > 512 ? 512 : blocks;
        hipLaunchKernelGGL(tiny_wgrad_3x3_kernel, dim3(nb), dim3(256), 0, s, x, gy, gw, M, parts);
        return nb;
    }
    hipLaunchKernelGGL(tiny_wgrad_1x1_kernel, dim3(blocks), dim3(256), 0, s, x, gy, gw, M, g.cin, g.cout, parts);
    return blocks;
}
