"""What tests/test_filter_prep_cases_cpu.py and tests/test_filter_prep_gpu.py share: the derived forms of a convolution filter -- the
tap-flipped copy (cn_conv_weight_tflip), the two bf16 operand copies (cn_conv_weight_prep_bf16), the Winograd F(2x2) and F(4x4)
transforms in their forward and data-gradient layouts (cn_conv_wino_filter, cn_conv_wino4_filter), the parity-class filters of an
upsample-folded layer and the scatter-back of their gradient (cn_upfold_weights, cn_upfold_wgrad) -- and cn_sumpool2, the adjoint of
the x2 nearest upsample.  Plain numpy: nothing here touches a device or the library.

  * one float64 statement of each operation, written from its meaning (never from the kernel);
  * the inputs that make a comparison exact: index-coded integers for the pure permutations (every element distinct, below 2^24),
    integers in [-3, 3] for the sums, multiples of 4 for F(2x2) (two halvings stay whole), the cast table of tests/stream_cases.py
    for the bf16 rounding;
  * the case tables: every row names the smallest shape that reaches one edge -- a channel pair, a tap count, a total next to a
    block of 256, the grid cap of the entry (4096 or 8192 blocks of 256: a second trip of the grid-stride loop) and a ragged block
    past it, every kernel extent the upsample-folded path admits."""
import itertools

import numpy as np

from tests.stream_cases import bf16_bits, bf16_round, cast_table, exact_margin  # noqa: F401  (the GPU test takes them from here)

CN_OK, CN_EINVAL = 0, -1
F32, BF16 = 0, 1
BLOCK = 256
CAP_4096, CAP_8192 = 4096 * BLOCK, 8192 * BLOCK             # elements of one trip of the capped grids


# ---- tap flip and the bf16 operand copies -----------------------------------------------------------------------------------------------
def tflip(w):
    """w[t][ci][co] -> wt[t][co][ci] = w[T - 1 - t][ci][co]: the filter of the data gradient, which runs the taps backwards and
    swaps the channel roles"""
    return np.ascontiguousarray(w[::-1].transpose(0, 2, 1))


def prep_bf16(u):
    """fp32 patterns u[t][ci][co] (uint32) -> (wf[t][co][ci], wd[t][ci][co]) bf16 patterns (uint16): each element rounded to nearest
    even, wd in place and wf with the reduction axis of the forward (ci) contiguous"""
    wd = bf16_bits(u).reshape(u.shape)
    return np.ascontiguousarray(wd.transpose(0, 2, 1)), wd


def table_patterns(taps, cin, cout):
    """fp32 patterns (uint32) [t][ci][co] drawn from the cast table (every bf16 pattern with the low halves exact / just under a
    tie / the tie / just over / the top: both zeros, infinities, NaNs, the carry into the exponent among them), walked with a stride
    coprime to its length: neighbours differ, and 327 680 elements or more hold every row of the table"""
    tab = cast_table()
    i = np.arange(taps * cin * cout, dtype=np.int64)
    return tab[(i * 7919 + 3) % len(tab)].reshape(taps, cin, cout)


def index_coded(shape, start=1):
    """every element distinct: its own flat index + start (the largest stays below 2^24, so fp32 holds each one)"""
    n = int(np.prod(shape))
    assert n + start < 2 ** 24
    return (np.arange(n, dtype=np.float64) + start).reshape(shape)


def small_ints(shape, seed, lim=3, step=1.0):
    return np.random.RandomState(seed).randint(-lim, lim + 1, size=shape).astype(np.float64) * step


# ---- Winograd -----------------------------------------------------------------------------------------------------------------------------
# the standard matrices of F(2x2, 3x3) and F(4x4, 3x3) (Lavin & Gray 2015): Y = A^T [(G g G^T) . (B^T d B)] A
G2 = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
              np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
               np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
WINO = {2: (G2, BT2, AT2), 4: (G4, BT4, AT4)}              # by output tile extent m of F(m x m, 3x3)

# Roundings one term of an output element passes through, in units of 2^-24 relative (each rounding of a sum is relative to the
# computed sum, which is at most the sum of |terms|, so it counts once for every term in it).
#   F(4x4), one stage, the worst row c0 g0 + c1 g1 + c2 g2 with c = 1/24, 1/12, 1/6: the constant is a rounded fp32 (1), its product
#   with g (1), the two adds (2) = 4; the rows c (g0 +- g1 + g2): two adds, the constant, the product = 4 as well; a contraction to
#   fused multiply-adds only removes roundings.  Two stages: 8.
#   F(2x2), one stage: 0.5 (g0 +- g1 + g2): the two adds round, the halving does not = 2.  Two stages: 4.
# The error of the first stage passes through the second stage's |G|, which the bound's |G| |g| |G|^T holds; products of two
# roundings are below 2^-40 of it and go into the slack factor.
WINO_ROUNDINGS = {2: 4, 4: 8}
WINO_SLACK = 1.0 + 2.0 ** -10


def wino_operand(w, dgrad):
    """the 3x3 filter g[a][b][k][n] the transform sees: w[a][b][ci][co] itself (forward: k = ci, n = co) or, for the data gradient,
    the filter of the adjoint convolution: taps flipped on both axes, channel roles swapped (k = co, n = ci)"""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2)) if dgrad else w


def wino_filter(w, m, dgrad, absolute=False):
    """U[plane][k][n] = (G g G^T)[plane] per (k, n); plane = row * (m + 2) + column.  absolute: |G| |g| |G|^T, the scale of the bound"""
    G = WINO[m][0]
    g = wino_operand(w, dgrad)
    if absolute:
        G, g = np.abs(G), np.abs(g)
    return (np.kron(G, G) @ g.reshape(9, -1)).reshape((len(G) ** 2,) + g.shape[2:])


def wino_bound(w, m, dgrad):
    return WINO_ROUNDINGS[m] * 2.0 ** -24 * WINO_SLACK * wino_filter(w, m, dgrad, absolute=True)


def wino_tile(g, d, m):
    """the m x m outputs of one (m + 2) x (m + 2) input tile d through the transforms, for one 3x3 filter g"""
    G, BT, AT = WINO[m]
    return AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T


def direct_tile(g, d, m):
    """the same outputs as a direct (VALID, cross-correlation) 3x3 convolution"""
    return np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(m)] for i in range(m)])


# ---- the upsample-folded layer --------------------------------------------------------------------------------------------------------
def same_pad(k):
    """low padding of a stride-1 SAME convolution with extent k"""
    return (k - 1) // 2


def upfold_axis(k, P):
    """One axis of UpSampling(2, nearest) -> Conv(k, stride 1, low padding P).  Output o = 2 i + p reads the upsampled rows
    o - P + kk, that is the STORED rows i + floor((p - P + kk) / 2); seen from the stored row s, tap kk of parity p lands on
    o = 2 s + tau with tau = p - 2 floor((p - P + kk) / 2).  Returns (tau[kk][p], k2 = tau_max - tau_min + 1, pad2 = -tau_min)."""
    tau = [[p - 2 * ((p - P + kk) // 2) for p in (0, 1)] for kk in range(k)]        # (// floors, also below zero)
    lo, hi = min(min(t) for t in tau), max(max(t) for t in tau)
    return tau, hi - lo + 1, -lo


def upfold_membership(k, P):
    """M[a][kk] = 1 where tap kk maps to class tap a = tau + pad2 (at the one parity tau has): Wc(tau) = sum_kk M[a][kk] w[kk]"""
    tau, k2, pad2 = upfold_axis(k, P)
    M = np.zeros((k2, k))
    for kk in range(k):
        for p in (0, 1):
            M[tau[kk][p] + pad2, kk] = 1.0
    return M


def upfold_weights(w, pads):
    """w[k..][ci][co] (nd = w.ndim - 2 spatial axes), low paddings per axis -> (wf[a'..][ci][co], wd[a..][co][ci], k2 per axis, pad2 per
    axis): wd = the N-D product of the per-axis class sums, transposed; wf = the same taps in reverse order, not transposed"""
    nd = w.ndim - 2
    wc = w
    for ax in range(nd):
        M = upfold_membership(w.shape[ax], pads[ax])
        wc = np.moveaxis(np.tensordot(M, wc, axes=([1], [ax])), 0, ax)
    wd = np.ascontiguousarray(np.swapaxes(wc, -1, -2))
    wf = np.ascontiguousarray(wc[(slice(None, None, -1),) * nd])
    geo = [upfold_axis(w.shape[ax], pads[ax]) for ax in range(nd)]
    return wf, wd, tuple(g[1] for g in geo), tuple(g[2] for g in geo)


def upfold_wgrad(gw2, ks, pads):
    """the adjoint of w -> wd: gw[kk..][ci][co] = the sum over the 2^nd parity combinations of gw2[a(kk, p)..][co][ci]"""
    nd = len(ks)
    geo = [upfold_axis(ks[ax], pads[ax]) for ax in range(nd)]
    cout, cin = gw2.shape[-2:]
    gw = np.zeros(tuple(ks) + (cin, cout))
    for kk in itertools.product(*[range(k) for k in ks]):
        for par in itertools.product((0, 1), repeat=nd):
            a = tuple(geo[ax][0][kk[ax]][par[ax]] + geo[ax][2] for ax in range(nd))
            gw[kk] += gw2[a].T
    return gw


def upsample2(x):
    """nearest x2 on every spatial axis of x[spatial..][c]"""
    for ax in range(x.ndim - 1):
        x = np.repeat(x, 2, axis=ax)
    return x


def conv_same(xu, w, pads):
    """stride-1 cross-correlation of xu[spatial..][ci] with w[k..][ci][co], zero padded (low pads[ax], high k - 1 - pads[ax])"""
    nd = w.ndim - 2
    xp = np.pad(xu, [(pads[ax], w.shape[ax] - 1 - pads[ax]) for ax in range(nd)] + [(0, 0)])
    y = np.zeros(xu.shape[:-1] + (w.shape[-1],))
    for kk in itertools.product(*[range(k) for k in w.shape[:nd]]):
        y += xp[tuple(slice(kk[ax], kk[ax] + xu.shape[ax]) for ax in range(nd))] @ w[kk]
    return y


def class_form_scatter(x, wd, pad2):
    """y[2 s + a - pad2] += wd[a]^T x[s]: the class filters as the data-gradient structure of a stride-2 convolution"""
    nd = x.ndim - 1
    y = np.zeros(tuple(2 * e for e in x.shape[:-1]) + (wd.shape[-2],))
    for s in itertools.product(*[range(e) for e in x.shape[:-1]]):
        for a in itertools.product(*[range(k) for k in wd.shape[:nd]]):
            o = tuple(2 * s[ax] + a[ax] - pad2[ax] for ax in range(nd))
            if all(0 <= o[ax] < y.shape[ax] for ax in range(nd)):
                y[o] += wd[a] @ x[s]
    return y


def class_form_gather(x, wf, pad2):
    """y[o] = sum_a' wf[a'] xs[o + a' - (k2 - 1 - pad2)] on the zero-stuffed xs[2 s] = x[s]: the forward the layer runs"""
    nd = x.ndim - 1
    xs = np.zeros(tuple(2 * e for e in x.shape[:-1]) + (x.shape[-1],))
    xs[(slice(None, None, 2),) * nd] = x
    k2 = wf.shape[:nd]
    return conv_same(xs, wf, [k2[ax] - 1 - pad2[ax] for ax in range(nd)])


def hardcoded_k2(k):
    """what ops.upfold_prepare sizes its class-filter buffer with, per used axis"""
    return k + 1 if k >= 3 else 3


# ---- sumpool2 ---------------------------------------------------------------------------------------------------------------------------
def sumpool2(gu, dt):
    """gu[n][2 d][2 h][2 w][c] (nd = 3) or gu[n][2 h][2 w][c] -> the sum of the 8 / 4 children of every stored cell, rounded once to the
    storage type"""
    sp = gu.shape[1:-1]
    shape = (gu.shape[0],) + tuple(v for e in sp for v in (e // 2, 2)) + (gu.shape[-1],)
    s = gu.reshape(shape).sum(axis=tuple(range(2, 2 + 2 * len(sp), 2)))
    return bf16_round(s) if dt == BF16 else s


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
CHANNEL_PAIRS = [(1, 1), (3, 5), (5, 3), (8, 8), (48, 20)]            # (cin, cout)
TAP_COUNTS = [1, 4, 9, 16, 27]
# (taps, cin, cout) with 255, 256 and 257 elements: one block short by one, one full block, a second block of one element
TOTALS = [(1, 15, 17), (1, 16, 16), (1, 257, 1)]
# one trip of 4096 blocks exactly, and a second trip of four blocks (cn_conv_weight_tflip, cn_conv_weight_prep_bf16)
CAP_4096_CASES = [(1, 1024, 1024), (1, 1025, 1024)]
FLAT_CASES = ([(t, ci, co) for t in TAP_COUNTS for ci, co in CHANNEL_PAIRS] + TOTALS + CAP_4096_CASES)
# the Winograd transforms run one lane per (ci, co): small pairs, the totals next to a block, and past the cap with a ragged last block
# (1023 x 1026 = 4096 x 256 + 1022: three full blocks and one of 254 lanes on the second trip)
WINO_PAIRS = CHANNEL_PAIRS + [(15, 17), (16, 16), (257, 1)]
WINO_CAP_PAIR = (1023, 1026)
WINO_ONEHOT_PAIR = (5, 3)
WINO_ONEHOT_AT = [(0, 0), (4, 2), (2, 1)]                             # (ci, co) positions of the single 1
WINO_REAL_PAIRS = [(3, 5), (48, 20), (64, 64)]

UPFOLD_KS = {2: list(itertools.product((2, 3, 4), repeat=2)), 3: list(itertools.product((2, 3, 4), repeat=3))}
UPFOLD_EXTENTS = [(nd, ks, 3, 5) for nd in (2, 3) for ks in UPFOLD_KS[nd]]          # (nd, extents, cin, cout) at P = (k - 1) // 2
# other low paddings, one extent each: (nd, extents, pads)
UPFOLD_PADS = [(2, (3, 3), (0, 0)), (2, (4, 4), (2, 2)), (2, (2, 3), (1, 0)), (3, (3, 4, 2), (0, 2, 1)), (3, (4, 4, 4), (2, 0, 1))]
# both sides of 8192 blocks: (nd, extents, cin = cout)
UPFOLD_WGRAD_CAP = [(2, (2, 2), 724), (2, (2, 2), 725)]             # 4 c^2 = 2 096 704 and 2 102 500 around 2 097 152
UPFOLD_WEIGHTS_CAP = [(2, (2, 2), 482), (2, (2, 2), 483)]           # 9 c^2 = 2 090 916 and 2 099 601 (k2 = 3 x 3 class taps)
UPFOLD_CHANNELS = [(2, (3, 3), ci, co) for ci, co in CHANNEL_PAIRS] + [(3, (3, 3, 3), 8, 8), (2, (4, 4), 15, 17), (2, (2, 2), 16, 4),
                                                                       (2, (2, 2), 257, 1)]

# (x shape, kernel, cout) as tests/test_ops_gpu.py: UPFOLD_CASES -- odd stored extents, cin = cout = 8: the extents no layer of the
# networks has
UPFOLD_EXTENT_CASES = [((1, 3, 5, 8), k, 8) for k in ((2, 2), (3, 4), (4, 3), (2, 4))] + \
                      [((1, 2, 3, 3, 8), k, 8) for k in ((2, 2, 2), (2, 3, 4), (4, 4, 4), (3, 3, 4))]

# sumpool2: (nd, n, d, h, w, c) of the STORED grid (d = 1 for nd = 2): every extent 1, one vector, totals off a block of 256
SUMPOOL = [(2, 1, 1, 1, 1, 4), (3, 1, 1, 1, 1, 4), (2, 2, 1, 3, 5, 8), (3, 2, 3, 1, 5, 12), (2, 1, 1, 1, 7, 4), (2, 3, 1, 7, 1, 20),
           (3, 1, 5, 3, 1, 4), (2, 1, 1, 16, 16, 4), (2, 1, 1, 257, 1, 4), (3, 2, 3, 5, 7, 12)]


def k3_of(nd, ks):
    """the three-entry extent / padding arrays the C entries take: the depth entry of a 2-D layer is 1 / 0"""
    return (1,) * (3 - nd) + tuple(ks), (0,) * (3 - nd) + tuple(same_pad(k) for k in ks)


def pads3_of(nd, pads):
    return (0,) * (3 - nd) + tuple(pads)


def flat_seed(*dims):
    return 101 + sum((i + 1) * 131 * d for i, d in enumerate(dims)) % 9973


def sumpool_input(row, dt):
    """children: integers in [-3, 3] for fp32 (every sum whole and exact); for bf16 in [-100, 100] -- each one a bf16 value, every partial
    sum whole and below 2^24, the total (up to 800) past the 8 bits of bf16: the one rounding at the store is seen"""
    nd, n, d, h, w, c = row
    shape = (n,) + ((2 * d,) if nd == 3 else ()) + (2 * h, 2 * w, c)
    return small_ints(shape, flat_seed(*row) + dt, lim=100 if dt == BF16 else 3)
