"""What tests/test_stream_cases_cpu.py and tests/test_stream_edges_gpu.py share: the streaming maps, row maps, loss reductions, pools,
GAN losses and the Adam / EMA step of csrc/elementwise.hip.

  * one float64 statement of each operation, written from its meaning (losses.py, perceptual_loss.py, the Keras layers);
  * fp32 -> bf16 round-to-nearest-even as integer arithmetic on uint32, and the cast table (every bf16 pattern x five low halves);
  * the case tables, one per entry: every row names the smallest shapes that reach an edge, the dtype, the misaligned operand and
    the path the launch must take;
  * stream_plan(): the launch decisions of the fourteen entries as they stood inline before plan_stream existed, transcribed
    statement by statement -- never generated from cn_stream_plan, which it pins.

Exactness: inputs are small integers (quarters where an activation output is meant), slopes, scales and coefficients dyadic, so
every term is a multiple of 2^-k and (sum of |terms|) 2^k < 2^24: fp32 holds every partial sum in any order, fused or not, and the
kernels must give the float64 result element for element.  exact_margin() is that condition; the CPU test holds it on every exact
case, together with "the result is representable in the storage type"."""
import itertools

import numpy as np

F32, BF16 = 0, 1
SCALAR, VEC, POOL2 = 0, 1, 2                     # the path codes of cn_stream_plan
NONE, LRELU, RELU, TANH = 0, 1, 2, 3             # CN_ACT_*
CN_OK, CN_EINVAL, CN_EUNSUPPORTED = 0, -1, -3

# the operation codes of cn_stream_plan and the operands whose alignment each entry looks at, in its argument order (bit i of `aligned`)
OPS = ["act_fwd", "act_bwd", "axpby", "mul", "cast", "sqdiff_sum", "row_sumsq", "row_scale", "row_scale_diff", "tap_bwd",
       "maxpool_fwd", "avgpool3_same", "maxpool_bwd", "maxpool2_bwd_act"]
OPERANDS = {"act_fwd": ("x", "y"), "act_bwd": ("gy", "y", "gx"), "axpby": ("x", "y", "out"), "mul": ("x", "y", "out"),
            "cast": ("src", "dst"), "sqdiff_sum": ("a", "b"), "row_sumsq": ("x",), "row_scale": ("x", "out"),
            "row_scale_diff": ("x", "x2", "out"), "tap_bwd": ("y", "target", "g", "out"), "maxpool_fwd": ("x", "y"),
            "avgpool3_same": ("x", "y"), "maxpool_bwd": ("x", "gy", "gx"), "maxpool2_bwd_act": ("x", "gy", "target", "gx")}
PATHS = {op: (SCALAR, VEC) for op in OPS}                        # every path code an entry can report
PATHS["maxpool_bwd"] = (SCALAR, VEC, POOL2)
PATHS["maxpool2_bwd_act"] = (POOL2,)
DTYPES = {op: (F32, BF16) for op in OPS}
DTYPES["row_sumsq"] = (F32,)


def all_aligned(op):
    return (1 << len(OPERANDS[op])) - 1


def mask_of(op, mis):
    """the `aligned` mask of a call whose operand `mis` (a name of OPERANDS[op], or None) is off a vector boundary"""
    return all_aligned(op) & ~(0 if mis is None else 1 << OPERANDS[op].index(mis))


# ---- float64 models -----------------------------------------------------------------------------------------------------------------
def act(x, a, slope):
    if a == LRELU:
        return np.where(x > 0, x, x * slope)
    if a == RELU:
        return np.where(x > 0, x, 0.0)
    if a == TANH:
        return np.tanh(x)
    return x + 0.0


def act_deriv(y, a, slope):
    """the derivative of an activation from its OUTPUT y"""
    if a == LRELU:
        return np.where(y > 0, 1.0, slope)
    if a == RELU:
        return np.where(y > 0, 1.0, 0.0)
    if a == TANH:
        return 1.0 - y * y
    return np.ones_like(y)


def axpby(x, y, a, b):
    return a * x + (b * y if y is not None else 0.0)


def row_scale(x, x2, s, k):
    """(x - x2) s[row] k on (rows, row)"""
    return (x - (x2 if x2 is not None else 0.0)) * s[:, None] * k


def tap_bwd(y, t, g, s, k, a, slope):
    return ((g if g is not None else 0.0) + (y - t) * s[:, None] * k) * act_deriv(y, a, slope)


def masked_diff(a, b, m):
    """(pixels, c) values, (pixels,) uint8 mask"""
    return (a - (b if b is not None else 0.0)) * m.astype(np.float64)[:, None]


def pool_out(h, k, s, pad):
    return (h + 2 * pad - k) // s + 1


def maxpool_fwd(x, k, s, pad):
    """ZeroPadding2D(pad), then a VALID max pool: (n, h, w, c) -> (n, oh, ow, c)"""
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c))
    xp[:, pad:pad + h, pad:pad + w] = x
    oh, ow = pool_out(h, k, s, pad), pool_out(w, k, s, pad)
    y = np.empty((n, oh, ow, c))
    for oy in range(oh):
        for ox in range(ow):
            y[:, oy, ox] = xp[:, oy * s:oy * s + k, ox * s:ox * s + k].reshape(n, k * k, c).max(1)
    return y


def maxpool_bwd(x, gy, k, s, pad):
    """the gradient of every window goes to its first maximum in row-major window order, and nowhere if that cell is padding"""
    n, h, w, c = x.shape
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c))
    xp[:, pad:pad + h, pad:pad + w] = x
    gp = np.zeros_like(xp)
    oh, ow = pool_out(h, k, s, pad), pool_out(w, k, s, pad)
    bi, ci = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
    for oy in range(oh):
        for ox in range(ow):
            arg = xp[:, oy * s:oy * s + k, ox * s:ox * s + k].reshape(n, k * k, c).argmax(1)       # (argmax: the first of equals)
            np.add.at(gp, (bi, oy * s + arg // k, ci * 0 + ox * s + arg % k, ci), gy[:, oy, ox])
    return gp[:, pad:pad + h, pad:pad + w].copy()                  # what fell on the padding is dropped


def maxpool2_bwd_act(x, gy, t, s, k):
    """ReLU -> 2 x 2 / 2 pool backward in one pass: (routed gy + (x - t) s[sample] k) relu'(x), x the ReLU output"""
    r = maxpool_bwd(x, gy, 2, 2, 0)
    if t is not None:
        r = r + (x - t) * (s if len(s) > 1 else np.repeat(s, x.shape[0]))[:, None, None, None] * k
    return r * (x > 0)


def avgpool3_same(x):
    """3 x 3 / stride 1 / SAME average over the cells inside the image: (mean, the integer sum, the count)"""
    n, h, w, c = x.shape
    tot, cnt = np.zeros_like(x), np.zeros((h, w))
    for dy, dx in itertools.product((-1, 0, 1), repeat=2):
        ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
        yd, xd = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
        tot[:, ys, xs] += x[:, yd, xd]
        cnt[ys, xs] += 1
    return tot / cnt[None, :, :, None], tot, cnt


def chan_affine3_fwd(x, perm, scale, off):
    """y[.., j] = scale x[.., perm[j]] + off[j] on (pixels, 3)"""
    return scale * x[:, list(perm)] + np.asarray(off, np.float64)[None, :]


def chan_affine3_bwd(gy, perm, scale):
    """the transpose of the map above: gx[.., perm[j]] += scale gy[.., j]"""
    gx = np.zeros_like(gy)
    for j in range(3):
        gx[:, perm[j]] += scale * gy[:, j]
    return gx


def softplus(x):
    return np.logaddexp(0.0, x)


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gan_terms(s, label):
    """losses.py:7-11: the per-score terms of label softplus(-s) + (1 - label) softplus(s); the loss is their mean"""
    return label * softplus(-s) + (1.0 - label) * softplus(s)


def gan_loss_bwd(s, gout, label):
    return gout * (-label * sigmoid(-s) + (1.0 - label) * sigmoid(s)) / len(s)


def adam_step(th, g, m, v, ema, lr_t, b1, b2, eps, alpha):
    """one Keras Adam step (lr_t already bias-corrected) and the EMA of the new theta: (theta, m, v, ema | None, step)"""
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    step = lr_t * m1 / (np.sqrt(v1) + eps)
    th1 = th - step
    return th1, m1, v1, (None if ema is None else alpha * ema + (1.0 - alpha) * th1), step


def ema_step(ema, th, alpha):
    return alpha * ema + (1.0 - alpha) * th


# ---- fp32 -> bf16, round to nearest even, in integers ---------------------------------------------------------------------------------
def bf16_bits(u):
    """uint32 fp32 patterns -> uint16 bf16 patterns: keep the high half, go up when the low half is past the middle or on the middle
    with an odd high half (a carry walks into the exponent, and from the largest finite value to infinity, by itself); a NaN keeps
    sign and high half and becomes quiet"""
    u = np.asarray(u, np.uint32)
    q, rem = (u >> np.uint32(16)).astype(np.uint32), u & np.uint32(0xFFFF)
    up = (rem > 0x8000) | ((rem == 0x8000) & ((q & 1) == 1))
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, q | np.uint32(0x40), q + up.astype(np.uint32)).astype(np.uint16)


def bf16_round(x):
    """float64 / fp32 values -> the float64 value of their bf16 rounding (through fp32)"""
    bits = bf16_bits(np.asarray(x, np.float32).view(np.uint32)).astype(np.uint32) << np.uint32(16)
    return bits.view(np.float32).astype(np.float64)


def storage_round(x, dt):
    """the single rounding of a float64 result to the storage type"""
    return bf16_round(x) if dt == BF16 else np.asarray(x, np.float32).astype(np.float64)


LOW_HALVES = (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)         # exact, just under the tie, the tie, just over it, the top


def cast_table():
    """every bf16 pattern b with each low half: 327 680 fp32 patterns (uint32), b-major"""
    b = np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)
    return (b | np.asarray(LOW_HALVES, np.uint32)[None, :]).reshape(-1)


def is_nan32(u):
    return (np.asarray(u, np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def is_nan16(b):
    return (np.asarray(b, np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
def exact_margin(terms):
    """(sum of |terms|) 2^k for the smallest k that makes every term a whole number of 2^-k; `terms`: arrays that broadcast against
    each other (every product and addend of one output element; a reduction passes its summed |terms|).  inf if no k <= 40 does."""
    terms = [np.asarray(t, np.float64) for t in terms]
    for k in range(41):
        if all(np.array_equal(t * 2.0 ** k, np.round(t * 2.0 ** k)) for t in terms):
            return float(max(np.max(sum(np.abs(t) for t in terms)), 0.0)) * 2.0 ** k
    return float("inf")


def ints(shape, lo, hi, seed, step=1.0):
    """integers of [lo, hi] times `step`, float64"""
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float64) * step


def sparse_signs(shape, seed):
    """{-1, 0, 1}: what the capped reductions take to stay under 2^24"""
    return ints(shape, -1, 1, seed)


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
CAP_V, CAP_S = 8192 * 256 * 4 + 4 * 300 + 3, 8192 * 256 + 300   # past the 8192 blocks of ew_blocks: 4 per lane / 1 per lane
SMALL = (1, 3, 4, 7, 1027)                                        # a tail only, a full vector, vector + tail, five blocks + tail

# (entry, variant, dtype, misaligned operand, path, numels): variant = the activation (act_*), "y" / "noy" (axpby), the direction (cast)
FLAT = [
    ("act_fwd", LRELU, F32, None, VEC, SMALL + (CAP_V,)),         # aligned: 4 per lane, ragged tail, second trip of the loop
    ("act_fwd", LRELU, BF16, None, VEC, SMALL + (CAP_V,)),
    ("act_fwd", LRELU, F32, "x", SCALAR, SMALL + (CAP_S,)),       # input off by one element: the VEC = false body
    ("act_fwd", LRELU, F32, "y", SCALAR, SMALL),                  # output off by one element
    ("act_fwd", LRELU, BF16, "x", SCALAR, SMALL),
    ("act_fwd", LRELU, BF16, "y", SCALAR, SMALL + (CAP_S,)),
    ("act_fwd", RELU, F32, None, VEC, SMALL),
    ("act_fwd", RELU, BF16, "y", SCALAR, SMALL),
    ("act_fwd", TANH, F32, None, VEC, SMALL),                     # 0 and arguments where tanh is +-1 in fp32
    ("act_fwd", TANH, BF16, "x", SCALAR, SMALL),
    ("act_fwd", "inplace", F32, None, VEC, SMALL),                # y == x
    ("act_fwd", "inplace", BF16, "x", SCALAR, SMALL),             # y == x, both off by one element
    ("act_bwd", LRELU, F32, None, VEC, SMALL + (CAP_V,)),
    ("act_bwd", LRELU, BF16, None, VEC, SMALL + (CAP_V,)),
    ("act_bwd", LRELU, F32, "gy", SCALAR, SMALL + (CAP_S,)),
    ("act_bwd", RELU, F32, "y", SCALAR, SMALL),
    ("act_bwd", TANH, F32, "gx", SCALAR, SMALL),
    ("act_bwd", TANH, BF16, "gy", SCALAR, SMALL + (CAP_S,)),
    ("act_bwd", RELU, BF16, "y", SCALAR, SMALL),
    ("act_bwd", LRELU, BF16, "gx", SCALAR, SMALL),
    ("act_bwd", TANH, F32, None, VEC, SMALL),
    ("act_bwd", RELU, BF16, None, VEC, SMALL),
    ("axpby", "y", F32, None, VEC, SMALL + (CAP_V,)),
    ("axpby", "y", BF16, None, VEC, SMALL + (CAP_V,)),
    ("axpby", "noy", F32, None, VEC, SMALL),                      # y == NULL counts as aligned
    ("axpby", "noy", BF16, None, VEC, SMALL),
    ("axpby", "y", F32, "x", SCALAR, SMALL + (CAP_S,)),
    ("axpby", "y", F32, "y", SCALAR, SMALL),
    ("axpby", "y", F32, "out", SCALAR, SMALL),
    ("axpby", "y", BF16, "x", SCALAR, SMALL),
    ("axpby", "y", BF16, "y", SCALAR, SMALL + (CAP_S,)),
    ("axpby", "y", BF16, "out", SCALAR, SMALL),
    ("axpby", "noy", F32, "out", SCALAR, SMALL),
    ("axpby", "noy", BF16, "x", SCALAR, SMALL),
    ("mul", None, F32, None, VEC, SMALL + (CAP_V,)),
    ("mul", None, BF16, None, VEC, SMALL + (CAP_V,)),
    ("mul", None, F32, "x", SCALAR, SMALL),
    ("mul", None, F32, "y", SCALAR, SMALL + (CAP_S,)),
    ("mul", None, F32, "out", SCALAR, SMALL),
    ("mul", None, BF16, "x", SCALAR, SMALL + (CAP_S,)),
    ("mul", None, BF16, "y", SCALAR, SMALL),
    ("mul", None, BF16, "out", SCALAR, SMALL),
    # cast: dtype = the SOURCE type; values that bf16 holds, so the maps are exact (the rounding itself: the cast table)
    ("cast", "to_bf16", F32, None, VEC, SMALL + (CAP_V,)),
    ("cast", "to_bf16", F32, "src", SCALAR, SMALL + (CAP_S,)),
    ("cast", "to_bf16", F32, "dst", SCALAR, SMALL),
    ("cast", "to_f32", BF16, None, VEC, SMALL + (CAP_V,)),
    ("cast", "to_f32", BF16, "src", SCALAR, SMALL),
    ("cast", "to_f32", BF16, "dst", SCALAR, SMALL + (CAP_S,)),
]

ROW_CAP = 512 * 4096 + 4096 + 8                                   # past the 512 blocks per row of the row maps
ROWS = (4, 5, 4096 + 1024 + 4, 4096 + 1024 + 5)                   # one vector, not a multiple of 4, two blocks with a ragged second one
# (entry, variant, dtype, misaligned operand, rows, row lengths -> path: row % 4 == 0 and every operand aligned is VEC)
# variant: None, or (g given, activation) for tap_bwd
ROW = [
    ("row_scale", None, F32, None, 3, ROWS),                      # rows 4 and 5124 VEC, 5 and 5125 SCALAR (row % 4)
    ("row_scale", None, BF16, None, 3, ROWS),
    ("row_scale", None, F32, None, 1, (4, ROW_CAP)),              # the cap: a second trip of the block loop, vector path
    ("row_scale", None, BF16, "x", 1, (4, ROW_CAP)),              # the cap on the scalar path, bf16
    ("row_scale", None, F32, "x", 3, ROWS),
    ("row_scale", None, F32, "out", 3, ROWS),
    ("row_scale", None, BF16, "out", 1, ROWS),
    ("row_scale_diff", None, F32, None, 3, ROWS),
    ("row_scale_diff", None, BF16, None, 3, ROWS),
    ("row_scale_diff", None, BF16, None, 1, (4, ROW_CAP)),
    ("row_scale_diff", None, F32, "x2", 1, (4, ROW_CAP)),
    ("row_scale_diff", None, F32, "x", 3, ROWS),
    ("row_scale_diff", None, F32, "x2", 3, ROWS),
    ("row_scale_diff", None, F32, "out", 1, ROWS),
    ("row_scale_diff", None, BF16, "x", 1, ROWS),
    ("row_scale_diff", None, BF16, "x2", 3, ROWS),
    ("row_scale_diff", None, BF16, "out", 3, ROWS),
    ("tap_bwd", (True, RELU), F32, None, 3, ROWS),
    ("tap_bwd", (False, RELU), F32, None, 3, ROWS),               # g == NULL counts as aligned
    ("tap_bwd", (True, LRELU), BF16, None, 3, ROWS),
    ("tap_bwd", (False, TANH), BF16, None, 1, ROWS),
    ("tap_bwd", (True, TANH), F32, None, 1, (4, ROW_CAP)),
    ("tap_bwd", (True, RELU), BF16, "g", 1, (4, ROW_CAP)),
    ("tap_bwd", (True, LRELU), F32, "y", 3, ROWS),
    ("tap_bwd", (True, TANH), F32, "target", 3, ROWS),
    ("tap_bwd", (True, RELU), F32, "g", 1, ROWS),
    ("tap_bwd", (False, LRELU), F32, "out", 3, ROWS),
    ("tap_bwd", (True, TANH), BF16, "y", 3, ROWS),
    ("tap_bwd", (False, RELU), BF16, "target", 1, ROWS),
    ("tap_bwd", (True, LRELU), BF16, "g", 3, ROWS),
    ("tap_bwd", (True, RELU), BF16, "out", 3, ROWS),
]

SQ_CAP_V, SQ_CAP_S = 512 * 256 * 4 + 4 * 300 + 3, 512 * 256 + 300   # past the 512 blocks of cn_sqdiff_sum
# (dtype, misaligned operand, path, numels); every row runs in default and in deterministic mode, out = 5 before, scale = 0.25
SQDIFF = [
    (F32, None, VEC, (1, 5, 1027, SQ_CAP_V)),
    (BF16, None, VEC, (1, 5, 1027, SQ_CAP_V)),
    (F32, "a", SCALAR, (1, 5, 1027, SQ_CAP_S)),
    (F32, "b", SCALAR, (1, 5, 1027)),
    (BF16, "a", SCALAR, (1, 5, 1027)),
    (BF16, "b", SCALAR, (1, 5, 1027, SQ_CAP_S)),
]
SUMSQ_CAP = 64 * 8192 + 8192 + 4                                  # past the 64 blocks per row of cn_row_sumsq
# (misaligned operand, rows, row lengths): row % 4 == 0 and x aligned is VEC; both modes, out = NaN before
ROW_SUMSQ = [
    (None, 3, (4, 5, 8192 + 4)),                                  # 4 and 8196 VEC, 5 SCALAR
    (None, 1, (4, 5, 8192 + 4, SUMSQ_CAP)),
    ("x", 3, (4, 5, 8192 + 4)),
    ("x", 1, (4, SUMSQ_CAP)),
]

# (c, b given, pixels)
MASKED_DIFF = [(c, b, p) for c in (1, 3, 5) for b in (False, True) for p in (1, 257)]

# data kinds of the pools: distinct values of both signs (padding wins at negative borders), {0, 1, 2} (every window full of ties),
# all negative
MIXED, TIES, NEG = "mixed", "ties", "neg"
# (n, h, w, c, k, s, pad, dtype, misaligned operand, data, forward path, backward path)
MAXPOOL = [
    (2, 2, 2, 4, 2, 2, 0, F32, None, MIXED, VEC, POOL2),          # oh = ow = 1
    (2, 8, 2, 12, 2, 2, 0, BF16, None, TIES, VEC, POOL2),         # ties on the 2 x 2 kernel
    (1, 7, 3, 4, 2, 2, 0, F32, None, MIXED, VEC, VEC),            # odd extents: the last row and column are in no window
    (1, 7, 8, 12, 2, 2, 0, BF16, None, NEG, VEC, VEC),            # odd height only
    (2, 8, 8, 8, 2, 2, 0, F32, "x", TIES, SCALAR, SCALAR),        # c = 8 misaligned: the scalar kernels with c % 4 == 0
    (2, 8, 8, 8, 2, 2, 0, BF16, "gx", MIXED, VEC, SCALAR),        # (the forward does not see gx)
    (1, 8, 8, 8, 2, 2, 0, F32, "gy", MIXED, SCALAR, SCALAR),      # (the forward: its output y, which has gy's shape, off by one)
    (1, 2, 3, 1, 2, 2, 0, F32, None, MIXED, SCALAR, SCALAR),
    (2, 8, 13, 3, 2, 2, 0, BF16, None, TIES, SCALAR, SCALAR),
    (2, 7, 7, 4, 3, 2, 1, F32, None, MIXED, VEC, VEC),            # ResNet-50's pool: padding wins where a border window is negative
    (2, 8, 8, 12, 3, 2, 1, BF16, None, MIXED, VEC, VEC),          # even extents with pad 1: the last padding row is in no window
    (2, 8, 7, 4, 3, 2, 1, F32, None, TIES, VEC, VEC),             # ties on the 4-channel kernel, against zero padding too
    (1, 13, 8, 12, 3, 2, 1, F32, None, NEG, VEC, VEC),            # all negative: every border window gives zero and routes nowhere
    (2, 7, 8, 6, 3, 2, 1, F32, None, MIXED, SCALAR, SCALAR),
    (2, 8, 13, 3, 3, 2, 1, BF16, None, TIES, SCALAR, SCALAR),     # ties on the scalar kernel
    (1, 3, 2, 1, 3, 2, 1, BF16, None, NEG, SCALAR, SCALAR),       # oh = ow = 1 with padding on every side
    (1, 8, 8, 8, 3, 2, 1, BF16, "x", NEG, SCALAR, SCALAR),
    (2, 7, 7, 12, 3, 2, 0, F32, None, MIXED, VEC, VEC),           # overlapping rows and columns, no padding
    (2, 8, 8, 4, 3, 2, 0, BF16, None, TIES, VEC, VEC),            # (8 - 3) % 2: the last row and column are in no window
    (1, 8, 13, 6, 3, 2, 0, F32, None, MIXED, SCALAR, SCALAR),
    (1, 3, 3, 3, 3, 2, 0, BF16, None, MIXED, SCALAR, SCALAR),     # one window
    (2, 7, 8, 4, 3, 1, 1, F32, None, MIXED, VEC, VEC),            # stride 1: one element collects from up to nine windows
    (1, 3, 7, 12, 3, 1, 1, BF16, None, TIES, VEC, VEC),
    (2, 8, 7, 1, 3, 1, 1, F32, None, TIES, SCALAR, SCALAR),
    (1, 13, 2, 6, 3, 1, 1, BF16, None, NEG, SCALAR, SCALAR),
    (1, 8, 8, 8, 3, 1, 1, F32, "gy", MIXED, SCALAR, SCALAR),
]
FWD_MIS = {"x": "x", "gy": "y"}                                   # the operand the forward run of a row misaligns

# (n, h, w, c, dtype, target given, s_rows, misaligned operand) -> CN_OK on POOL2, or the refusal
POOL2_ACT = [
    (2, 2, 2, 4, F32, False, 1, None, CN_OK),
    (3, 8, 2, 12, BF16, False, 1, None, CN_OK),                   # bf16, no target
    (3, 2, 8, 4, F32, True, 3, None, CN_OK),                      # a scale per sample
    (3, 8, 8, 8, F32, True, 1, None, CN_OK),                      # one scale for every sample under a target
    (3, 2, 8, 12, BF16, True, 3, None, CN_OK),
    (2, 8, 2, 4, BF16, True, 1, None, CN_OK),
    (2, 7, 8, 4, F32, True, 1, None, CN_EUNSUPPORTED),            # odd h
    (2, 8, 13, 4, BF16, False, 1, None, CN_EUNSUPPORTED),         # odd w
    (2, 8, 8, 6, F32, True, 2, None, CN_EUNSUPPORTED),            # c % 4
    (2, 8, 8, 8, F32, True, 2, "x", CN_EUNSUPPORTED),
    (2, 8, 8, 8, BF16, True, 1, "gy", CN_EUNSUPPORTED),
    (2, 8, 8, 8, F32, True, 2, "target", CN_EUNSUPPORTED),
    (2, 8, 8, 8, BF16, False, 1, "gx", CN_EUNSUPPORTED),
]

# (n, h, w, c, dtype, misaligned operand, path): the extents give windows of 1, 2, 3, 4, 6 and 9 cells
AVGPOOL = [
    (2, 1, 1, 4, F32, None, VEC), (2, 1, 2, 8, BF16, None, VEC), (1, 2, 2, 4, F32, None, VEC), (2, 1, 3, 8, F32, None, VEC),
    (1, 2, 3, 4, BF16, None, VEC), (2, 3, 5, 8, F32, None, VEC), (1, 5, 5, 4, BF16, None, VEC), (3, 5, 5, 8, F32, None, VEC),
    (2, 1, 1, 1, F32, None, SCALAR), (2, 2, 1, 3, BF16, None, SCALAR), (1, 3, 3, 1, F32, None, SCALAR), (2, 5, 2, 3, F32, None, SCALAR),
    (2, 5, 5, 3, BF16, None, SCALAR), (2, 3, 5, 8, F32, "x", SCALAR), (1, 5, 3, 4, BF16, "y", SCALAR),
]
AVG_COUNTS = {1, 2, 3, 4, 6, 9}

PERMS = list(itertools.permutations(range(3)))
AFFINE_PIXELS = (1, 257)

GAN_N = (1, 63, 64, 65, 256, 257, 600)                            # one lane ... a wavefront +- 1 ... the block +- 1 ... a third trip
GAN_LABELS = (0.0, 1.0)
GAN_SPECIAL = (0.0, -0.0, 30.0, -30.0, 100.0, -100.0)             # both zeros, where softplus / sigmoid saturate in fp32, and far past
GAN_GROUPS = (1, 16, 17)                                          # one job, a full launch, a second launch of one job

ADAM_N = (1, 255, 257, 8192 * 256 + 300)
ADAM_BETAS = ((0.0, 0.9), (0.9, 0.999), (0.5, 0.9))
ADAM_LR, ADAM_EPS, EMA_ALPHA = 1e-3, 1e-7, 0.999


def gan_scores(n, seed):
    """fp32 scores: ordinary ones (normal, sigma 3) with every GAN_SPECIAL value put in where there is room"""
    s = (np.random.RandomState(seed).randn(n) * 3).astype(np.float32)
    k = min(n, len(GAN_SPECIAL))
    s[np.linspace(0, n - 1, k).astype(int)] = np.asarray(GAN_SPECIAL[:k], np.float32)
    return s


def adam_state(n, seed):
    """a drawn fp32 state (theta, g, m, v, ema): v >= 0, m of either sign; element 0 (and every 97th) has v = 0 with g = 0, element 1
    (and every 97th after it) v = 0 with |g| << eps"""
    r = np.random.RandomState(seed)
    th, g, m = (r.randn(n).astype(np.float32) for _ in range(3))
    v = (r.rand(n) * 2).astype(np.float32) ** 2
    ema = r.randn(n).astype(np.float32)
    v[0::97], g[0::97] = 0.0, 0.0
    v[1::97], g[1::97] = 0.0, np.float32(1e-12)
    return th, g * np.float32(0.1), m * np.float32(0.1), v, ema


def pool_data(kind, shape, seed):
    if kind == TIES:
        return ints(shape, 0, 2, seed)
    r = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if kind == NEG:
        return -(r.permutation(n) % 120 + 1).astype(np.float64).reshape(shape)        # -120 .. -1 (bf16 holds them)
    x = ((r.permutation(n) % 241) - 120).astype(np.float64).reshape(shape)             # -120 .. 120; distinct while n <= 241
    x[:, :2, :2] = -np.abs(x[:, :2, :2]) - 1                                           # the corner window is negative: zero padding wins it
    return x


# ---- the inputs of a table row: (operands in the entry's order (None: absent), scalars, float64 result, terms for exact_margin) ------
SLOPE, AX_A, AX_B = 0.25, 0.5, -1.5
ROW_S, ROW_K = (0.5, 2.0, -1.5), 0.25                             # per-row scales that differ, and the common factor
TAP_S, TAP_K = (0.5, 2.0, -1.0), 0.5
TANH_ARGS = np.asarray([0.0, 16.0, -16.0, 32.0, -32.0, 64.0, -64.0])   # tanh is 0 or +-1 after the rounding to fp32


def flat_case(entry, variant, dt, numel):
    seed = numel % 9973 + 17 * OPS.index(entry) + dt
    x, y = ints(numel, -8, 8, seed), ints(numel, -8, 8, seed + 1)
    if entry == "act_fwd":
        a = LRELU if variant == "inplace" else variant
        if a == TANH:
            x = TANH_ARGS[np.random.RandomState(seed).randint(0, len(TANH_ARGS), numel)]
        want = storage_round(act(x, a, SLOPE), dt)                # (the rounding is the identity but for tanh(+-16 ..) = +-1)
        return [x], (a, SLOPE), want, [want]
    if entry == "act_bwd":
        a, out = variant, ints(numel, -4, 4, seed + 2, 0.25)      # an activation OUTPUT: quarters in [-1, 1]
        want = x * act_deriv(out, a, SLOPE)
        return [x, out], (a, SLOPE), want, [out * out, want]
    if entry == "axpby":
        y = y if variant == "y" else None
        return [x, y], (AX_A, AX_B), axpby(x, y, AX_A, AX_B), [AX_A * x] + ([AX_B * y] if y is not None else [])
    if entry == "mul":
        return [x, y], (), x * y, [x * y]
    if entry == "cast":
        x = ints(numel, -128, 128, seed, 0.25)                    # bf16 holds them
        return [x], (), x, [x]
    raise ValueError(entry)


def row_case(entry, variant, dt, rows, row):
    seed = row % 9973 + 17 * OPS.index(entry) + dt + rows
    if entry in ("row_scale", "row_scale_diff"):
        x, x2 = ints((rows, row), -8, 8, seed), (ints((rows, row), -8, 8, seed + 1) if entry == "row_scale_diff" else None)
        s = np.asarray(ROW_S[:rows])
        want = row_scale(x, x2, s, ROW_K)
        return [x, x2], (s, ROW_K), want, [x - (x2 if x2 is not None else 0.0), (s * ROW_K)[:, None], want]
    has_g, a = variant
    q = 0.5 if a == TANH else 1.0                                 # tanh outputs: halves in [-1, 1], so 1 - y^2 is 0, 3/4 or 1
    lim = 2 if a == TANH else 4
    y, t = ints((rows, row), -lim, lim, seed, q), ints((rows, row), -lim, lim, seed + 1, q)
    g = ints((rows, row), -3, 3, seed + 2) if has_g else None
    s = np.asarray(TAP_S[:rows])
    want = tap_bwd(y, t, g, s, TAP_K, a, SLOPE)
    return [y, t, g], (s, TAP_K, a, SLOPE), want, [(y - t) * s[:, None] * TAP_K, g if has_g else 0.0 * y, y * y, want]


SQ_PRESET, SQ_SCALE = 5.0, 0.25


def sqdiff_case(dt, numel):
    b = ints(numel, -4, 4, numel % 9973 + dt)
    a = b + sparse_signs(numel, numel % 9973 + dt + 1)
    total = float(((a - b) ** 2).sum())
    return [a, b], SQ_PRESET + SQ_SCALE * total, [np.asarray(SQ_PRESET), np.asarray(SQ_SCALE * total)]


def sumsq_case(rows, row):
    x = ints((rows, row), -2, 2, row % 9973 + rows)
    want = (x * x).sum(1)
    return x, want, [want]


def masked_diff_case(c, has_b, pixels):
    a, b = ints((pixels, c), -8, 8, pixels + c), (ints((pixels, c), -8, 8, pixels + c + 1) if has_b else None)
    m = np.random.RandomState(pixels + c + 2).choice([0, 1, 1, 3], pixels).astype(np.uint8)
    return a, b, m, masked_diff(a, b, m)


def maxpool_case(row):
    n, h, w, c, k, s, pad, dt, mis, kind = row[:10]
    x = pool_data(kind, (n, h, w, c), h * 31 + w * 7 + c + k + pad)
    oh, ow = pool_out(h, k, s, pad), pool_out(w, k, s, pad)
    gy = ints((n, oh, ow, c), -4, 4, h * 31 + w * 7 + c + 1)
    gy[gy == 0] = 1.0                                             # (a misrouted gradient always shows)
    return x, gy, maxpool_fwd(x, k, s, pad), maxpool_bwd(x, gy, k, s, pad)


def pool2_act_case(row):
    n, h, w, c, dt, has_t, s_rows, mis, rc = row
    seed = h * 31 + w * 7 + c + s_rows
    x = np.maximum(ints((n, h, w, c), -3, 6, seed), 0.0)           # a ReLU output: zeros among the positives
    gy = ints((n, h // 2, w // 2, c), -4, 4, seed + 1)
    t = ints((n, h, w, c), 0, 6, seed + 2) if has_t else None
    s = np.asarray(ROW_S[:s_rows]) if has_t else None
    want = maxpool2_bwd_act(x, gy, t, s, ROW_K) if rc == CN_OK else None
    return x, gy, t, s, want


def avgpool_case(row):
    n, h, w, c = row[:4]
    return ints((n, h, w, c), -8, 8, h * 31 + w * 7 + c)


AVG_ROUNDINGS = 3       # units of 2^-24 relative: the reciprocal 1.f / cnt counts one ulp (2), the product acc * r one rounding (1)


def avgpool_bound(mean, dt):
    """the sum of integers is exact; |error| <= AVG_ROUNDINGS 2^-24 |mean| in fp32.  bf16 adds ONE rounding to nearest of the fp32
    value: half a bf16 ulp of its binade, 2^(e - 8) for 2^e <= |value| < 2^(e + 1) (8 significant bits) -- up to 2^-8 of the value,
    not 2^-9: 7/3 lies 5.2e-3 from its nearest bf16 neighbour 2.328125, 2^-8.8 of it (tests/test_stream_cases_cpu.py shows it on
    torch's own rounding)"""
    a = np.abs(mean)
    bound = a * (AVG_ROUNDINGS * 2.0 ** -24)
    if dt == BF16:
        top = a + bound                                           # (the fp32 value may sit in the next binade)
        bound = bound + np.where(top > 0, 2.0 ** (np.floor(np.log2(np.where(top > 0, top, 1.0))) - 8), 0.0)
    return bound


AFFINE_SCALE, AFFINE_OFF = 0.5, (1.0, -2.0, 0.5)


def gan_yardstick(s32, label, gout=None):
    """the same expression term by term in torch float32 on the CPU: forward (summed in float64, / n), or the per-score gradient"""
    import torch
    import torch.nn.functional as F
    s = torch.from_numpy(np.asarray(s32, np.float32))
    lab = torch.tensor(label, dtype=torch.float32)
    if gout is None:
        terms = lab * F.softplus(-s) + (1.0 - lab) * F.softplus(s)
        return float(terms.double().sum()) / len(s32)
    g = torch.tensor(gout, dtype=torch.float32)
    return (g * (-lab * torch.sigmoid(-s) + (1.0 - lab) * torch.sigmoid(s)) / float(len(s32))).double().numpy()


GAN_FACTOR = 4.0        # a different libm and the fp32 order of the sum


def gan_fwd_bound(s32, label):
    """(float64 loss, bound on |error|, the yardstick's own error)"""
    terms = gan_terms(np.asarray(s32, np.float64), label)
    ref = float(terms.mean())
    yard = abs(gan_yardstick(s32, label) - ref)
    return ref, max(GAN_FACTOR * yard, len(s32) * 2.0 ** -24 * float(np.abs(terms).mean())), yard


def gan_bwd_bound(s32, gout, label):
    """(float64 gradient, per-element bound, the yardstick's own per-element error)"""
    ref = gan_loss_bwd(np.asarray(s32, np.float64), float(np.float32(gout)), label)
    yard = np.abs(gan_yardstick(s32, label, gout) - ref)
    return ref, np.maximum(GAN_FACTOR * yard, 4 * 2.0 ** -24 * np.abs(ref)), yard


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


ADAM_STEP_ROUNDINGS = 5   # ulps (2^-23) on the step lr m / (sqrt(v) + eps): v carries 5 half-ulps (b2 v: 1, (1 - b2) g g: 3, the sum: 1)
#                           = 2.5 ulps, halved by the root: 1.25; the root 1; + eps 0.5; lr m 0.5; the division 1: 4.25, rounded up


def adam_bounds(th, g, m, v, ema, lr_t, b1, b2, eps, alpha):
    """float64 step from the fp32 state and fp32 coefficients, and per-element bounds on |kernel - float64|, each rounding 2^-24 relative
    of what it rounds (second-order terms: a factor 1 + 2^-10 on the whole):
      m:     b1 m 1, (1 - b1) g 2 (the subtraction, the product), the sum 1
      v:     b2 v 1, (1 - b2) g g 3, the sum 1
      theta: half an ulp of the new theta + ADAM_STEP_ROUNDINGS 2^-23 |step| + what the bound of m moves the step (lr dm / (sqrt(v) + eps);
             m may cancel, so its error is carried as an absolute one)
      ema:   alpha ema 1, (1 - alpha) theta 2, the sum 1, + (1 - alpha) times the bound of theta"""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    th, g, m, v, lr_t, b1, b2, eps, alpha = (f(a) for a in (th, g, m, v, lr_t, b1, b2, eps, alpha))
    ema = None if ema is None else f(ema)
    th1, m1, v1, ema1, step = adam_step(th, g, m, v, ema, lr_t, b1, b2, eps, alpha)
    u, slack = 2.0 ** -24, 1.0 + 2.0 ** -10
    bm = u * (np.abs(b1 * m) + 2 * np.abs((1 - b1) * g) + np.abs(b1 * m) + np.abs((1 - b1) * g)) * slack
    bv = u * (np.abs(b2 * v) + 3 * np.abs((1 - b2) * g * g) + v1) * slack
    bth = (0.5 * ulp32(th1) + ADAM_STEP_ROUNDINGS * 2.0 ** -23 * np.abs(step) + lr_t * bm / (np.sqrt(v1) + eps)) * slack
    out = {"theta": (th1, bth), "m": (m1, bm), "v": (v1, bv)}
    if ema is not None:
        out["ema"] = (ema1, (u * (np.abs(alpha * ema) + 2 * np.abs((1 - alpha) * th1) + np.abs(ema1)) + (1 - alpha) * bth) * slack)
    return out


def ema_bound(ema, th, alpha):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    ema, th, alpha = f(ema), f(th), f(alpha)
    e1 = ema_step(ema, th, alpha)
    return e1, 2.0 ** -24 * (np.abs(alpha * ema) + 2 * np.abs((1 - alpha) * th) + np.abs(e1)) * (1.0 + 2.0 ** -10)


def plan_requests():
    """every launch of the tables: (what, op, dtype, rows, row, c, h, w, k, s, pad, misaligned operand, the path the row claims or the
    refusal)"""
    out = []
    for entry, variant, dt, mis, path, numels in FLAT:
        out += [("%s %s" % (entry, variant), entry, dt, 1, n, 0, 0, 0, 0, 0, 0, mis, path) for n in numels]
    for entry, variant, dt, mis, rows, lens in ROW:
        out += [("%s %s" % (entry, variant), entry, dt, rows, r, 0, 0, 0, 0, 0, 0, mis, VEC if mis is None and r % 4 == 0 else SCALAR) for r in lens]
    for dt, mis, path, numels in SQDIFF:
        out += [("sqdiff_sum", "sqdiff_sum", dt, 1, n, 0, 0, 0, 0, 0, 0, mis, path) for n in numels]
    for mis, rows, lens in ROW_SUMSQ:
        out += [("row_sumsq", "row_sumsq", F32, rows, r, 0, 0, 0, 0, 0, 0, mis, VEC if mis is None and r % 4 == 0 else SCALAR) for r in lens]
    for n, h, w, c, k, s, pad, dt, mis, kind, fpath, bpath in MAXPOOL:
        out.append(("maxpool_fwd " + kind, "maxpool_fwd", dt, n, 0, c, h, w, k, s, pad, FWD_MIS.get(mis), fpath))
        out.append(("maxpool_bwd " + kind, "maxpool_bwd", dt, n, 0, c, h, w, k, s, pad, mis, bpath))
    for n, h, w, c, dt, has_t, s_rows, mis, rc in POOL2_ACT:
        out.append(("maxpool2_bwd_act", "maxpool2_bwd_act", dt, n, 0, c, h, w, 2, 2, 0, mis, POOL2 if rc == CN_OK else rc))
    for n, h, w, c, dt, mis, path in AVGPOOL:
        out.append(("avgpool3_same", "avgpool3_same", dt, n, 0, c, h, w, 3, 1, 1, mis, path))
    return out


# ---- the launch rule, transcribed ----------------------------------------------------------------------------------------------------
def ew_blocks(n):
    b = (n + 255) // 256
    return 8192 if b > 8192 else (b if b else 1)


def cdiv_c(a, b):
    """C's integer division, which rounds towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def stream_plan(op, dt, rows, row, c, h, w, k, s, pad, aligned, det):
    """(return code, [path, grid x, grid y, floats of deterministic partials]) of the entry `op` -- flat maps and reductions: row =
    numel; row maps: rows x row; pools: rows = n -- as the entry decided inline"""
    al = (aligned & all_aligned(op)) == all_aligned(op)
    if op in ("act_fwd", "act_bwd", "axpby", "mul", "cast"):
        vec = al
        return CN_OK, [VEC if vec else SCALAR, ew_blocks((row + 3) // 4 if vec else row), 1, 0]
    if op == "sqdiff_sum":
        vec = al
        blocks = ew_blocks(row // (4 if vec else 1) + 1)
        if blocks > 512:
            blocks = 512
        return CN_OK, [VEC if vec else SCALAR, blocks, 1, blocks if det else 0]
    if op == "row_sumsq":
        vec = al and row % 4 == 0
        bpr = (row + 256 * 32 - 1) // (256 * 32)
        if bpr > 64:
            bpr = 64
        return CN_OK, [VEC if vec else SCALAR, bpr, rows, bpr * rows if det else 0]
    if op in ("row_scale", "row_scale_diff", "tap_bwd"):
        vec = al and row % 4 == 0
        bpr = (row + 256 * 16 - 1) // (256 * 16)
        if bpr > 512:
            bpr = 512
        return CN_OK, [VEC if vec else SCALAR, bpr, rows, 0]
    n = rows
    if op == "maxpool_fwd":
        oh, ow = cdiv_c(h + 2 * pad - k, s) + 1, cdiv_c(w + 2 * pad - k, s) + 1
        total = n * oh * ow * c
        if c % 4 == 0 and al and total // 4 < (1 << 30) and n * h * w * c // 4 < (1 << 30):
            return CN_OK, [VEC, ew_blocks(total // 4), 1, 0]
        return CN_OK, [SCALAR, ew_blocks(total), 1, 0]
    if op == "avgpool3_same":
        v4 = c % 4 == 0 and al
        return CN_OK, [VEC if v4 else SCALAR, ew_blocks(n * h * w * (c // 4 if v4 else c)), 1, 0]
    if op == "maxpool_bwd":
        oh, ow = cdiv_c(h + 2 * pad - k, s) + 1, cdiv_c(w + 2 * pad - k, s) + 1
        total = n * h * w * c
        if k == 2 and s == 2 and pad == 0 and h % 2 == 0 and w % 2 == 0 and c % 4 == 0 and al:
            return CN_OK, [POOL2, ew_blocks(n * oh * ow * (c // 4)), 1, 0]
        if c % 4 == 0 and al and total // 4 < 2147483647:
            return CN_OK, [VEC, ew_blocks(total // 4), 1, 0]
        return CN_OK, [SCALAR, ew_blocks(total), 1, 0]
    if op == "maxpool2_bwd_act":
        if h % 2 or w % 2 or c % 4 or not al:
            return CN_EUNSUPPORTED, None
        return CN_OK, [POOL2, ew_blocks(n * (h // 2) * (w // 2) * (c // 4)), 1, 0]
    raise ValueError(op)


def alv(p, dt):
    """static inline bool alv(const void* p, int dt): 4-wide access needs 16 (fp32) / 8 (bf16) bytes; NULL (None) counts as aligned"""
    return ((p or 0) & (7 if dt == BF16 else 15)) == 0


def entry_aligned(op, dt, dst_dt, p):
    """the alignment term of each entry's launch condition AS THE ENTRY WROTE IT INLINE before plan_stream existed, on the addresses
    p of its tensor operands in argument order (OPERANDS[op]; None: NULL) -- transcribed entry by entry, the pin of the mask code the
    entries share now (stream_mask, through cn_stream_plan_ptrs)"""
    if op == "act_fwd":
        return alv(p[0], dt) and alv(p[1], dt)                                   # alv(x, dt) && alv(y, dt)
    if op == "act_bwd":
        return alv(p[0], dt) and alv(p[1], dt) and alv(p[2], dt)                 # alv(gy, dt) && alv(y, dt) && alv(gx, dt)
    if op in ("axpby", "mul"):
        return alv(p[0], dt) and alv(p[1], dt) and alv(p[2], dt)                 # alv(x, dt) && alv(y, dt) && alv(out, dt)
    if op == "cast":
        return alv(p[0], dt) and alv(p[1], dst_dt)                               # alv(src, src_dt) && alv(dst, dst_dt)
    if op == "sqdiff_sum":
        return alv(p[0], dt) and alv(p[1], dt)                                   # alv(a, dt) && alv(b, dt)
    if op == "row_sumsq":
        return ((p[0] or 0) & 15) == 0                                           # al16(x)
    if op == "row_scale":
        return alv(p[0], dt) and alv(p[1], dt)                                   # alv(x, dt) && alv(out, dt)
    if op == "row_scale_diff":
        return alv(p[0], dt) and alv(p[1], dt) and alv(p[2], dt)                 # alv(x, dt) && alv(x2, dt) && alv(out, dt)
    if op == "tap_bwd":                                                          # alv(y) && alv(target) && alv(out) && (!g || alv(g))
        return alv(p[0], dt) and alv(p[1], dt) and alv(p[3], dt) and (not p[2] or alv(p[2], dt))
    if op in ("maxpool_fwd", "avgpool3_same"):
        return alv(p[0], dt) and alv(p[1], dt)                                   # alv(x, dt) && alv(y, dt)
    if op == "maxpool_bwd":
        return alv(p[0], dt) and alv(p[1], dt) and alv(p[2], dt)                 # alv(x, dt) && alv(gy, dt) && alv(gx, dt)
    if op == "maxpool2_bwd_act":                                                 # !(!alv(x) || !alv(gy) || !alv(gx) || (target && !alv(target)))
        return not (not alv(p[0], dt) or not alv(p[1], dt) or not alv(p[3], dt) or (bool(p[2]) and not alv(p[2], dt)))
    raise ValueError(op)


OPTIONAL = {("axpby", "y"), ("tap_bwd", "g"), ("maxpool2_bwd_act", "target")}   # operands that may be NULL


def uncapped_blocks(op, row, vec):
    """the block count of a flat map / a reduction / one row of a row map before its cap, and the cap"""
    if op in ("act_fwd", "act_bwd", "axpby", "mul", "cast"):
        return (((row + 3) // 4 if vec else row) + 255) // 256, 8192
    if op == "sqdiff_sum":
        return (row // (4 if vec else 1) + 1 + 255) // 256, 512
    if op == "row_sumsq":
        return (row + 8191) // 8192, 64
    return (row + 4095) // 4096, 512
