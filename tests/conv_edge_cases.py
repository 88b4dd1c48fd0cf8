"""Shared table and helpers of the forward / data-gradient edge tests (tests/test_conv_edge_cases_cpu.py, tests/test_conv_edges_gpu.py).
Plain Python: nothing here touches a device.

Every forward / data-gradient kernel multiplies fp32 values (the bf16 kernels: bf16 values, whose products fp32 holds exactly) and
accumulates in fp32.  With integer x, w, bias, res and gy in [-3, 3] and A = conv(|x|, |w|) + |bias| + |res| < 2^24 elementwise,
every partial sum is an integer fp32 holds exactly in ANY order of the adds -- across K steps, across K slices joined by atomics and
in the deterministic slab sum.  So the result must equal the float64 reference bit for bit, and the index logic of a kernel (gather,
padding taps, tile edges, slice ends, parity classes) is tested with no tolerance at all.  ReLU and LeakyReLU with slope 0.25 (a
power of two) keep that: tanh stays with its tolerance test.

M = n * out_d * out_h * out_w is the number of output rows, K = taps * cin the length of the reduction."""
import ctypes
import functools

import numpy as np
import torch

from confignet_amd import ops
from confignet_amd._lib import lib
from oracle import ref_ops as O
from tests import test_conv_plan_cpu as P
from tests.test_conv_plan_cpu import REQUESTS

SLOPE = 0.25
(UP2K4_RGB, S2_IMAGE_DGRAD, S1_IMAGE_DGRAD, THIN_PAR_IGEMM, THIN_COOP, THIN, C3, C7S2, FWD2, IGEMM, UNSUPPORTED) = range(11)
LAUNCHING_ROUTES = tuple(range(10))
ROUTE_NAMES = ["UP2K4_RGB", "S2_IMAGE_DGRAD", "S1_IMAGE_DGRAD", "THIN_PAR_IGEMM", "THIN_COOP", "THIN", "C3", "C7S2", "FWD2", "IGEMM", "UNSUPPORTED"]
FORWARD = ("fwd", "res", "stats", "fwd_dt")
DGRAD = ("dgrad", "dgrad_w", "dgrad_w_res", "dgrad_dt")

# id -> (x shape NHWC / NDHWC, kernel, cout, stride, up, explicit pad) and the edge the geometry is there for
TABLE = {
    "a": ((3, 5, 7, 48), (3, 3), 52, 1, 0, None),            # M = 105 and cout = 52 fill no tile; data gradient: cin 52, scalar gather
    "b": ((40, 1, 1, 64), (3, 3), 48, 1, 0, None),           # 1x1 output: all taps but the centre are padding, M = 40 < 64
    "c": ((2, 17, 13, 48), (3, 3), 96, 2, 0, None),          # odd extents under stride 2: the other SAME split, data gradient not parity-ordered
    "d": ((2, 16, 12, 48), (3, 3), 96, 2, 0, None),          # even extents: parity classes of 1 / 2 / 2 / 4 taps
    "e7": ((1, 37, 45, 3), (7, 7), 24, 2, 0, 3),             # the 7x7 image kernel, ragged 8x32 tiles
    "e3s1": ((2, 9, 11, 3), (3, 3), 64, 1, 0, None),         # image layer, stride 1
    "e3s2": ((2, 9, 11, 3), (3, 3), 48, 2, 0, None),         # image layer, stride 2, odd extents
    "e3s2even": ((2, 10, 12, 3), (3, 3), 48, 2, 0, None),    # image layer, stride 2, even extents
    "f": ((2, 3, 5, 4, 48), (3, 3, 3), 64, 1, 1, None),      # 3-D with folded upsample
    "g": ((2, 5, 7, 64), (4, 4), 48, 1, 1, None),            # k4 with upsample, asymmetric pad
    "h": ((9, 16, 16, 64), (1, 1), 136, 2, 0, None),         # 1x1 stride 2, cout = 128 + 8
    "h144": ((9, 16, 16, 64), (1, 1), 144, 2, 0, None),      # data gradient: one live parity class with T = 1, tiles with no K step
    "i36": ((2, 9, 7, 64), (1, 1), 36, 1, 0, None),          # plain 1x1 below g_fwd2_min_c
    "i52": ((2, 9, 7, 64), (1, 1), 52, 1, 0, None),          # plain 1x1 product of the LDS-DMA loop
    "i16": ((2, 9, 7, 16), (1, 1), 52, 1, 0, None),          # one K step: not above g_fwd2_min_nks
    "j24": ((1, 11, 9, 24), (3, 3), 64, 1, 0, None),         # cin is no multiple of 16
    "j6": ((3, 5, 7, 6), (3, 3), 12, 1, 0, None),            # cin is no multiple of 4: the data gradient is refused
    "k1": ((2, 9, 11, 8), (3, 3), 1, 1, 0, None),            # thin output
    "k3": ((1, 9, 11, 32), (3, 3), 3, 1, 0, None),           # thin output, cooperative kernel
    "kpar": ((2, 8, 12, 4), (3, 3), 32, 2, 0, None),         # data gradient with cout 4 and parity order
    "p16": ((2, 8, 12, 16), (3, 3), 32, 2, 0, None),         # data gradient: parity order on the register-staged loop (cout 16)
    "p32": ((2, 8, 12, 32), (3, 3), 32, 2, 0, None),         # data gradient: parity order on the 128x32 tile of the LDS-DMA loop
    "up2k4": ((1, 20, 13, 32), (4, 4), 3, 1, 1, None),       # map_final on ragged 8x16 tiles
    "l32": ((2, 7, 9, 32), (3, 3), 32, 1, 0, None),          # the 128x32 tile of the LDS-DMA loop
    "m": ((1, 4, 4, 512), (3, 3), 64, 1, 0, None),           # M = 16
    "n96": ((2, 8, 8, 96), (3, 3), 96, 1, 0, None),          # cout = 96: residual epilogues on a 96-wide launch
    "n192": ((2, 16, 16, 96), (3, 3), 192, 2, 0, None),      # M = 128: a fused request drops the split
    "s128": ((3, 8, 16, 48), (3, 3), 96, 1, 0, None),        # 128 rows a sample: the 128-row tiles can carry the statistics
}
STATS_NAMES = ("h", "h144", "n96", "n192", "s128")           # entries whose forward launch carries cn_conv_fwd_stats

# Winograd F(2x2, 3x3) -- exact with filters that are integer multiples of 4 -- and F(4x4, 3x3) at its tolerance: (x shape, cout)
WINO_SHAPES = [((2, 9, 7, 16), 64), ((1, 5, 6, 16), 128), ((1, 1, 1, 16), 64), ((1, 17, 33, 32), 64)]
WINO4_SHAPES = [((1, 16, 32, 16), 64), ((2, 32, 64, 64), 64)]

FORCED_CFGS = (0, 1, 2, 3, 4)
FORCED_SPLITS = (1, 3, 8, 16)
TILE_OF = {0: (128, 128), 1: (128, 64), 2: (64, 64), 3: (128, 32), 4: (128, 96)}


def geom(case):
    xs, k, cout, stride, up, epad = case
    return ops.ConvSpec(k, stride=stride, up=up, explicit_pad=epad).geom(xs, cout)


def filter_shape(case):
    xs, k, cout = case[0], case[1], case[2]
    return tuple(k) + (xs[-1], cout)


def rows(g):
    return g.n * g.out_d * g.out_h * g.out_w


def ktot(g):
    return g.k_d * g.k_h * g.k_w * g.cin


def request_geom(case, request):
    """the geometry the request plans with (the data-gradient one for the dgrad requests), None where the call refuses before planning"""
    return P.request_geom(geom(case), request)


def plan_of(case, request):
    """(return code, route, tile, K slices, parity order, profile family) of cn_conv_fwd_plan under the tuning in force; None where
    the call refuses the layer before it plans (every such refusal is CN_EUNSUPPORTED)"""
    got = P.plan_request(geom(case), request)
    return None if got is None else (got[0],) + tuple(got[1][:5])


def split_class(splits):
    return "1" if splits == 1 else "2-7" if splits < 8 else "8-15" if splits < 16 else "16"


def gemm_entries(request="fwd"):
    """the table entries whose default plan for `request` is one of the two implicit-GEMM routes (the ones cn_conv_tune configures)"""
    out = []
    for name, case in TABLE.items():
        p = plan_of(case, request)
        if p is not None and p[0] == 0 and p[1] in (FWD2, IGEMM):
            out.append(name)
    return out


def _seed(case):
    return 7 + sum(case[0]) * 31 + case[2] * 17 + case[3] * 5 + case[4]


def _draw(rng, shape, lim, real):
    if real:
        return torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32).astype(np.float64))
    return torch.from_numpy(rng.integers(-lim, lim + 1, size=shape).astype(np.float64))


def integer_inputs(case, seed=None, lim=3, real=False):
    """x, w, bias, res (shaped like y), gy (shaped like y) and resx (shaped like the upsampled x): integers drawn uniformly from
    [-lim, lim] (real = True: standard-normal fp32 values, for the rounding pass), as float64 CPU tensors"""
    g = geom(case)
    rng = np.random.default_rng(_seed(case) if seed is None else seed)
    ys = ops.geom_out_shape(g)
    return {"x": _draw(rng, case[0], lim, real), "w": _draw(rng, filter_shape(case), lim, real), "bias": _draw(rng, (g.cout,), lim, real),
            "res": _draw(rng, ys, lim, real), "gy": _draw(rng, ys, lim, real), "resx": _draw(rng, ops.geom_in_shape(g, upsampled=True), lim, real)}


def _conv(case, x, w, b):
    _, _, _, stride, up, epad = case
    xu = O.upsample2(x) if up else x
    return O.conv_valid_padded(xu, w, b, stride, epad) if epad is not None else O.conv_same(xu, w, b, stride=stride)


def _act(v, act):
    if act == P.ACT_LRELU:
        return torch.where(v > 0, v, SLOPE * v)
    return torch.relu(v) if act == P.ACT_RELU else v


def _dgrad(case, gy, w):
    """gradient of sum(conv(xu, w) * gy) with respect to the (upsampled) input xu, through autograd"""
    _, _, _, stride, up, epad = case
    g = geom(case)
    xu = torch.zeros(ops.geom_in_shape(g, upsampled=True), dtype=w.dtype, requires_grad=True)      # (linear in xu: any value does)
    y = O.conv_valid_padded(xu, w, None, stride, epad) if epad is not None else O.conv_same(xu, w, None, stride=stride)
    assert tuple(y.shape) == tuple(gy.shape), (tuple(y.shape), tuple(gy.shape))
    (y * gy).sum().backward()
    return xu.grad.detach()


def reference(case, request, inputs=None, dtype=torch.float64, absolute=False):
    """What the call of `request` (tests/test_conv_plan_cpu.py: REQUESTS) must give on the table entry, in `dtype` on the CPU (the
    reference: float64).  Forward requests: act(conv(x, w) + bias [+ res]), LeakyReLU with slope 0.25 / ReLU as REQUESTS says; data
    gradients: with respect to the (upsampled) input [+ resx].  absolute = True: the same sum over absolute values without the
    activation -- the A of the exactness precondition and of the rounding bound."""
    q = REQUESTS[request]
    i = {k: (v.abs() if absolute else v).to(dtype) for k, v in (inputs or integer_inputs(case)).items()}
    if q[0]:
        out = _dgrad(case, i["gy"], i["w"])
        return out + i["resx"] if q[4] else out
    out = _conv(case, i["x"], i["w"], i["bias"] if q[2] else None)
    if q[4]:
        out = out + i["res"]
    return out if absolute else _act(out, q[3])


def exact_bound(case, request="res", inputs=None):
    """A = conv(|x|, |w|) + |bias| + |res| elementwise (the data-gradient requests: the same of |gy|, |w| and |resx|): every partial
    sum of every kernel is an integer of at most that size"""
    return reference(case, request, inputs, absolute=True)


def stats_reference(v, mode, n):
    """cn_conv_fwd_stats: mode 1 = [sum a, sum a^2] of the stored values, mode 2 = [sum v, sum v^2, sum l, sum l^2] with
    l = leaky_relu(v, 0.25) of the pre-activation values, per (sample, channel); v: the stored / pre-activation output in float64"""
    v = v.reshape(n, -1, v.shape[-1])
    if mode == 1:
        return torch.stack([v.sum(1), (v * v).sum(1)])
    l = torch.where(v > 0, v, SLOPE * v)
    return torch.stack([v.sum(1), (v * v).sum(1), l.sum(1), (l * l).sum(1)])


def stats_bounds(v, mode, n):
    """largest float64 sum of absolute values behind an entry of (the integer sums, the sums in units of 1/16): exact in fp32 while
    they stay below 2^24 and 2^20"""
    v = v.abs().reshape(n, -1, v.shape[-1])
    whole, sixteenth = max(float(v.sum(1).max()), float((v * v).sum(1).max())), 0.0
    if mode == 1:
        sixteenth = whole          # (a = l: the activated values are multiples of 1/4, their squares of 1/16)
    else:
        sixteenth = float((v * v).sum(1).max())
    return whole, sixteenth


@functools.lru_cache(maxsize=None)
def stats_inputs(name, mode):
    """integer inputs of the statistics test: [-3, 3] where every sum stays exact, else [-1, 1]"""
    case = TABLE[name]
    for lim in (3, 1):
        inp = integer_inputs(case, lim=lim)
        pre = _conv(case, inp["x"], inp["w"], inp["bias"])
        whole, sixteenth = stats_bounds(pre, mode, case[0][0])
        if whole < 2 ** 24 and sixteenth < 2 ** 20:
            break
    return inp


def rounding_bound(A, k, s):
    """|got - ref| <= 2 (K + S + 2) 2^-24 A: fp32 accumulation of K products and S slice adds in any order, two more adds for bias and
    residual, the factor 2 for truncating intermediate rounding inside the MFMA (as in tests/test_wgrad_edges_gpu.py)"""
    return 2.0 * (k + s + 2) * 2.0 ** -24 * A


# ---- the bf16 forward's own tile rule (csrc/igemm_bf16.hip: conv_bf16 picks by launch size alone and ignores cn_conv_tune) -------
def bf16_tile(g):
    """the tile conv_bf16 launches for the geometry g (the data gradient: its dgrad_geom): 0 = 128x128, 1 = 128x64, 2 = 64x64,
    3 = 128x32, 4 = 128x96.  A hand-kept replay of the rule in csrc/igemm_bf16.hip (conv_bf16, which carries a comment pointing
    here): the library reports no plan for the bf16 calls, so a change to that rule has to be made here as well."""
    m = rows(g)
    c128 = -(-m // 128)
    t128, t128x64 = c128 * -(-g.cout // 128), c128 * -(-g.cout // 64)
    if g.cout <= 32:
        cfg = 3
    elif g.cout > 64 and t128 >= 512:
        cfg = 0
    elif t128x64 >= 512:
        cfg = 1
    else:
        cfg = 2
    if g.cout % 96 == 0 and g.cout % 128 != 0 and c128 * (g.cout // 96) >= 256:
        cfg = 4
    return cfg


# 1x1 layers on M = 2 * 63 * 65 = 8190 rows (64 tiles of 128 rows, the last ragged), one per tile arm the table does not reach, and
# one whose cin is no multiple of 32 (the register-staged kernel instead of the LDS-DMA loop)
BF16_EXTRA = {
    "t128x128": ((2, 63, 65, 32), (1, 1), 1032, 1, 0, None),      # 64 x 9 = 576 tiles of 128 x 128, columns ragged
    "t128x64": ((2, 63, 65, 32), (1, 1), 584, 1, 0, None),        # 64 x 5 = 320 < 512 tiles of 128 x 128, 64 x 10 = 640 of 128 x 64
    "t128x96": ((2, 63, 65, 32), (1, 1), 480, 1, 0, None),        # 64 x 5 = 320 >= 256 tiles of 128 x 96
    "t128x128-cin40": ((2, 63, 65, 40), (1, 1), 1032, 1, 0, None),
}
BF16_TABLE = tuple(n for n, c in TABLE.items() if c[0][-1] % 8 == 0 and c[2] % 8 == 0)


def tune(cfg, splits):
    ops.check(lib.cn_conv_tune(cfg, splits, 0), "cn_conv_tune")


def byref(g):
    return ctypes.byref(g)
