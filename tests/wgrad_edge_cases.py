"""Shared table and helpers of the filter-gradient edge tests (tests/test_wgrad_edge_cases_cpu.py, tests/test_wgrad_edges_gpu.py).
Plain Python: nothing here touches a device.

Every filter-gradient kernel multiplies fp32 or bf16 inputs and accumulates in fp32.  With integer inputs in [-3, 3] every product
(|.| <= 9) and every partial sum (|.| <= 9 M < 2^24 for every M of the table) is an integer that fp32 holds exactly, in ANY order of
the adds -- across K steps, MFMA blocks, row-slice slabs and atomics alike.  So the result must equal the integer reference bit
for bit, and the index logic of a kernel (gather, padding taps, tile edges, slice ends, padding workgroups) is tested with no
tolerance at all.

M = n * out_d * out_h * out_w is the length of the reduction, Ktot = taps * cin the number of filter rows."""
import ctypes

import numpy as np
import torch

from confignet_amd import ops
from confignet_amd._lib import lib
from oracle import ref_ops as O

# id -> (x shape NHWC / NDHWC, kernel, cout, stride, up, explicit pad) and the edge the geometry is there for
TABLE = {
    "A": ((3, 5, 7, 8), (3, 3), 12, 1, 0, None),           # M = 105 and Ktot = 72 fill no tile; ragged last stage
    "B": ((40, 1, 1, 16), (3, 3), 8, 1, 0, None),          # 1x1 output: every stage advance wraps the w, h and n digits; all taps but the centre are padding
    "C": ((5, 2, 3, 20), (3, 3), 36, 1, 0, None),          # M = 30 < KB: one K step, fewer than the prologue's stages
    "D": ((2, 17, 13, 48), (3, 3), 96, 2, 0, None),        # odd extents, stride-2 SAME split, cout = exactly one 96-wide tile
    "E": ((1, 37, 45, 4), (7, 7), 24, 2, 0, 3),            # explicit pad, 49 taps on 4 channels: a float4 piece is a whole tap
    "F": ((2, 3, 5, 4, 8), (3, 3, 3), 8, 1, 1, None),      # 3-D, folded upsample (>> up), M = 960
    "G": ((2, 5, 7, 16), (4, 4), 8, 1, 1, None),           # k4 + upsample, asymmetric SAME pad, Ktot = 256 = one 256 tile exactly
    "H": ((9, 16, 16, 64), (1, 1), 136, 2, 0, None),       # Ktot = 64, the wgrad2_takes boundary; cout = 128 + 8
    "I": ((3, 24, 20, 16), (3, 3), 100, 1, 0, None),       # M = 1440: 8 splits and 9 / 10 / 12 / 15 (padded XCD-ordered grid); Ktot = 144 = 128 + 16; cout no tile multiple
    "J": ((2, 6, 6, 44), (3, 3), 68, 1, 0, None),          # Ktot = 396 = 3 * 128 + 12, cout = 64 + 4
    "K": ((2, 14, 14, 8), (3, 3), 16, 1, 0, None),         # M = 392 = 6 * 64 + 8 = 3 * 128 + 8: a LAST slice of 8 rows, shorter than a stage of either depth
}

# The routing boundaries of ops.conv_wgrad / cn_conv_wgrad_ws, run on the default heuristic only: (id, geometry, profile families
# the call must show -- the kernel that takes it)
ROUTING = [
    ("H-cin60", ((9, 16, 16, 60), (1, 1), 136, 2, 0, None), {"igemm_wgrad<64x64>": 1}),      # Ktot = 60 < 64: the atomic kernel
    ("A-cin6", ((3, 5, 7, 6), (3, 3), 12, 1, 0, None), {"igemm_wgrad<128x32>": 1}),          # cin % 4 != 0: the atomic kernel, scalar gather
    ("thin", ((2, 9, 11, 8), (3, 3), 4, 1, 0, None), {}),                                    # the thin route (no profile bracket)
    ("cout4-wide", ((2, 9, 11, 72), (3, 3), 4, 1, 0, None), {"igemm_wgrad<128x32>": 1}),     # cout <= 4 but cin > 64: not thin
    ("k27", ((2, 11, 301, 3), (3, 3), 64, 2, 0, None), {"c3_wgrad": 1}),                     # the K = 27 route
    ("k27-cout68", ((2, 11, 301, 3), (3, 3), 68, 2, 0, None), {"igemm_wgrad<64x64>": 1}),    # past the K = 27 route's cout limit
]

# bf16 filter gradient (cn_conv_wgrad_bf16 takes cin % 8 == 0 and cout % 8 == 0): the table entries it takes, and two shapes whose
# own slice rule takes the XCD-ordered 1-D grid (more than one tile, >= 16 slices; bf16_planned_splits below): three 128x32 tiles
# with M = 4096 -> 16 slices of 256 rows, and with M = 6200 -> 22 slices of 288 rows in a grid padded to 24 (the last slice: 152 rows)
BF16_TABLE = ("B", "D", "F", "G", "H")
BF16_XCD = [((16, 16, 16, 32), (3, 3), 32, 1, 0, None), ((31, 10, 20, 32), (3, 3), 32, 1, 0, None)]

# The tiles of csrc/wgrad2.hip: (cn_conv_tune code, profile family, filter rows, output channels, reduction rows per stage KB)
TILES = [
    (0, "igemm_wgrad<128x128>", 128, 128, 16),
    (4, "igemm_wgrad<128x96>", 128, 96, 16),
    (2, "igemm_wgrad<64x64>", 64, 64, 32),
    (3, "igemm_wgrad<128x32>", 128, 32, 32),
    (5, "igemm_wgrad<256x64>", 256, 64, 16),
]
WANTS = (1, 3, 8, 11, 16)          # workgroup target of a forced plan = want * (tiles of the launch)
STAGES = (3, 0)                    # cn_conv_loop_select(ns): three stages, the default (four; the 128x32 tile always has three)
SPLIT_CLASSES = ("1", "2-7", "8k", ">8, not 8k")


def geom(case):
    xs, k, cout, stride, up, epad = case
    return ops.ConvSpec(k, stride=stride, up=up, explicit_pad=epad).geom(xs, cout)


def filter_shape(case):
    xs, k, cout = case[0], case[1], case[2]
    return tuple(k) + (xs[-1], cout)


def rows(g):
    """M: output positions = the length of the filter gradient's reduction"""
    return g.n * g.out_d * g.out_h * g.out_w


def ktot(g):
    return g.k_d * g.k_h * g.k_w * g.cin


def tiles_of(g, tile):
    _, _, bi, bn, _ = tile
    return -(-ktot(g) // bi) * -(-g.cout // bn)


def planned_splits(g):
    """Row slices cn_conv_wgrad_ws plans for g under the tuning in force (the workspace is one slab per slice; none = one slice)."""
    nbytes = int(lib.cn_conv_wgrad_workspace_bytes(ctypes.byref(g)))
    return max(1, nbytes // (4 * ktot(g) * g.cout))


def reported_plan(g, bf16=False):
    """What cn_conv_wgrad_plan reports for the routed call on fp32 / bf16 operands under the tuning in force: (return code, route, tile,
    row slices, rows per slice, XCD-ordered 1-D grid?).  Routes: csrc/common.h WgradRoute (3 = the LDS-DMA kernel, 5 = the bf16 one)."""
    out = (ctypes.c_longlong * 12)()
    dt = 1 if bf16 else 0
    rc = lib.cn_conv_wgrad_plan(ctypes.byref(g), dt, dt, 0, 0xFFFFFFFF, -1, out)
    return rc, out[0], out[1], out[2], out[3], out[6] == 1 and out[7] == 1 and out[2] > 1


def replayed_splits(g, tile, want):
    """The forced-target arithmetic of cn_wgrad2_plan (csrc/wgrad2.hip) by hand: s = clamp((target + tiles / 2) / tiles, 1,
    ceil(M / 4 KB)) slices asked for, rows per slice rounded up to KB, slices = ceil(M / rows)."""
    kb, m, tiles = tile[4], rows(g), tiles_of(g, tile)
    target = want * tiles
    s = 1 if tiles >= target else (target + tiles // 2) // tiles
    s = max(1, min(s, -(-m // (4 * kb))))
    r = -(-(-(-m // s)) // kb) * kb
    return -(-m // r)


def bf16_tile(g):
    """wgrad_tile_cfg (csrc/conv_geom.h): (filter rows, output channels) of the tile cn_conv_wgrad_bf16 launches"""
    if g.cout <= 32:
        return 128, 32
    if ktot(g) >= 128 and g.cout % 96 == 0 and g.cout % 128 != 0:
        return 128, 96
    if ktot(g) >= 128 and g.cout >= 128:
        return 128, 128
    return 64, 64


def bf16_planned_splits(g):
    """The bf16 kernel's slice rule (csrc/conv_dispatch.hip: bf16_wgrad_slices) by hand: (row slices, XCD-ordered 1-D grid?) -- kept as
    an independent replay of what cn_conv_wgrad_plan reports (tests/test_wgrad_edge_cases_cpu.py holds the two together).  Used for
    the number of atomic adds in the rounding bound and to show which shapes take the XCD order (more than one tile and >= 16 slices;
    the grid is then padded to a multiple of 8 slices)."""
    bm, bn = bf16_tile(g)
    m, tiles = rows(g), -(-ktot(g) // bm) * -(-g.cout // bn)
    per_cu = 3 if bm * bn >= 128 * 128 else 4 if bm * bn >= 128 * 96 else 5
    target = 256 * per_cu * (1 if bn >= 96 else 2)
    s = min(target // tiles, m // 512)
    s = max(s, min(m // 256, -(-256 // tiles)))
    if s >= 16:
        s &= ~7
    s = max(s, 1)
    r = -(-m // s)
    if r < 256:
        r = min(256, -(-m // 32) * 32)
    r = -(-r // 32) * 32
    s = -(-m // r)
    return s, tiles > 1 and s >= 16


def split_class(splits):
    if splits == 1:
        return SPLIT_CLASSES[0]
    if splits < 8:
        return SPLIT_CLASSES[1]
    return SPLIT_CLASSES[2] if splits % 8 == 0 else SPLIT_CLASSES[3]


def forced_plan(case):
    """{(tile code, want): row slices} with the tile and a workgroup target of want * tiles forced through cn_conv_tune.  Leaves
    the LAST tuning in force: the caller restores cn_conv_tune(-1, 0, 0)."""
    g = geom(case)
    out = {}
    for tile in TILES:
        for want in WANTS:
            ops.check(lib.cn_conv_tune(tile[0], 0, want * tiles_of(g, tile)), "cn_conv_tune")
            out[(tile[0], want)] = planned_splits(g)
    return out


def integer_inputs(case, seed):
    """x and the output gradient, integers drawn uniformly from [-3, 3], as float64 CPU tensors"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=case[0]).astype(np.float64)
    gy = rng.integers(-3, 4, size=ops.geom_out_shape(geom(case))).astype(np.float64)
    return torch.from_numpy(x), torch.from_numpy(gy)


def reference(x, gy, case, dtype=torch.float64):
    """The filter gradient of the table entry `case` through torch autograd on the CPU, in `dtype` (the reference: float64)."""
    xs, k, cout, stride, up, epad = case
    xr = x.to(dtype)
    w = torch.zeros(tuple(k) + (xs[-1], cout), dtype=dtype, requires_grad=True)       # (linear in w: the gradient does not depend on it)
    xu = O.upsample2(xr) if up else xr
    y = O.conv_valid_padded(xu, w, None, stride, epad) if epad is not None else O.conv_same(xu, w, None, stride=stride)
    assert tuple(y.shape) == tuple(gy.shape), (tuple(y.shape), tuple(gy.shape))
    (y * gy.to(dtype)).sum().backward()
    return w.grad.detach()
