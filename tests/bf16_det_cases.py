"""Shared inputs and the fp32 emulation of the deterministic bf16 filter gradient's tests (tests/test_bf16_det_plan_cpu.py,
tests/test_bf16_det_wgrad_gpu.py).  Plain Python: nothing here touches a device.

In deterministic mode the bf16 filter gradient (csrc/igemm_bf16.hip) writes one slab per row slice and cn_sum_parts adds the slabs in
slice order.  Integer inputs cannot tell that order from any other -- every sum is exact.  The ORDER-SENSITIVE inputs can: x holds
integers in [-3, 3] and row m of gy holds integers in [-3, 3] times 2^e with e = E[m // rows], one exponent per slice.  Every value
is exact in bf16 (|k| <= 3 needs two mantissa bits), every product is k 2^e with |k| <= 9, and a slice of at most 288 rows sums to a
multiple of 2^e below 9 * 288 * 2^e < 2^12 * 2^e: exact in fp32 in any order of the adds inside the slice.  The only rounding left is
in the adds ACROSS slices, whose exponents spread over 24 binades, so the bits of the result are a function of the order of those
adds alone -- and the expected bits are the float64 slice partials (exact in fp32) added in fp32 the way cn_sum_parts adds fewer than
64 parts: t = 0; t += p_0; ... t += p_(S-1); then one more fp32 add onto the target."""
import ctypes

import torch

from confignet_amd._lib import CN_BF16, lib
from tests import wgrad_edge_cases as W

# one exponent per slice (22 = the most slices of W.BF16_XCD): neighbours far apart, so that no order of the adds is harmless
E = [0, 8, 16, 24, 4, 12, 20, 2, 10, 18, 6, 14, 22, 1, 9, 17, 3, 11, 19, 5, 13, 21]
BF16_ROUTE, SUM_PARTS = 5, 1      # csrc/common.h: CN_WG_BF16; csrc/conv_dispatch.hip: WG_SUM_PARTS


def bf16_plan(g, det):
    """cn_conv_wgrad_plan of the routed call on bf16 operands: (return code, the 12 plan fields)"""
    out = (ctypes.c_longlong * 12)()
    rc = lib.cn_conv_wgrad_plan(ctypes.byref(g), CN_BF16, CN_BF16, 0, 0xFFFFFFFF, det, out)
    return rc, list(out)


def rows_and_slices(case):
    rc, p = bf16_plan(W.geom(case), 1)
    assert rc == 0 and p[0] == BF16_ROUTE, (rc, p)
    return int(p[3]), int(p[2])


def order_inputs(case, seed=41):
    """(x, gy) as float64 CPU tensors: integers in [-3, 3], row m of gy scaled by 2^E[m // rows]"""
    g = W.geom(case)
    rows, slices = rows_and_slices(case)
    assert 1 < slices <= len(E) and rows <= 288
    x, gy = W.integer_inputs(case, seed)
    scale = torch.tensor([2.0 ** E[m // rows] for m in range(W.rows(g))], dtype=torch.float64)
    gy = (gy.reshape(-1, g.cout) * scale[:, None]).reshape(gy.shape)
    assert torch.equal(gy.to(torch.bfloat16).double(), gy) and torch.equal(x.to(torch.bfloat16).double(), x)
    return x, gy


def slice_partials(x, gy, case):
    """The float64 filter gradient of every row slice alone (gy zero outside the slice), each exact in fp32"""
    g = W.geom(case)
    rows, slices = rows_and_slices(case)
    flat = gy.reshape(-1, g.cout)
    parts = []
    for s in range(slices):
        only = torch.zeros_like(flat)
        only[s * rows:(s + 1) * rows] = flat[s * rows:(s + 1) * rows]
        p = W.reference(x, only.reshape(gy.shape), case)
        assert torch.equal(p.float().double(), p)
        parts.append(p)
    return parts


def emulate(parts, order, prior=None):
    """cn_sum_parts on fewer than 64 parts, in fp32: t = 0, t += part for the parts in `order`, then target + t (the target: zeros
    after the zero pass of a write, else the fp32 tensor `prior`)"""
    assert len(parts) < 64
    t = torch.zeros(parts[0].shape, dtype=torch.float32)
    for s in order:
        t = t + parts[s].float()
    return (torch.zeros_like(t) if prior is None else prior.float().cpu()) + t


def fraction_different(a, b):
    return float((a != b).double().mean())


def order_prior(shape, seed=43):
    """An fp32 target for the accumulate mode whose add rounds too: standard-normal values times 2^20"""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 2.0 ** 20).float()


def sweep():
    """(taps, cin, cout, M) of the workspace bound: 1 .. 64 taps, 8 .. 2048 channels, 2^8 .. 2^22 rows"""
    chans = (8, 16, 24, 32, 48, 64, 96, 128, 136, 192, 256, 512, 1024, 2048)
    ms = sorted({1 << k for k in range(8, 23)} | {3 << k for k in range(8, 21)} | {6200, 1440, 100000, 1000001})
    for taps in range(1, 65):
        for cin in chans:
            for cout in chans:
                for m in ms:
                    yield taps, cin, cout, m


class SweepGeom:
    """What W.bf16_planned_splits and W.bf16_tile read of a geometry: a 1 x taps filter over M = n output positions"""
    out_d = out_h = out_w = k_d = k_h = 1

    def __init__(self, taps, cin, cout, m):
        self.n, self.k_w, self.cin, self.cout = m, taps, cin, cout

