"""The gradient kernels of the depthwise 3x3 convolution (csrc/depthwise.hip: dwconv3x3_dgrad_kernel, dwconv3x3_wgrad_kernel) on the
smallest shapes at which each index rule can go wrong, at both strides:

  (1, 1, 1, 4)     block larger than the image; every tap but the centre is padding
  (2, 5, 7, 8)     odd extents: stride-2 pads (1, 1); a ragged last block in x and y
  (3, 8, 6, 6)     even extents: stride-2 pads (0, 1); c % 4 != 0, the scalar path
  (1, 9, 9, 32)    one wave across channel groups
  (2, 4, 4, 960)   the network's widest depthwise layer at its smallest map
  (2, 33, 17, 8)   more pixels than one filter-gradient slice: 3 slices at stride 1
  (2, 33, 33, 8)   the smallest such shape with two slices at STRIDE 2 (578 output pixels; a slice at c = 8 holds 512 -- at
                   stride 2 (2, 33, 17, 8) has 306 and stays one slice)
  (1, 5, 5, 70)    c % 4 != 0 with c > 64: the scalar path with two channel blocks, the last one with 58 dead lanes of 64

Exact arithmetic: inputs and taps are integers in [-4, 4], so every term is at most 16 in size and the longest reduction
(2 * 33 * 33 terms) stays far below 2^24: fp32 holds every sum exactly in any order, and each result is compared with the float64
statement by torch.equal.  What a call must write holds NaN before it; 256 guard floats on both sides must be unchanged
(tests/chan_slices_cases.py: Guarded; the shapes live there too, next to the recorded slice plans that cover them)."""
import functools

import numpy as np
import pytest
import torch

from tests.chan_slices_cases import DW_EDGE_SHAPES, NAN, Guarded, to_device as _dev

pytestmark = pytest.mark.gpu

SHAPES = DW_EDGE_SHAPES
_id = lambda s: "x".join(map(str, s))


def _ints(shape, seed, lo=-4, hi=4):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def _geom(e, s):
    o = -(-e // s)
    return o, ((o - 1) * s + 3 - e) // 2


def _windows(x, stride):
    """the zero-padded input and the nine strided windows of it that meet the output grid"""
    n, h, wd, c = x.shape
    (oh, ph), (ow, pw) = _geom(h, stride), _geom(wd, stride)
    xp = np.zeros((n, (oh - 1) * stride + 3, (ow - 1) * stride + 3, c))
    xp[:, ph:ph + h, pw:pw + wd] = x
    win = {(ky, kx): (slice(None), slice(ky, ky + (oh - 1) * stride + 1, stride), slice(kx, kx + (ow - 1) * stride + 1, stride))
           for ky in range(3) for kx in range(3)}
    return xp, win, (slice(None), slice(ph, ph + h), slice(pw, pw + wd))


def _statement(x, w, gy, stride):
    """float64 (y, gx, gw) of the depthwise 3x3 convolution, TF "same" padding"""
    xp, win, inner = _windows(x, stride)
    y, gxp, gw = np.zeros(gy.shape), np.zeros_like(xp), np.zeros((3, 3, x.shape[-1]))
    for (ky, kx), s in win.items():
        y += xp[s] * w[ky, kx]
        gxp[s] += gy * w[ky, kx]
        gw[ky, kx] = (gy * xp[s]).sum((0, 1, 2))
    return y, gxp[inner], gw


@functools.lru_cache(maxsize=None)
def _case(shape, stride):
    """x, w, gy and the float64 statements of y, gx, gw: drawn once per (shape, stride), never changed"""
    n, h, wd, c = shape
    oh, ow = _geom(h, stride)[0], _geom(wd, stride)[0]
    x, w, gy = _ints(shape, 11 * h + wd + c + stride), _ints((3, 3, c), c + 5), _ints((n, oh, ow, c), 3 * h + 7 * wd + c + stride)
    return (x, w, gy) + _statement(x, w, gy, stride)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_statement_is_the_forward_kernels(shape, stride):
    """the float64 statement the gradients are derived from is what cn_dwconv3x3_fwd computes"""
    from confignet_amd import ops
    x, w, gy, y, gx, gw = _case(shape, stride)
    got = ops.dwconv3x3_fwd(_dev(x), _dev(w)[..., None], None, stride)
    assert torch.equal(got.double().cpu(), torch.from_numpy(y))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_input_gradient_exact(shape, stride):
    from confignet_amd import ops
    x, w, gy, y, gx, gw = _case(shape, stride)
    out = Guarded(shape, NAN)
    ops.dwconv3x3_dgrad(_dev(gy), _dev(w)[..., None], shape, stride, out=out.t)
    out.check(gx, "dgrad %s stride %d" % (shape, stride))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_filter_gradient_exact_written_and_accumulated(shape, stride):
    from confignet_amd import ops
    x, w, gy, y, gx, gw = _case(shape, stride)
    c = shape[-1]
    out = Guarded((3, 3, c, 1), NAN)
    ops.dwconv3x3_wgrad(_dev(x), _dev(gy), stride, out=out.t, accumulate=False)
    out.check(gw, "wgrad written %s stride %d" % (shape, stride))
    held = _ints((3, 3, c, 1), c + 17, -50, 50)
    acc = Guarded((3, 3, c, 1), _dev(held))
    ops.dwconv3x3_wgrad(_dev(x), _dev(gy), stride, out=acc.t, accumulate=True)
    acc.check(held[..., 0] + gw, "wgrad accumulated %s stride %d" % (shape, stride))
    fresh = ops.dwconv3x3_wgrad(_dev(x), _dev(gy), stride)
    assert tuple(fresh.shape) == (3, 3, c, 1) and torch.equal(fresh.double().cpu().reshape(3, 3, c), torch.from_numpy(gw))


def test_the_slice_plan_splits_the_long_shapes():
    from confignet_amd._lib import lib
    assert lib.cn_dwconv3x3_wgrad_slices(2, 33, 17, 8, 1) >= 2 and lib.cn_dwconv3x3_wgrad_slices(2, 33, 33, 8, 2) >= 2
    assert lib.cn_dwconv3x3_wgrad_slices(1, 1, 1, 4, 1) == 1
    # batch 32: the 7 x 7 x 960 layer and the 128 x 128 x 32 layer want different splits
    assert lib.cn_dwconv3x3_wgrad_slices(32, 7, 7, 960, 1) == 25 and lib.cn_dwconv3x3_wgrad_slices(32, 128, 128, 32, 1) == 1024


@pytest.mark.parametrize("stride", [1, 2])
def test_filter_gradient_is_bit_identical_in_deterministic_mode_and_under_a_sink(stride):
    """float inputs, a shape with several slices: two runs give the same bits in deterministic mode, and the sum deferred to the
    join of a gradient sink gives those bits too"""
    from confignet_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 33, 33, 8), generator=g)
    gy = torch.randn((2, -(-33 // stride), -(-33 // stride), 8), generator=g)
    ops.set_deterministic(True)
    try:
        a = ops.dwconv3x3_wgrad(x.cuda(), gy.cuda(), stride)
        b = ops.dwconv3x3_wgrad(x.cuda(), gy.cuda(), stride)
        w = torch.zeros((3, 3, 8, 1), device="cuda", requires_grad=True)
        w.grad = torch.zeros_like(w)
        with ops.grad_sink([w]):
            ops.sink_dwconv3x3_wgrad(x.cuda(), gy.cuda(), stride, ops.sink_for(w))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    assert torch.equal(a, b) and torch.equal(a, w.grad)
    ref = torch.from_numpy(_statement(x.double().numpy(), np.zeros((3, 3, 8)), gy.double().numpy(), stride)[2])
    # 1089 products of unit normals per tap, summed in fp32: far inside 1e-5 of the largest entry
    assert float((a.double().cpu().reshape(3, 3, 8) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
