"""The three BatchNormalization training kernels whose arithmetic can be made exact (csrc/bn_train.hip: bn_train_apply_kernel,
bn_train_bwd_reduce_kernel, bn_train_bwd_apply_kernel), called through `lib` on edge shapes: dead lanes in the last channel
block, the scalar path (c % 4 != 0; with c = 70 over two channel blocks, the second with 6 live lanes of 64), one slice,
several slices with a ragged last one.  (cn_bn_train_coef takes a reciprocal root and has no exact form:
tests/test_bn_train_gpu.py holds it against float64.)

Exact arithmetic: x, gy, y, mean, a, b are integers of at most 9 in size, r is 1/2, the sums handed to the backward apply pass
are multiples of m and m is a power of two there, so every intermediate is a multiple of 1/4 far below 2^24 and fp32 holds it
exactly, fused or not, in any order: results are compared with the float64 statement by torch.equal.  y takes the values 0 and 6
themselves (the mask 0 < y < 6 excludes both).  Outputs hold NaN before the call; 256 guard floats on both sides stay
(tests/chan_slices_cases.py: Guarded)."""
import pytest
import torch

from tests.chan_slices_cases import BN_REDUCE_SHAPES, Guarded, to_device as _dev

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU6 = 0, 4
REDUCE_SHAPES = BN_REDUCE_SHAPES                                                      # (rows, channels)
APPLY_SHAPES = [(64, 8), (32, 6), (512, 96), (1024, 260), (16, 1280), (32, 70)]       # rows a power of two: 1 / m is exact
_id = lambda s: "x".join(map(str, s))


def _case(m, c, seed):
    g = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    return {"x": ints(-4, 4, m, c), "gy": ints(-4, 4, m, c), "y": ints(-3, 9, m, c), "mean": ints(-2, 2, c), "a": ints(-3, 3, c),
            "b": ints(-3, 3, c), "r": torch.full((c,), 0.5, dtype=torch.float64), "db": ints(-3, 3, c) * m, "dg": ints(-3, 3, c) * m}


def _g(t, act):
    return t["gy"] * ((t["y"] > 0) & (t["y"] < 6)).double() if act == ACT_RELU6 else t["gy"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU6], ids=["linear", "relu6"])
@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=_id)
def test_apply_exact(shape, act):
    from confignet_amd._lib import check, lib
    m, c = shape
    t = _case(m, c, m + c)
    x = t["x"] * 2                                   # a x + b reaches past 6 and below 0
    out = Guarded((m, c))
    d = [_dev(v) for v in (x, t["a"], t["b"])]
    check(lib.cn_bn_train_apply(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.t.data_ptr(), m, c, act, _stream()), "apply")
    want = t["a"] * x + t["b"]
    out.check(want.clamp(0, 6) if act == ACT_RELU6 else want, "apply %s act %d" % (shape, act))


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU6], ids=["linear", "relu6"])
@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=_id)
def test_backward_reduce_exact(shape, act):
    from confignet_amd._lib import check, lib
    m, c = shape
    t = _case(m, c, 3 * m + c)
    slices = lib.cn_bn_train_bwd_slices(m, c)
    assert slices >= 1 and (shape != (512, 96) or slices > 1) and (shape != (1000, 260) or slices > 1)
    part = Guarded((slices, 2 * c))
    d = {k: _dev(t[k]) for k in ("gy", "y", "x", "mean", "r")}
    check(lib.cn_bn_train_bwd_reduce(d["gy"].data_ptr(), d["y"].data_ptr() if act else None, d["x"].data_ptr(), d["mean"].data_ptr(),
                                     d["r"].data_ptr(), part.t.data_ptr(), slices, m, c, act, _stream()), "bwd_reduce")
    g = _g(t, act)
    xh = (t["x"] - t["mean"]) * t["r"]
    per = -(-m // slices)
    want = torch.stack([torch.cat([g[s * per:(s + 1) * per].sum(0), (g * xh)[s * per:(s + 1) * per].sum(0)]) for s in range(slices)])
    part.check(want, "bwd_reduce %s act %d" % (shape, act))
    assert lib.cn_bn_train_bwd_reduce(d["gy"].data_ptr(), None, d["x"].data_ptr(), d["mean"].data_ptr(), d["r"].data_ptr(),
                                      part.t.data_ptr(), slices + 1, m, c, ACT_NONE, _stream()) == -1            # a wrong slice count is refused


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU6], ids=["linear", "relu6"])
@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=_id)
def test_backward_apply_exact(shape, act):
    from confignet_amd._lib import check, lib
    m, c = shape
    t = _case(m, c, 5 * m + c)
    out = Guarded((m, c))
    d = {k: _dev(t[k]) for k in ("gy", "y", "x", "mean", "r", "a")}
    sums = _dev(torch.cat([t["db"], t["dg"]]))
    check(lib.cn_bn_train_bwd_apply(d["gy"].data_ptr(), d["y"].data_ptr() if act else None, d["x"].data_ptr(), d["mean"].data_ptr(),
                                    d["r"].data_ptr(), d["a"].data_ptr(), sums.data_ptr(), out.t.data_ptr(), m, c, act, _stream()), "bwd_apply")
    xh = (t["x"] - t["mean"]) * t["r"]
    out.check(t["a"] * (_g(t, act) - (t["db"] + xh * t["dg"]) / m), "bwd_apply %s act %d" % (shape, act))
