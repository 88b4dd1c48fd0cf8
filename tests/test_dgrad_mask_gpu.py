"""The data gradient with the ReLU backward of the layer in front in its epilogue, through the C ABI: cn_conv_dgrad_w_mask (csrc/fwd2.hip:
fwd2_mask_kernel -- the plain 1x1 product and the gathered form) and cn_conv_fwd_wino_ep (csrc/winograd.hip: wino_fwd_kernel<true>).

Exact cases by the method of tests/conv_edge_cases.py: integer inputs in [-3, 3], every product, partial sum and column sum an integer
below 2^24 (asserted), so the results equal the float64 reference exactly in any order of the adds.  The masks hold positive and
negative values, 0.0 and -0.0.  Per case:
  * gu has the bits of the unfused pair on the same build (cn_conv_dgrad_w / _res, or cn_conv_fwd_wino with the data-gradient filter,
    followed by cn_act_bwd);
  * gu equals the float64 reference (transposed convolution on the CPU, then the mask);
  * colsum and colsum2 equal the float64 column sums;
  * a launch with colsum = NULL gives the same gu;
  * destinations that held non-zero values are added to, not overwritten.
Outputs and sum destinations are views into sentinel-guarded allocations.  The refusals leave everything untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_edge_cases as C
from tests.test_conv_edges_gpu import GuardedOut, _call

from confignet_amd._lib import CN_EUNSUPPORTED, CN_F32

ACT_NONE, ACT_RELU = 0, 2
FWD2, UNSUPPORTED = 8, 10

# id -> (x shape, kernel, cout, stride, up, explicit pad) of the FORWARD convolution whose data gradient is taken: the launch's rows
# are the pixels of x, its reduction runs over cout (x taps), its columns are the channels of x
FWD2_CASES = {
    "p25": ((1, 5, 5, 64), (1, 1), 64, 1, 0, None),          # M = 25: one tile, rows past M
    "p162": ((2, 9, 9, 128), (1, 1), 128, 1, 0, None),       # M = 162: the last tile partial; two column tiles
    "p162n80": ((2, 9, 9, 80), (1, 1), 128, 1, 0, None),     # 80 columns: the column guard (a multiple of 4, not of 64)
    "g36": ((1, 6, 6, 32), (3, 3), 64, 1, 0, None),          # gathered 3x3 into 32 channels (F(2x2) declines: 32 % 64): the 128 x 32 tile
}
# (n, h, w, reduction channels, output channels) of the F(2x2) launch = the data gradient of a 3x3 convolution of `cout` channels into `cin`
WINO_CASES = {
    "w6": (1, 6, 6, 16, 64),                                  # two K steps; one 8 x 8-tile block, partly filled
    "w17": (2, 17, 17, 32, 128),                              # odd extent: the ox + 1 < w / oy + ph < h guards, four blocks an image
}


def _mask_like(shape, seed):
    """the saved activation: integers in [-2, 2] (zeros among them) with -0.0 on every seventh element"""
    rng = np.random.default_rng(seed)
    m = torch.from_numpy(rng.integers(-2, 3, size=shape).astype(np.float32))
    flat = m.view(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    assert bool((flat > 0).any()) and bool((flat < 0).any())
    assert bool(((flat == 0) & torch.signbit(flat)).any()) and bool(((flat == 0) & ~torch.signbit(flat)).any())
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _fwd2_inputs(name):
    from confignet_amd import ops
    case = FWD2_CASES[name]
    host = C.integer_inputs(case)
    host["mask"] = _mask_like(ops.geom_in_shape(C.geom(case), upsampled=True), 11 + len(name)).double()
    bound = C.exact_bound(case, "dgrad_w_res", host)
    assert float(bound.reshape(-1, bound.shape[-1]).sum(0).max()) + 1000 * 5 < 2 ** 24        # (+ the destinations' previous content)
    dev = {k: v.float().cuda() for k, v in host.items()}
    # .float() of the mask would keep -0.0; make sure of it
    assert bool(((dev["mask"] == 0) & torch.signbit(dev["mask"])).any())
    torch.cuda.synchronize()
    return host, dev


@functools.lru_cache(maxsize=None)
def _fwd2_ref(name, with_res):
    """float64 on the CPU, computed once: (gu, column sums)"""
    host = _fwd2_inputs(name)[0]
    gu = C.reference(FWD2_CASES[name], "dgrad_w_res" if with_res else "dgrad_w", host)
    gu = gu * (host["mask"] > 0)
    return gu, gu.reshape(-1, gu.shape[-1]).sum(0)


def _mask_call(case, d, out, res, colsum, colsum2):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    g, p = C.geom(case), ops._ptr
    return lib.cn_conv_dgrad_w_mask(ctypes.byref(g), p(d["gy"]), p(d["w"]), p(d["resx"]) if res else None, p(d["mask"]), p(out),
                                    p(colsum), p(colsum2), ops._stream())


def _act_bwd(gu, mask):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    out = torch.empty_like(gu)
    ops.check(lib.cn_act_bwd(ops._ptr(gu), ops._ptr(mask), ops._ptr(out), gu.numel(), ACT_RELU, 0.0, CN_F32, ops._stream()), "cn_act_bwd")
    return out


def _check_sums(dst, base, want, what):
    assert dst.intact(), what + ": a guard of a sum destination was written"
    got = dst.out.cpu().double() - base
    assert torch.equal(got, want), what + ": column sums differ at %s" % (torch.nonzero(got != want).view(-1)[:8].tolist(),)


@pytest.fixture(autouse=True)
def _defaults():
    """the built-in plan, and the default mode whatever the suite runs in (deterministic mode refuses the sums: its own test below)"""
    from confignet_amd import ops
    was = ops.DETERMINISTIC
    ops.set_deterministic(False)
    C.tune(-1, 0)
    yield
    ops.set_deterministic(was)
    C.tune(-1, 0)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("name", list(FWD2_CASES))
def test_the_lds_dma_launch_with_the_mask_epilogue(name, with_res):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = FWD2_CASES[name]
    host, d = _fwd2_inputs(name)
    request = "dgrad_w_res" if with_res else "dgrad_w"
    gq = C.request_geom(case, request)
    out8 = (ctypes.c_int * 8)()
    rc = lib.cn_conv_fwd_plan_ep(ctypes.byref(gq), 1, 0, ACT_NONE, int(with_res), 0, 1, CN_F32, CN_F32, ctypes.byref(out8))
    what = "%s res=%d plan %s" % (name, with_res, list(out8))
    assert rc == 0 and out8[0] == FWD2 and out8[2] == 1, what
    assert out8[1] == (3 if name == "g36" else 2), what
    assert C.rows(gq) == {"p25": 25, "p162": 162, "p162n80": 162, "g36": 36}[name] and gq.cout == {"p162": 128, "p162n80": 80, "g36": 32}.get(name, 64)
    shape = ops.geom_in_shape(C.geom(case), upsampled=True)
    ref_gu, ref_sums = _fwd2_ref(name, with_res)
    # the unfused pair
    y0 = GuardedOut(shape)
    assert _call(case, request, d, y0.out) == 0, what + ": " + lib.cn_last_error_string().decode()
    pair = _act_bwd(y0.out, d["mask"])
    # fused, sums into zeroed destinations
    y, s1, s2 = GuardedOut(shape), GuardedOut((gq.cout,)), GuardedOut((gq.cout,))
    s1.out.zero_()
    s2.out.zero_()
    assert _mask_call(case, d, y.out, with_res, s1.out, s2.out) == 0, what + ": " + lib.cn_last_error_string().decode()
    torch.cuda.synchronize()
    assert y.intact(), what + ": a guard was written"
    assert torch.equal(_bits(y.out), _bits(pair)), what + ": not the bits of the unfused pair"
    assert torch.equal(y.out.cpu().double(), ref_gu), what + ": not the float64 reference"
    _check_sums(s1, 0.0, ref_sums, what + " colsum")
    _check_sums(s2, 0.0, ref_sums, what + " colsum2")
    # without sums: the same gu
    yn = GuardedOut(shape)
    assert _mask_call(case, d, yn.out, with_res, None, None) == 0, what
    # one destination only, holding values: added to
    base = torch.arange(gq.cout, dtype=torch.float32) % 5 - 2
    s3 = GuardedOut((gq.cout,))
    s3.out.copy_(base.cuda())
    y3 = GuardedOut(shape)
    assert _mask_call(case, d, y3.out, with_res, None, s3.out) == 0, what
    torch.cuda.synchronize()
    assert yn.intact() and y3.intact()
    assert torch.equal(_bits(yn.out), _bits(y.out)) and torch.equal(_bits(y3.out), _bits(y.out)), what + ": gu depends on the sum destinations"
    _check_sums(s3, base.double(), ref_sums, what + " colsum2 alone, added to")


@functools.lru_cache(maxsize=None)
def _wino_inputs(name):
    n, h, w, cin, cout = WINO_CASES[name]
    rng = np.random.default_rng(5 + h)
    host = {"gy": torch.from_numpy(rng.integers(-3, 4, size=(n, h, w, cin)).astype(np.float64)),
            # the forward filter [3][3][cout][cin] of the convolution whose data gradient this is; even integers: the filter
            # transform's halves and quarters stay integers or dyadic fractions that fp32 holds exactly
            "w": torch.from_numpy((4 * rng.integers(-1, 2, size=(3, 3, cout, cin))).astype(np.float64)),
            "mask": _mask_like((n, h, w, cout), 3 + h).double()}
    # float64 reference: the data gradient = the transposed convolution
    gy = host["gy"].permute(0, 3, 1, 2)
    wt = host["w"].permute(3, 2, 0, 1)                         # conv_transpose2d: (in = cin of this launch, out, kh, kw)
    gu = torch.nn.functional.conv_transpose2d(gy, wt, padding=1).permute(0, 2, 3, 1).contiguous()
    bound = torch.nn.functional.conv_transpose2d(gy.abs(), wt.abs(), padding=1)
    # every intermediate of F(2x2) (input differences of up to 4 |gy|, filter sums of up to 9/4 |w|): a generous factor 16 on the
    # element's bound; the column sums are sums of finished elements (+ the destinations' previous content)
    assert 16 * float(bound.max()) < 2 ** 24
    assert float(bound.permute(0, 2, 3, 1).reshape(-1, cout).sum(0).max()) + 5000 < 2 ** 24
    gu = gu * (host["mask"] > 0)
    host["ref"], host["ref_sums"] = gu, gu.reshape(-1, cout).sum(0)
    dev = {k: host[k].float().cuda() for k in ("gy", "w", "mask")}
    torch.cuda.synchronize()
    return host, dev


@pytest.mark.parametrize("name", list(WINO_CASES))
def test_the_winograd_launch_with_the_mask_epilogue(name):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, h, w, cin, cout = WINO_CASES[name]
    host, d = _wino_inputs(name)
    p, s = ops._ptr, ops._stream()
    u = torch.empty((16, cin, cout), device="cuda", dtype=torch.float32)
    # cn_conv_wino_filter(dgrad = 1) takes the forward filter [3][3][its cin = cout here][its cout = cin here]
    ops.check(lib.cn_conv_wino_filter(p(d["w"]), p(u), cout, cin, 1, s), "cn_conv_wino_filter")
    shape, what = (n, h, w, cout), name

    def fused(out, c1, c2):
        return lib.cn_conv_fwd_wino_ep(n, h, w, cin, cout, p(d["gy"]), p(u), p(out), p(d["mask"]), p(c1), p(c2), s)

    y0 = GuardedOut(shape)
    assert lib.cn_conv_fwd_wino(n, h, w, cin, cout, p(d["gy"]), p(u), None, p(y0.out), ACT_NONE, 0.0, s) == 0, lib.cn_last_error_string().decode()
    pair = _act_bwd(y0.out, d["mask"])
    y, s1, s2 = GuardedOut(shape), GuardedOut((cout,)), GuardedOut((cout,))
    s1.out.zero_()
    s2.out.zero_()
    assert fused(y.out, s1.out, s2.out) == 0, lib.cn_last_error_string().decode()
    torch.cuda.synchronize()
    assert y0.intact() and y.intact(), what + ": a guard was written"
    assert torch.equal(_bits(y.out), _bits(pair)), what + ": not the bits of the unfused pair"
    assert torch.equal(y.out.cpu().double(), host["ref"]), what + ": not the float64 reference"
    _check_sums(s1, 0.0, host["ref_sums"], what + " colsum")
    _check_sums(s2, 0.0, host["ref_sums"], what + " colsum2")
    yn, y3, s3 = GuardedOut(shape), GuardedOut(shape), GuardedOut((cout,))
    base = torch.arange(cout, dtype=torch.float32) % 5 - 2
    s3.out.copy_(base.cuda())
    assert fused(yn.out, None, None) == 0 and fused(y3.out, s3.out, None) == 0
    torch.cuda.synchronize()
    assert yn.intact() and y3.intact()
    assert torch.equal(_bits(yn.out), _bits(y.out)) and torch.equal(_bits(y3.out), _bits(y.out)), what + ": gu depends on the sum destinations"
    _check_sums(s3, base.double(), host["ref_sums"], what + " colsum alone, added to")


def _refused(case, d, with_res, sums=True):
    """the call answers CN_EUNSUPPORTED and leaves gu and the sum destinations as they were"""
    from confignet_amd import ops
    gq = C.geom(case)
    y, s1, s2 = GuardedOut(ops.geom_in_shape(gq, upsampled=True)), GuardedOut((gq.cin,)), GuardedOut((gq.cin,))
    rc = _mask_call(case, d, y.out, with_res, s1.out if sums else None, s2.out if sums else None)
    torch.cuda.synchronize()
    assert rc == CN_EUNSUPPORTED, rc
    assert y.untouched() and s1.untouched() and s2.untouched()


def _plain_inputs(case, seed):
    from confignet_amd import ops
    host = C.integer_inputs(case)
    host["mask"] = _mask_like(ops.geom_in_shape(C.geom(case), upsampled=True), seed).double()
    return {k: v.float().cuda() for k, v in host.items()}


def test_a_launch_that_splits_k_is_refused_with_nothing_written():
    """n = 1, 4 x 4, K = 2048, N = 64: the query says so (the plan of the residual request splits), and the call writes nothing"""
    from confignet_amd._lib import lib
    case = ((1, 4, 4, 64), (1, 1), 2048, 1, 0, None)
    gq = C.request_geom(case, "dgrad_w")
    assert (C.rows(gq), gq.cin, gq.cout) == (16, 2048, 64)
    out8 = (ctypes.c_int * 8)()
    assert lib.cn_conv_fwd_plan(ctypes.byref(gq), 1, 0, ACT_NONE, 0, 0, CN_F32, CN_F32, ctypes.byref(out8)) == 0 and out8[2] > 1, list(out8)
    for has_res in (0, 1):
        rc = lib.cn_conv_fwd_plan_ep(ctypes.byref(gq), 1, 0, ACT_NONE, has_res, 0, 1, CN_F32, CN_F32, ctypes.byref(out8))
        assert rc == CN_EUNSUPPORTED and list(out8) == [UNSUPPORTED, -1, 1, 0, -1, 0, 0, 0], (rc, list(out8))
    d = _plain_inputs(case, 21)
    _refused(case, d, False)
    _refused(case, d, True)


def test_an_upsampled_geometry_is_refused_with_nothing_written():
    case = ((1, 4, 4, 64), (3, 3), 64, 1, 1, None)
    assert C.geom(case).up == 1
    d = _plain_inputs(case, 22)
    _refused(case, d, False)
    _refused(case, d, True)


def test_sums_in_deterministic_mode_are_refused_with_nothing_written():
    """the atomics fix no order of additions: with sums both entries refuse; without sums the launch is the same one"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    ops.set_deterministic(True)
    case = FWD2_CASES["p162"]
    d = _fwd2_inputs("p162")[1]
    _refused(case, d, False)
    _refused(case, d, True)
    n, h, w, cin, cout = WINO_CASES["w6"]
    dw = _wino_inputs("w6")[1]
    p, s = ops._ptr, ops._stream()
    u = torch.empty((16, cin, cout), device="cuda", dtype=torch.float32)
    ops.check(lib.cn_conv_wino_filter(p(dw["w"]), p(u), cout, cin, 1, s), "cn_conv_wino_filter")
    y, s1 = GuardedOut((n, h, w, cout)), GuardedOut((cout,))
    assert lib.cn_conv_fwd_wino_ep(n, h, w, cin, cout, p(dw["gy"]), p(u), p(y.out), p(dw["mask"]), p(s1.out), None, s) == CN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert y.untouched() and s1.untouched()
    y = GuardedOut(ops.geom_in_shape(C.geom(case), upsampled=True))
    assert _mask_call(case, d, y.out, False, None, None) == 0
    torch.cuda.synchronize()
    assert y.intact() and torch.equal(y.out.cpu().double(), _fwd2_ref("p162", False)[0])
