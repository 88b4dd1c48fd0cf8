"""The 64 x 48 body of the LDS-DMA loop (csrc/fwd2.hip: 16-wide MFMA blocks, v_mfma_f32_16x16x4_f32) -- the data gradient from the
original filter into a 48-channel tensor, through cn_conv_dgrad_w / cn_conv_dgrad_w_res.

Exact cases by the method of tests/conv_edge_cases.py: integer inputs in [-3, 3], every partial sum an integer below 2^24, so the
result equals the float64 reference bit for bit in any order of the adds; outputs are views into sentinel-guarded allocations.  Every
launch first asserts through cn_fwd2_col_block -- the function cn_fwd2 selects with -- which body it takes: a test that ran the
64 x 64 body where it means the 64 x 48 one fails.  One random-valued case checks the accumulate arithmetic against the float64
oracle at the family's bar, 2e-4 of the output scale (tests/test_ops_gpu.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_edge_cases as C
from tests.test_conv_edges_gpu import GuardedOut, _call, _compare

# id -> (x shape, kernel, cout, stride, up, explicit pad) of the FORWARD convolution (cin = 48: the data gradient's 48 columns)
CASES = {
    "a": ((2, 16, 12, 48), (3, 3), 96, 2, 0, None),          # even extents: parity classes of 1 / 2 / 2 / 4 taps, tiles straddling two classes
    "b": ((2, 17, 13, 48), (3, 3), 96, 2, 0, None),          # odd extents: not parity-ordered, M = 442 with a partial last tile
    "c": ((1, 8, 8, 48), (3, 3), 48, 2, 0, None),            # the 1-tap class has 3 K steps: fewer than the 4 stages
    "d": ((1, 5, 7, 48), (3, 3), 64, 1, 0, None),            # M = 35 < 64; 4 K steps per tap = the stage count
    "e": ((3, 8, 16, 48), (3, 3), 96, 1, 0, None),           # forced K splits, atomics and deterministic slabs
    "f": ((2, 3, 5, 4, 48), (3, 3, 3), 64, 1, 1, None),      # the 3-D parity-balanced form
    "r": ((2, 32, 32, 48), (3, 3), 96, 2, 0, None),          # the random-valued case
}
DEFAULT_LOOP = (-1, 0, 0, -1)


@functools.lru_cache(maxsize=None)
def _inputs(name, real=False):
    from confignet_amd import ops
    host = C.integer_inputs(CASES[name], real=real)
    if not real:
        assert float(C.exact_bound(CASES[name], "dgrad_w_res", host).max()) < 2 ** 24
    dev = {k: v.float().cuda() for k, v in host.items()}
    dev["wt"] = ops.weight_tflip(dev["w"])
    torch.cuda.synchronize()
    return host, dev


@functools.lru_cache(maxsize=None)
def _ref64(name, request, real=False):
    """float64 reference on the CPU: computed once, shared, never changed"""
    return C.reference(CASES[name], request, _inputs(name, real)[0])


@functools.lru_cache(maxsize=None)
def _ref(name, request):
    return _ref64(name, request).float().cuda()


def _col_block(name, request, loop):
    """the MFMA column block the request's launch takes under the tuning in force, the loop selection resolved as cn_fwd2 resolves it"""
    from confignet_amd._lib import lib
    case = CASES[name]
    plan = C.plan_of(case, request)
    assert plan is not None and plan[0] == 0 and plan[1] == C.FWD2, (name, request, plan)
    gq = C.request_geom(case, request)
    kb = loop[1] or 16
    if kb == 32 and (gq.cin % 32 != 0 or plan[2] != 2):
        kb = 16
    np_ = loop[3] if loop[3] >= 0 else 0
    if plan[2] != 2 or kb == 32:
        np_ = 0
    gathered = 1                                   # (3x3 / 3x3x3 filters: never the plain 1x1 product)
    return lib.cn_fwd2_col_block(plan[2], C.REQUESTS[request][1], gathered, gq.cout, kb, np_)


def _run(name, request="dgrad_w", loop=DEFAULT_LOOP, block=16):
    """the request on the case under `loop` and the tile / split tuning in force: asserts the body, runs, checks the guards; returns
    the output (a copy)"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = CASES[name]
    d = _inputs(name)[1]
    ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
    try:
        what = "%s %s loop %s plan %s" % (name, request, loop, C.plan_of(case, request))
        assert _col_block(name, request, loop) == block, what + ": not the %d-wide body" % block
        shape = ops.geom_in_shape(C.geom(case), upsampled=True)
        y = GuardedOut(shape)
        rc = _call(case, request, d, y.out)
        assert rc == 0, what + ": " + lib.cn_last_error_string().decode()
        torch.cuda.synchronize()
        assert y.intact(), what + ": a guard was written"
        return y.out.clone(), what
    finally:
        ops.check(lib.cn_conv_loop_select(*DEFAULT_LOOP), "cn_conv_loop_select")


def _exact(name, request="dgrad_w", loop=DEFAULT_LOOP, block=16):
    got, what = _run(name, request, loop, block)
    _compare(got, _ref(name, request), what, 48)
    return got


@pytest.fixture(autouse=True)
def _defaults():
    """every case starts from the built-in plan (the 64 x 64 tile for all of them) and leaves no tuning behind"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    was = ops.DETERMINISTIC
    C.tune(-1, 0)
    yield
    ops.set_deterministic(was)
    ops.check(lib.cn_conv_loop_select(*DEFAULT_LOOP), "cn_conv_loop_select")
    C.tune(-1, 0)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f"])
def test_the_integer_result_on_the_default_loop(name):
    case = CASES[name]
    gq = C.request_geom(case, "dgrad_w")
    assert gq.cout == 48 and C.rows(gq) == {"a": 384, "b": 442, "c": 64, "d": 35, "f": 960}[name]
    assert C.plan_of(case, "dgrad_w")[4] == {"a": 1, "b": 0, "c": 1, "d": 0, "f": 0}[name]           # parity-ordered rows
    assert C.plan_of(case, "dgrad_w")[3] == {"a": 1, "b": 6, "c": 1, "d": 1, "f": 12}[name]          # K slices of the built-in plan
    _exact(name)


def test_fewer_k_steps_than_stages_on_a_forced_loop():
    """case c: the 1-tap parity class has 48 / 16 = 3 K steps; cn_conv_loop_select(1, 16, 3, 0) makes that the stage count"""
    _exact("c", loop=(1, 16, 3, 0))
    _exact("c", loop=(1, 16, 4, 0))


def test_the_residual_in_the_epilogue_is_the_data_gradient_plus_an_add_bit_for_bit():
    """case d, integers (exact) and standard-normal values (the same roundings in the same order: v + res after the last K step)"""
    got = _exact("d", "dgrad_w_res")
    plain = _exact("d", "dgrad_w")
    assert torch.equal(got, plain + _inputs("d")[1]["resx"])
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case, d = CASES["d"], _inputs("d", True)[1]
    assert _col_block("d", "dgrad_w_res", DEFAULT_LOOP) == 16 and _col_block("d", "dgrad_w", DEFAULT_LOOP) == 16
    shape = ops.geom_in_shape(C.geom(case), upsampled=True)
    y0, y1 = GuardedOut(shape), GuardedOut(shape)
    assert _call(case, "dgrad_w", d, y0.out) == 0 and _call(case, "dgrad_w_res", d, y1.out) == 0, lib.cn_last_error_string().decode()
    torch.cuda.synchronize()
    assert y0.intact() and y1.intact()
    assert torch.equal(y1.out, y0.out + d["resx"])


@pytest.mark.parametrize("deterministic", [False, True])
def test_forced_k_splits(deterministic):
    """case e under cn_conv_tune(2, s, 0), s = 1 / 3 / 8: one launch, atomics over a zero pass, and -- deterministic -- partial slabs"""
    from confignet_amd import ops
    ops.set_deterministic(deterministic)
    for splits in (1, 3, 8):
        C.tune(2, splits)
        plan = C.plan_of(CASES["e"], "dgrad_w")
        assert plan[2] == 2 and plan[3] == splits, plan
        _exact("e")


@pytest.mark.parametrize("name", ["a", "b"])
def test_three_and_four_stages_give_the_same_bits(name):
    """standard-normal values: the stage count changes when a K step is loaded, not the order it is added in"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case, d = CASES[name], _inputs(name, True)[1]
    C.tune(2, 1)
    shape = ops.geom_in_shape(C.geom(case), upsampled=True)
    outs = []
    try:
        for loop in ((1, 16, 3, 0), (1, 16, 4, 0)):
            ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
            assert _col_block(name, "dgrad_w", loop) == 16
            y = GuardedOut(shape)
            assert _call(case, "dgrad_w", d, y.out) == 0, lib.cn_last_error_string().decode()
            torch.cuda.synchronize()
            assert y.intact()
            outs.append(y.out.clone())
    finally:
        ops.check(lib.cn_conv_loop_select(*DEFAULT_LOOP), "cn_conv_loop_select")
    assert torch.equal(outs[0], outs[1])
    ref = _ref64(name, "dgrad_w", True)
    assert float((outs[0].cpu().double() - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    _exact(name, loop=(1, 16, 3, 0))
    _exact(name, loop=(1, 16, 4, 0))


@pytest.mark.parametrize("loop", [(1, 32, 0, 0), (1, 16, 0, 1), (1, 16, 0, 2)])
def test_the_forced_variants_keep_the_64_column_body_and_the_integer_result(loop):
    """32-deep stages and loader waves exist on the 64 x 64 body only: the selection must leave them there"""
    for name in ("a", "b"):
        _exact(name, loop=loop, block=32)


def test_random_values_against_the_float64_oracle():
    """(2, 32, 32, 48) -> 96, stride 2: 2e-4 of the output scale, the bar of this family"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case, d = CASES["r"], _inputs("r", True)[1]
    C.tune(-1, 0)                                   # (the layer's own plan: tests/golden/conv_plans.json CONV_CASES[8])
    plan = C.plan_of(case, "dgrad_w")
    assert plan[1:5] == (C.FWD2, 2, 1, 1) and _col_block("r", "dgrad_w", DEFAULT_LOOP) == 16, plan
    y = GuardedOut(ops.geom_in_shape(C.geom(case), upsampled=True))
    assert _call(case, "dgrad_w", d, y.out) == 0, lib.cn_last_error_string().decode()
    torch.cuda.synchronize()
    assert y.intact()
    ref = _ref64("r", "dgrad_w", True)
    err, scale = float((y.out.cpu().double() - ref).abs().max()), float(ref.abs().max())
    print("max |err| %.3e = %.3e of the output scale %.3e" % (err, err / scale, scale))
    assert err <= 2e-4 * scale
