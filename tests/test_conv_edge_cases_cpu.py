"""What the forward / data-gradient edge tests (tests/test_conv_edges_gpu.py) rest on, checked without a GPU: the geometry table of
tests/conv_edge_cases.py reaches every launching route of plan_conv_fwd (csrc/conv_dispatch.hip), both row orders on both
implicit-GEMM routes, every K-slice class and every fused request; a forced tile and split reach the kernel they name; the exactness
precondition A < 2^24 holds for every entry and request; and the float64 reference on integer inputs is the integer result exactly.
tests/golden/conv_edge_plans.json pins (return code, route, tile, K slices, parity order, profile family) per entry and request, so a
later change to the plan cannot quietly move an entry off the arm it is there for."""
import json
import os

import pytest
import torch

from confignet_amd._lib import lib
from tests import conv_edge_cases as C
from tests import test_conv_plan_cpu as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_edge_plans.json")


@pytest.fixture(autouse=True)
def _no_tuning_left_behind():
    yield
    lib.cn_conv_tune(-1, 0, 0)
    lib.cn_conv_loop_select(-1, 0, 0, -1)


def _plans():
    return {name: {r: C.plan_of(case, r) for r in C.REQUESTS} for name, case in C.TABLE.items()}


def test_the_pinned_plans_of_the_table():
    pinned = json.load(open(GOLDEN))
    assert set(pinned) == set(C.TABLE)
    for name, plans in _plans().items():
        for r, got in plans.items():
            assert (None if got is None else list(got)) == pinned[name][r], (name, r, got)


def test_the_table_reaches_every_route_row_order_slice_class_and_fused_request():
    plans = _plans()
    launched = [(n, r, p) for n, reqs in plans.items() for r, p in reqs.items() if p is not None and p[0] == 0]
    routes = {p[1] for _, _, p in launched}
    assert routes == set(C.LAUNCHING_ROUTES), [C.ROUTE_NAMES[r] for r in set(C.LAUNCHING_ROUTES) - routes]
    for route in (C.FWD2, C.IGEMM):
        assert {p[4] for _, _, p in launched if p[1] == route} == {0, 1}, C.ROUTE_NAMES[route]
        assert {p[2] for _, _, p in launched if p[1] == route} >= {2, 3}, C.ROUTE_NAMES[route]
    assert {C.split_class(p[3]) for _, _, p in launched if p[1] in (C.FWD2, C.IGEMM)} == {"1", "2-7", "8-15", "16"}
    # the plain form of the LDS-DMA loop: a 1x1 stride-1 layer it takes (plan_conv_fwd: p.plain)
    assert plans["i52"]["fwd"][1] == C.FWD2 and C.TABLE["i52"][1] == (1, 1) and C.TABLE["i52"][3] == 1
    assert plans["i36"]["fwd"][1] == C.IGEMM and plans["i16"]["fwd"][1] == C.IGEMM          # below g_fwd2_min_c / not above g_fwd2_min_nks
    for req in ("stats", "res", "dgrad_w_res", "fwd_dt", "dgrad_dt", "dgrad_w"):
        assert any(r == req for _, r, _ in launched), req
    # a fused request drops the split the plain one takes; a refused request carries its code
    assert plans["n192"]["fwd"][3] > 1 and plans["n192"]["res"][3] == 1 and plans["n192"]["stats"][3] == 1
    assert plans["m"]["fwd"][3] == 16 and plans["m"]["res"][0] == P.CN_EUNSUPPORTED
    assert plans["j6"]["dgrad"][:2] == (P.CN_EINVAL, C.UNSUPPORTED)
    # what single entries are there for
    assert plans["a"]["dgrad"][1] == C.IGEMM and C.TABLE["a"][2] % 16 != 0
    assert plans["c"]["dgrad"][4] == 0 and plans["d"]["dgrad"][4] == 1 and plans["h144"]["dgrad"][1:5] == (C.FWD2, 2, 1, 1)
    assert plans["p16"]["dgrad"][1:5] == (C.IGEMM, 3, 1, 1) and plans["kpar"]["dgrad"][1] == C.THIN_PAR_IGEMM
    assert plans["l32"]["fwd"][1:3] == (C.FWD2, 3) and plans["e7"]["fwd"][1] == C.C7S2 and plans["up2k4"]["fwd"][1] == C.UP2K4_RGB
    assert plans["k3"]["fwd"][1] == C.THIN_COOP and plans["k1"]["fwd"][1] == C.THIN
    assert plans["e3s1"]["dgrad"][1] == C.S1_IMAGE_DGRAD and plans["e3s2"]["dgrad"][1] == C.S2_IMAGE_DGRAD
    assert (plans["e3s2"]["dgrad"][4], plans["e3s2even"]["dgrad"][4]) == (0, 1)


def test_every_forced_tile_and_split_reaches_the_kernel_it_names():
    """cn_conv_tune on the entries the two implicit-GEMM routes take: the plan names the forced tile and split, on FWD2 or IGEMM
    (plan_conv_fwd's last rule: the 128x32 tile on more than 32 channels is the register-staged loop's); with the LDS-DMA loop
    switched off every one of them is the register-staged loop's."""
    seen = set()
    for req in ("fwd", "dgrad", "dgrad_w"):
        names = C.gemm_entries(req)
        assert len(names) >= 10
        for loop in (-1, 0):
            lib.cn_conv_loop_select(loop, 0, 0, -1)
            for cfg in C.FORCED_CFGS:
                for splits in (1, 3, 8):
                    lib.cn_conv_tune(cfg, splits, 0)
                    for name in names:
                        rc, route, tile, s, par, family = C.plan_of(C.TABLE[name], req)
                        assert rc == 0 and route in (C.FWD2, C.IGEMM) and (tile, s) == (cfg, splits), (name, req, cfg, splits, route, tile, s)
                        assert loop != 0 or route == C.IGEMM, (name, req)
                        gq = C.request_geom(C.TABLE[name], req)
                        if route == C.FWD2:
                            assert cfg != 3 or gq.cout == 32, (name, req)
                        seen.add((route, cfg, C.split_class(s), par))
            lib.cn_conv_loop_select(-1, 0, 0, -1)
    for route in (C.FWD2, C.IGEMM):
        for cfg in C.FORCED_CFGS:
            for cls in ("1", "2-7", "8-15"):
                for par in (0, 1):
                    assert (route, cfg, cls, par) in seen, (C.ROUTE_NAMES[route], cfg, cls, par)


@pytest.mark.parametrize("name", list(C.TABLE))
def test_the_exactness_precondition_and_the_reference(name):
    """A < 2^24 for every request of the entry; float64 and float32 arithmetic on the CPU give the same integers (the reference is
    right and the sum really does not depend on its order); K = taps * cin <= 4608 and M stays small."""
    case = C.TABLE[name]
    g = C.geom(case)
    assert C.ktot(g) <= 4608 and C.rows(g) < 1100
    inp = C.integer_inputs(case)
    assert all(float(v.abs().max()) <= 3.0 and torch.equal(v, v.round()) for v in inp.values()) and float(inp["x"].abs().max()) == 3.0
    for req in ("fwd", "res", "dgrad", "dgrad_w_res"):
        A = C.exact_bound(case, req, inp)
        assert float(A.max()) < 2 ** 24, (name, req)
        ref = C.reference(case, req, inp)
        ref32 = C.reference(case, req, inp, dtype=torch.float32)
        assert ref.dtype == torch.float64 and bool((ref.abs() <= A).all())
        assert torch.equal(ref * 4, (ref * 4).round()) and float(ref.abs().max()) > 0
        assert torch.equal(ref.float(), ref32), (name, req)
        assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("name", C.STATS_NAMES)
def test_the_statistics_sums_are_exact(name):
    """sum a, sum a^2 (mode 1) and sum v, sum v^2, sum l, sum l^2 (mode 2): integers below 2^24, or multiples of 1/16 below 2^20"""
    case = C.TABLE[name]
    assert C.plan_of(case, "stats")[:2] == (0, C.FWD2)
    for mode in (1, 2):
        inp = C.stats_inputs(name, mode)
        pre = C._conv(case, inp["x"], inp["w"], inp["bias"])
        whole, sixteenth = C.stats_bounds(pre, mode, case[0][0])
        assert whole < 2 ** 24 and sixteenth < 2 ** 20, (name, mode, whole, sixteenth)
        st = C.stats_reference(C._act(pre, P.ACT_LRELU) if mode == 1 else pre, mode, case[0][0])
        assert torch.equal(st * 16, (st * 16).round()) and torch.equal(st.float().double(), st)


def test_the_bf16_geometries_reach_every_tile_of_the_bf16_rule():
    """conv_bf16 (csrc/igemm_bf16.hip) picks its tile by launch size alone: the table reaches 64x64 and 128x32, BF16_EXTRA adds one
    geometry each for 128x128, 128x64 and 128x96 and one whose cin is no multiple of 32 (the register-staged kernel)."""
    assert {n: C.bf16_tile(C.geom(c)) for n, c in C.BF16_EXTRA.items()} == {"t128x128": 0, "t128x64": 1, "t128x96": 4, "t128x128-cin40": 0}
    fwd = {C.bf16_tile(C.geom(C.TABLE[n])) for n in C.BF16_TABLE} | {C.bf16_tile(C.geom(c)) for c in C.BF16_EXTRA.values()}
    assert fwd == {0, 1, 2, 3, 4}
    assert len(C.BF16_TABLE) >= 10 and all(C.TABLE[n][0][-1] % 8 == 0 and C.TABLE[n][2] % 8 == 0 for n in C.BF16_TABLE)
    for n, c in C.BF16_EXTRA.items():
        g = C.geom(c)
        assert C.rows(g) == 8190 and C.rows(g) % 128 != 0 and g.cout % 64 != 0 and 9 * C.ktot(g) + 6 < 2 ** 24
        assert (g.cin % 32 != 0) == (n == "t128x128-cin40")


def test_winograd_filters_that_are_multiples_of_four_keep_the_transform_exact():
    """F(2x2, 3x3): the filter transform G g G^T has rows (g0 + g1 + g2) / 2 and (g0 - g1 + g2) / 2, twice: with entries that are
    multiples of 4 in [-12, 12] every transformed entry is an integer of at most 27 in size; the input transform only adds."""
    G = torch.tensor([[1.0, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1.0]], dtype=torch.float64)
    w = torch.randint(-3, 4, (3, 3, 500), generator=torch.Generator().manual_seed(1)).double() * 4
    u = torch.einsum("ai,ijc,bj->abc", G, w, G)
    assert torch.equal(u, u.round()) and float(u.abs().max()) <= 27
    for xs, cout in C.WINO_SHAPES:
        # |x| <= 3: transformed input <= 12, products <= 324 a channel, output transform adds 9 of the 16: 9 * 324 * cin + bias < 2^24
        assert 9 * 12 * 27 * xs[-1] + 3 < 2 ** 24 and xs[-1] % 16 == 0 and cout % 64 == 0
