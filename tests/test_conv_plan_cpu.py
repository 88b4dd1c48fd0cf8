"""Which launch a convolution gets, checked without a GPU through cn_conv_fwd_plan (csrc/conv_dispatch.hip: plan_conv_fwd is the
function the calls themselves decide with).  tests/golden/conv_plans.json pins route / tile / K split / row order / profile family /
grid for the layer shapes of the GPU tests, the batch-16 256^2 iteration and one case per route and split-rule arm; the invariants
below hold over that whole list."""
import ctypes
import json
import os

import pytest

from confignet_amd._lib import CN_BF16, CN_EUNSUPPORTED, CN_F32, CnConvGeom, lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")
FIELDS = [n for n, _ in CnConvGeom._fields_]
CN_EINVAL = -1
(UP2K4_RGB, S2_IMAGE_DGRAD, S1_IMAGE_DGRAD, THIN_PAR_IGEMM, THIN_COOP, THIN, C3, C7S2, FWD2, IGEMM, UNSUPPORTED) = range(11)
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2

# request name -> (data-gradient geometry?, bt, has_bias, act, has_res, stats_mode, x_dt, y_dt): the calls of the pinned table
REQUESTS = {
    "fwd": (False, 0, 1, ACT_LRELU, 0, 0, CN_F32, CN_F32),
    "res": (False, 0, 1, ACT_RELU, 1, 0, CN_F32, CN_F32),
    "stats": (False, 0, 1, ACT_LRELU, 0, 1, CN_F32, CN_F32),
    "fwd_dt": (False, 0, 1, ACT_LRELU, 0, 0, CN_F32, CN_BF16),
    "dgrad": (True, 0, 0, ACT_NONE, 0, 0, CN_F32, CN_F32),
    "dgrad_w": (True, 1, 0, ACT_NONE, 0, 0, CN_F32, CN_F32),
    "dgrad_w_res": (True, 1, 0, ACT_NONE, 1, 0, CN_F32, CN_F32),
    "dgrad_dt": (True, 0, 0, ACT_NONE, 0, 0, CN_BF16, CN_F32),
}


def make_geom(values):
    g = CnConvGeom()
    for name, v in zip(FIELDS, values):
        setattr(g, name, v)
    return g


def dgrad_geom(g):
    """csrc/conv_geom.h: dgrad_geom -- the geometry cn_conv_dgrad* plan with (defined for dl = 1)."""
    d = make_geom([getattr(g, n) for n in FIELDS])
    d.in_d, d.in_h, d.in_w, d.cin = g.out_d, g.out_h, g.out_w, g.cout
    d.out_d, d.out_h, d.out_w, d.cout = (1 if g.nd == 2 else g.in_d << g.up), g.in_h << g.up, g.in_w << g.up, g.cin
    d.s_d = d.s_h = d.s_w = 1
    d.dl_d, d.dl_h, d.dl_w = g.s_d, g.s_h, g.s_w
    d.p_d, d.p_h, d.p_w = g.k_d - 1 - g.p_d, g.k_h - 1 - g.p_h, g.k_w - 1 - g.p_w
    d.up = 0
    return d


def plan(g, bt=0, has_bias=0, act=ACT_NONE, has_res=0, stats_mode=0, x_dt=CN_F32, y_dt=CN_F32):
    """(return code, [route, cfg, splits, par, family, grid x, y, z])"""
    out = (ctypes.c_int * 8)()
    rc = lib.cn_conv_fwd_plan(ctypes.byref(g), bt, has_bias, act, has_res, stats_mode, x_dt, y_dt, ctypes.byref(out))
    return rc, list(out)


def request_geom(g, name):
    """the geometry request `name` plans with, or None where the call refuses the layer before planning"""
    if not REQUESTS[name][0]:
        return g
    if (g.dl_d, g.dl_h, g.dl_w) != (1, 1, 1):
        return None
    if name == "dgrad_w_res" and (g.up or (g.s_d, g.s_h, g.s_w) != (1, 1, 1)):
        return None
    return dgrad_geom(g)


def plan_request(g, name):
    gq = request_geom(g, name)
    return None if gq is None else plan(gq, *REQUESTS[name][1:])


@pytest.fixture(scope="module")
def table():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def geoms(table):
    return [(e["name"], make_geom(e["g"])) for e in table["layers"]]


@pytest.fixture(autouse=True)
def _no_tuning_left_behind():
    yield
    lib.cn_conv_tune(-1, 0, 0)


def test_the_pinned_plans(table):
    assert table["fields"] == FIELDS and len(table["layers"]) >= 150
    seen = set()
    for e in table["layers"]:
        g = make_geom(e["g"])
        assert set(e["plans"]) == set(REQUESTS)
        for name, want in e["plans"].items():
            got = plan_request(g, name)
            assert (None if got is None else [got[0]] + got[1]) == want, (e["name"], name)
            if got is not None:
                seen.add(got[1][0])
    assert seen == set(range(11)), "the table no longer reaches every route"


def test_a_fused_request_never_plans_a_k_split(geoms):
    for forced in (0, 3, 8):
        lib.cn_conv_tune(-1, forced, 0)
        for name, g in geoms:
            for req in ("res", "stats", "dgrad_w_res"):
                got = plan_request(g, req)
                if got is not None:
                    assert got[1][2] == 1, (name, req, forced, got)


def test_the_data_gradient_from_the_original_filter_plans_like_the_one_from_the_flipped_copy(geoms):
    """cn_conv_dgrad_w plans dgrad_geom(g) with bt = 1: where that launches it is the launch cn_conv_dgrad (bt = 0) gets for the same
    geometry; where it does not, the layer is one the vectorised implicit-GEMM kernels do not take."""
    launched = 0
    for name, g in geoms:
        if request_geom(g, "dgrad_w") is None:
            continue
        d = dgrad_geom(g)
        rc1, p1 = plan(d, bt=1)
        rc0, p0 = plan(d, bt=0)
        assert (rc1, p1) == plan_request(g, "dgrad_w")
        if rc1 == 0:
            assert p1[0] in (FWD2, IGEMM) and (rc0, p0) == (rc1, p1), name
            launched += 1
        else:
            assert rc1 == CN_EUNSUPPORTED and p1[0] == UNSUPPORTED and (d.cout <= 4 or d.cin % 16 or d.cout % 4), name
    assert launched >= 50


def test_a_forced_tile_and_split_is_honoured_by_the_gemm_routes_and_ignored_by_the_others(geoms):
    base = {name: plan(g, has_bias=1, act=ACT_LRELU) for name, g in geoms}
    gemm = 0
    for cfg in range(5):
        for splits in (1, 3, 8):
            lib.cn_conv_tune(cfg, splits, 0)
            for name, g in geoms:
                rc, p = plan(g, has_bias=1, act=ACT_LRELU)
                if base[name][1][0] in (FWD2, IGEMM):
                    assert rc == 0 and p[0] in (FWD2, IGEMM) and (p[1], p[2]) == (cfg, splits), (name, cfg, splits, p)
                    gemm += 1
                else:
                    assert (rc, p) == base[name], (name, cfg, splits)
    assert gemm >= 15 * 50


def test_a_plan_without_a_launch_carries_its_code_and_no_grid(geoms):
    refused = 0
    for name, g in geoms:
        for req in REQUESTS:
            got = plan_request(g, req)
            if got is None:
                continue
            rc, p = got
            gq = request_geom(g, req)
            if p[0] == UNSUPPORTED:
                # an argument error where the fp32 call reports one (an implicit-GEMM layer with cout % 4 != 0, a thin layer whose
                # filter does not fit the LDS stage), CN_EUNSUPPORTED everywhere else
                fused = req in ("res", "stats", "dgrad_w_res", "dgrad_w", "fwd_dt", "dgrad_dt")
                bad_arg = not fused and ((gq.cout > 4 and gq.cout % 4 != 0) or (gq.cout <= 4 and 16 * gq.k_d * gq.k_h * gq.k_w * gq.cin > 65536))
                assert rc == (CN_EINVAL if bad_arg else CN_EUNSUPPORTED), (name, req, rc)
                assert p[1:] == [-1, 1, p[3], -1, 0, 0, 0], (name, req, p)
                refused += 1
            else:
                assert rc == 0 and p[5] >= 1 and p[6] >= 1 and p[7] >= 1, (name, req, p)
                assert p[7] == (p[2] if p[0] in (FWD2, IGEMM) else 1), (name, req, p)
    assert refused >= 100
