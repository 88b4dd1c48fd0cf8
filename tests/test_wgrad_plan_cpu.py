"""Which launch a filter gradient gets, checked without a GPU through cn_conv_wgrad_plan (csrc/conv_dispatch.hip: plan_conv_wgrad is
the function the calls themselves decide with).  tests/golden/wgrad_plans.json holds RECORDED results: what the entry points of the
commit before plan_conv_wgrad existed launched for each geometry, read off a host-only launch trace of that commit (DESIGN.md,
"Convolution dispatch") in default and in deterministic mode -- never generated from the plan function it pins.  The geometries are
the layers of tests/golden/conv_plans.json, the tables of tests/wgrad_edge_cases.py and one geometry per arm of every routing
predicate.  ("dt_*": the routed call cn_conv_wgrad_dt, recorded as the chain of older entry points ops.conv_wgrad used to walk.)
The file names a plan once per layer for all the requests that got it, leaves out the requests for which nothing was launched
("unsupported") and lists under "deterministic" only what differs from "default"; `table` below spells every request out again."""
import ctypes
import json
import os

import pytest

from confignet_amd._lib import CN_BF16, CN_EUNSUPPORTED, CN_F32, CnConvGeom, lib
from tests import wgrad_edge_cases as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plans.json")
FIELDS = [n for n, _ in CnConvGeom._fields_]
CN_EINVAL = -1
C3, THIN, TINY, WGRAD2, IGEMM, BF16, NONE = range(7)
ALL = 0xFFFFFFFF
DET_WS_FLOATS = 16 << 20          # csrc/common.h: CN_DET_WS_FLOATS, the deterministic workspace of one stream
MODES = {"default": 0, "deterministic": 1}

# request name -> (x storage type, gy storage type, slabs left to the caller, routes the entry point takes)
REQUESTS = {
    "atomic": (CN_F32, CN_F32, 0, 1 << TINY | 1 << IGEMM),                     # cn_conv_wgrad
    "ws": (CN_F32, CN_F32, 0, 1 << WGRAD2 | 1 << TINY | 1 << IGEMM),           # cn_conv_wgrad_ws, cn_conv_wgrad_workspace_bytes
    "slabs": (CN_F32, CN_F32, 1, 1 << WGRAD2 | 1 << TINY | 1 << IGEMM),        # cn_conv_wgrad_ws_slabs
    "bf16": (CN_BF16, CN_BF16, 0, 1 << BF16),                                  # cn_conv_wgrad_bf16
    "c3_f32": (CN_F32, CN_F32, 0, 1 << C3),                                    # cn_conv_wgrad_c3
    "c3_bf16": (CN_F32, CN_BF16, 0, 1 << C3),
    "thin": (CN_F32, CN_F32, 0, 1 << THIN),                                    # cn_conv_wgrad_thin
    "dt_f32": (CN_F32, CN_F32, 0, ALL),                                        # cn_conv_wgrad_dt
    "dt_f32_slabs": (CN_F32, CN_F32, 1, ALL),
    "dt_mixed": (CN_F32, CN_BF16, 0, ALL),
    "dt_bf16": (CN_BF16, CN_BF16, 0, ALL),
}


def make_geom(values):
    g = CnConvGeom()
    for name, v in zip(FIELDS, values):
        setattr(g, name, v)
    return g


def plan(g, request, det=0):
    """(return code, [route, tile, slices, rows, family, grid x, y, z, workspace floats, zero pass, what follows, stages])"""
    x_dt, gy_dt, slabs, routes = REQUESTS[request]
    out = (ctypes.c_longlong * 12)()
    rc = lib.cn_conv_wgrad_plan(ctypes.byref(g), x_dt, gy_dt, slabs, routes, det, out)
    return rc, list(out)


@pytest.fixture(scope="module")
def table():
    doc = json.load(open(GOLDEN))
    for e in doc["layers"]:
        full = {r: doc["unsupported"] for r in doc["requests"]}
        e["plans"] = {}
        for mode in MODES:              # ("default" first: "deterministic" starts from it)
            for names, plan_ in e[mode].items():
                assert set(names.split()) <= set(full), names
                full.update({r: plan_ for r in names.split()})
            e["plans"][mode] = dict(full)
    return doc


@pytest.fixture(scope="module")
def geoms(table):
    return [(e["name"], make_geom(e["g"])) for e in table["layers"]]


@pytest.fixture(autouse=True)
def _no_tuning_left_behind():
    yield
    lib.cn_conv_tune(-1, 0, 0)
    lib.cn_conv_loop_select(-1, 0, 0, -1)


def test_the_pinned_plans(table):
    """route, tile, slices, rows, family, grid, workspace and zero pass of every request, in both modes"""
    assert table["fields"] == FIELDS and table["requests"] == list(REQUESTS) and len(table["layers"]) >= 250
    assert table["plan"] == ["rc", "route", "tile", "slices", "rows", "family", "grid_x", "grid_y", "grid_z", "workspace_floats", "zero_pass"]
    seen = {m: set() for m in MODES}
    for e in table["layers"]:
        g = make_geom(e["g"])
        assert set(e["plans"]) == set(MODES)
        for mode, det in MODES.items():
            assert set(e["plans"][mode]) == set(REQUESTS)
            for name, want in e["plans"][mode].items():
                rc, p = plan(g, name, det)
                assert [rc] + p[:10] == want, (e["name"], mode, name)
                seen[mode].add(p[0])
    for mode in MODES:
        assert seen[mode] == set(range(7)), "the table no longer reaches every route in %s mode" % mode


def test_the_routed_call_takes_what_the_chain_of_entry_points_took(table):
    """cn_conv_wgrad_dt on fp32 operands = the K = 27 entry, else the thin one, else cn_conv_wgrad_ws; on bf16 operands
    cn_conv_wgrad_bf16; with a bf16 gy alone the K = 27 entry or nothing -- read off the recorded table itself"""
    for e in table["layers"]:
        for mode in MODES:
            p = e["plans"][mode]
            chain = next((p[r] for r in ("c3_f32", "thin") if p[r][1] != NONE), p["ws"])
            assert p["dt_f32"] == chain, (e["name"], mode)
            assert p["dt_f32_slabs"] == next((p[r] for r in ("c3_f32", "thin") if p[r][1] != NONE), p["slabs"]), (e["name"], mode)
            assert p["dt_mixed"] == p["c3_bf16"] and p["dt_bf16"] == p["bf16"], (e["name"], mode)


def test_a_plan_without_a_route_carries_its_code_no_grid_and_no_workspace(geoms):
    refused = 0
    for name, g in geoms:
        for det in (0, 1):
            for req in REQUESTS:
                rc, p = plan(g, req, det)
                if p[0] == NONE:
                    # an argument error only where the atomic kernel's partial filter does not fit the deterministic workspace
                    too_big = det == 1 and W.ktot(g) * g.cout > DET_WS_FLOATS and REQUESTS[req][0] == CN_F32 and REQUESTS[req][1] == CN_F32 \
                        and REQUESTS[req][3] & (1 << IGEMM)
                    assert rc == (CN_EINVAL if too_big else CN_EUNSUPPORTED), (name, req, det, rc)
                    assert p[1:] == [-1, 1, 0, -1, 0, 0, 0, 0, 0, 0, 0], (name, req, p)
                    refused += 1
                else:
                    assert rc == 0 and p[5] >= 1 and p[6] >= 1 and p[7] >= 1 and p[2] >= 1, (name, req, p)
    assert refused >= 1000
    assert any(plan(g, "atomic", 1)[0] == CN_EINVAL for _, g in geoms)


def test_a_forced_tile_and_target_is_honoured_by_the_lds_dma_route_and_ignored_by_the_others(geoms):
    base = {(name, req): plan(g, req) for name, g in geoms for req in ("dt_f32", "dt_bf16", "atomic")}
    honoured = 0
    for tile in W.TILES:
        for want in (1, 8):
            for name, g in geoms:
                target = want * W.tiles_of(g, tile)
                lib.cn_conv_tune(tile[0], 0, target)
                rc, p = plan(g, "dt_f32")
                b = base[(name, "dt_f32")]
                if b[1][0] == WGRAD2:
                    m, kb = W.rows(g), tile[4]
                    assert rc == 0 and p[0] == WGRAD2 and p[1] == tile[0] and p[2] == W.replayed_splits(g, tile, want), (name, tile[1], want, p)
                    assert p[3] % kb == 0 and -(-m // p[3]) == p[2], (name, p)                 # rows per slice: whole stages, and they cover M
                    honoured += 1
                elif b[1][0] == IGEMM:
                    # the atomic kernel keeps its own tile and takes the workgroup target alone
                    assert rc == b[0] and p[0] == IGEMM and p[1] == b[1][1] and p[4] == b[1][4], (name, tile[1], want, p)
                else:
                    assert (rc, p) == b, (name, tile[1], want)
                assert plan(g, "dt_bf16") == base[(name, "dt_bf16")], (name, tile[1], want)
                ra, pa = plan(g, "atomic")
                assert pa[0] == base[(name, "atomic")][1][0] and pa[1] == base[(name, "atomic")][1][1], (name, tile[1], want)
    assert honoured >= 10 * 100
    # a tile the filter gradient does not have (128 x 64) leaves every plan as it is
    lib.cn_conv_tune(1, 0, 0)
    for name, g in geoms:
        assert plan(g, "dt_f32") == base[(name, "dt_f32")], name


def test_the_stage_count_is_forced_on_the_lds_dma_route_only(geoms):
    base = {name: plan(g, "dt_f32") for name, g in geoms}
    lib.cn_conv_loop_select(-1, 0, 3, -1)
    for name, g in geoms:
        rc, p = plan(g, "dt_f32")
        assert (rc, p[:11]) == (base[name][0], base[name][1][:11]), name
        if p[0] == WGRAD2:              # (the 128 x 32 tile always has three stages)
            assert p[11] == 3 and base[name][1][11] == (3 if p[1] == 3 else 4), (name, p)
        else:
            assert p[11] == 0 and base[name][1][11] == 0, (name, p)


def test_the_workspace_the_query_reports_is_the_workspace_the_plan_uses(geoms):
    tunings = [(-1, 0)] + [(tile[0], want) for tile in W.TILES for want in (3, 11)]
    asked = 0
    for cfg, want in tunings:
        for name, g in geoms:
            lib.cn_conv_tune(cfg, 0, 0 if cfg < 0 else want * W.tiles_of(g, [t for t in W.TILES if t[0] == cfg][0]))
            rc, p = plan(g, "ws", det=-1)
            assert int(lib.cn_conv_wgrad_workspace_bytes(ctypes.byref(g))) == 4 * p[8], (name, cfg, want)
            assert p[8] == (p[2] * W.ktot(g) * g.cout if p[0] == WGRAD2 and p[2] > 1 else 0), (name, p)
            for req in ("dt_f32", "dt_mixed", "dt_bf16"):
                nbytes = ctypes.c_size_t(12345)
                rq = lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), REQUESTS[req][0], REQUESTS[req][1], ctypes.byref(nbytes))
                rc, p = plan(g, req, det=-1)
                assert rq == rc and nbytes.value == 4 * p[8], (name, req, cfg, want)
                assert (p[8] > 0) == (p[0] in (C3, THIN) or (p[0] == WGRAD2 and p[2] > 1)), (name, req, p)
                asked += 1
    assert asked >= 3 * 250 * 11


def test_in_deterministic_mode_no_plan_of_the_atomic_kernel_exceeds_the_stream_workspace(geoms):
    clamped = 0
    for cfg, target in ((-1, 0), (-1, 256), (-1, 100000), (0, 4096)):
        lib.cn_conv_tune(cfg, 0, target)
        for name, g in geoms:
            for req in ("atomic", "ws", "dt_f32"):
                rc, p = plan(g, req, det=1)
                if p[0] == IGEMM:
                    assert p[2] * W.ktot(g) * g.cout <= DET_WS_FLOATS, (name, req, p)
                    free = plan(g, req, det=0)[1]
                    assert free[0] == IGEMM and p[2] <= free[2], (name, req)
                    clamped += p[2] < free[2]
    assert clamped >= 3
