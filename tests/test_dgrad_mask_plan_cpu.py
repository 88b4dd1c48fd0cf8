"""The plan of a data gradient with the mask epilogue (cn_conv_dgrad_w_mask), checked without a GPU through cn_conv_fwd_plan_ep
(csrc/conv_dispatch.hip: plan_conv_fwd) over every geometry of tests/golden/conv_plans.json: without the mask the query is
cn_conv_fwd_plan; with it the request is planned as one with a residual that only the LDS-DMA loop serves."""
import ctypes
import json
import os

import pytest

from confignet_amd._lib import CN_EUNSUPPORTED, CN_F32, CnConvGeom, lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plans.json")
FIELDS = [n for n, _ in CnConvGeom._fields_]
FWD2, UNSUPPORTED = 8, 10
ACT_NONE, ACT_LRELU = 0, 1


def make_geom(values):
    g = CnConvGeom()
    for name, v in zip(FIELDS, values):
        setattr(g, name, v)
    return g


def plan(g, bt, has_bias, act, has_res, stats_mode):
    out = (ctypes.c_int * 8)()
    rc = lib.cn_conv_fwd_plan(ctypes.byref(g), bt, has_bias, act, has_res, stats_mode, CN_F32, CN_F32, ctypes.byref(out))
    return rc, list(out)


def plan_ep(g, bt, has_bias, act, has_res, stats_mode, has_mask):
    out = (ctypes.c_int * 8)()
    rc = lib.cn_conv_fwd_plan_ep(ctypes.byref(g), bt, has_bias, act, has_res, stats_mode, has_mask, CN_F32, CN_F32, ctypes.byref(out))
    return rc, list(out)


@pytest.fixture(scope="module")
def geoms():
    table = json.load(open(GOLDEN))
    assert table["fields"] == FIELDS
    return [(e["name"], make_geom(e["g"])) for e in table["layers"]]


def test_the_table_has_its_195_geometries(geoms):
    assert len(geoms) == 195


def test_without_the_mask_the_query_is_cn_conv_fwd_plan(geoms):
    for name, g in geoms:
        for bt in (0, 1):
            for has_bias, act, has_res, stats_mode in ((0, ACT_NONE, 0, 0), (0, ACT_NONE, 1, 0), (1, ACT_LRELU, 0, 0), (1, ACT_LRELU, 0, 1)):
                assert plan_ep(g, bt, has_bias, act, has_res, stats_mode, 0) == plan(g, bt, has_bias, act, has_res, stats_mode), (name, bt)


def test_a_mask_request_plans_like_a_residual_request_on_the_lds_dma_loop_and_nowhere_else(geoms):
    served = refused = 0
    for name, g in geoms:
        for bt in (0, 1):
            rc_res, p_res = plan(g, bt, 0, ACT_NONE, 1, 0)
            for has_res in (0, 1):
                rc, p = plan_ep(g, bt, 0, ACT_NONE, has_res, 0, 1)
                if p_res[0] == FWD2:
                    assert rc_res == 0 and (rc, p) == (rc_res, p_res), (name, bt, has_res, p, p_res)
                    assert p[2] == 1, (name, bt, has_res, p)          # (never a K split)
                    served += 1
                else:
                    assert rc == CN_EUNSUPPORTED and p == [UNSUPPORTED, -1, 1, p[3], -1, 0, 0, 0], (name, bt, has_res, rc, p)
                    refused += 1
    assert served >= 50 and refused >= 50
