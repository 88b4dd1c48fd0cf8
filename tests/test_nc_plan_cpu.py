"""Which launch a per-(sample, channel) reduction and a per-sample map get, checked without a GPU through cn_nc_reduce_plan and
cn_nc_rows_plan (csrc/elementwise.hip: plan_nc_reduce and plan_nc_rows are the functions the calls themselves decide with).
tests/golden/nc_plans.json holds RECORDED plans: what the formulas written out in nc_reduce_launch, cn_nc_reduce4, cn_nc_reduce_hxt,
cn_nc_lin2 and cn_norm_apply before the plan functions existed give for each shape (their deterministic workspace cap included, which
bound on none of them) -- never generated from the functions it pins.  The shapes are the edge shapes of tests/test_nc_edges_gpu.py
and every distinct call of one 256 x 256, batch-16 training iteration (scripts/ew_shapes_bench.py --shapes)."""
import ctypes
import json
import math
import os

import pytest

from confignet_amd._lib import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nc_plans.json")
DET_WS_FLOATS = 16 << 20          # csrc/common.h: CN_DET_WS_FLOATS, the deterministic workspace of one stream
CN_EINVAL = -1

# (n, s, c) -> V, TX, TY, channel blocks, rows per block, row blocks: two sums, not deterministic, not pre-zeroed
TABLE = {
    (2, 1, 8): (4, 2, 128, 1, 512, 1),             # one row, 127 idle ty
    (3, 35, 20): (4, 8, 32, 1, 128, 1),            # 3 dead lanes, tail loop only
    (5, 70, 3): (1, 4, 64, 1, 256, 1),             # scalar channels, 1 dead lane
    (4, 521, 4): (4, 1, 256, 1, 1024, 1),          # TX = 1
    (16, 16, 96): (4, 32, 8, 1, 32, 1),            # 8 dead lanes
    (2, 64, 260): (4, 64, 4, 2, 16, 4),            # 2nd channel block: 1 live lane of 64
    (1, 1030, 8): (4, 2, 128, 1, 512, 3),          # last block 6 rows
    (2, 1300, 12): (4, 4, 64, 1, 256, 6),          # last block 20 rows
    (2, 4099, 48): (4, 16, 16, 1, 64, 65),         # last block 3 rows
    (3, 600, 128): (4, 32, 8, 1, 32, 19),          # last block 24 rows
    (1, 9000, 4): (4, 1, 256, 1, 1024, 9),         # last block 808 rows
    (1, 16384, 8): (4, 2, 128, 1, 512, 32),        # full blocks only
}
# (n, s, c) -> (rows form, gx) per sample
ROWS_TABLE = {
    (1, 16384, 4): (1, 16), (1, 16383, 4): (0, 0), (2, 1366, 48): (1, 18), (3, 4096, 20): (1, 20), (1, 16384, 3): (1, 48),
    (2, 1040, 132): (0, 0),                        # q = 33
}


def reduce_plan(n, s, c, nsums, prezeroed=0, det=0):
    """[V, TX, TY, channel blocks, row blocks, rows per block, zero first, workspace floats]"""
    out = (ctypes.c_int * 8)()
    assert lib.cn_nc_reduce_plan(n, s, c, nsums, prezeroed, det, ctypes.byref(out)) == 0
    return list(out)


def rows_plan(G, CG, ny):
    out = (ctypes.c_int * 2)()
    assert lib.cn_nc_rows_plan(G, CG, ny, ctypes.byref(out)) == 0
    return list(out)


@pytest.fixture(scope="module")
def doc():
    return json.load(open(GOLDEN))


def test_the_pinned_reduction_plans(doc):
    assert doc["reduce_fields"] == ["n", "s", "c", "nsums", "det", "V", "TX", "TY", "cblk", "sblk", "rows_per_block", "parts_floats"]
    asked = {tuple(r[:5]) for r in doc["reduce_plans"]}
    for shape in map(tuple, doc["edge_shapes"]):
        assert {shape + (q, det) for q in (2, 3, 4) for det in (0, 1)} <= asked, shape
    assert len(doc["iteration_reduce"]) >= 20
    for r in doc["iteration_reduce"]:
        assert {tuple(r) + (0,), tuple(r) + (1,)} <= asked, r
    for n, s, c, nsums, det, V, TX, TY, cblk, sblk, rpb, parts in doc["reduce_plans"]:
        for prezeroed in (0, 1):
            p = reduce_plan(n, s, c, nsums, prezeroed, det)
            assert p[:6] == [V, TX, TY, cblk, sblk, rpb] and p[7] == parts, (n, s, c, nsums, det, p)


def test_the_recorded_plans_agree_with_the_table_of_edge_shapes(doc):
    assert [tuple(s) for s in doc["edge_shapes"]] == list(TABLE)
    rec = {tuple(r[:5]): r[5:] for r in doc["reduce_plans"]}
    for (n, s, c), (V, TX, TY, cblk, rpb, sblk) in TABLE.items():
        assert rec[(n, s, c, 2, 0)] == [V, TX, TY, cblk, sblk, rpb, 0], (n, s, c)
        assert reduce_plan(n, s, c, 2) == [V, TX, TY, cblk, sblk, rpb, int(sblk > 1), 0], (n, s, c)


def test_the_invariants_of_every_reduction_plan(doc):
    shapes = sorted({tuple(r[:3]) for r in doc["reduce_plans"]})
    multi = 0
    for n, s, c in shapes:
        for nsums in (1, 2, 3, 4):
            for det in (0, 1):
                for prezeroed in (0, 1):
                    V, TX, TY, cblk, sblk, rpb, zero_first, parts = reduce_plan(n, s, c, nsums, prezeroed, det)
                    what = (n, s, c, nsums, det, prezeroed)
                    assert V == (4 if c % 4 == 0 else 1) and TX * TY == 256, what
                    assert cblk * TX >= c // V > (cblk - 1) * TX, what
                    assert sblk * rpb >= s > (sblk - 1) * rpb, what
                    assert rpb >= 4 * TY and 1 <= sblk <= 256, what
                    assert zero_first == int(sblk > 1 and not det and not prezeroed), what
                    assert parts == (nsums * sblk * n * c if det and sblk > 1 else 0) and parts <= DET_WS_FLOATS, what
                    multi += sblk > 1
    assert multi >= 100


def test_the_pinned_rows_plans(doc):
    assert doc["rows_fields"] == ["G", "CG", "ny", "rows_form", "gx"]
    rec = {tuple(r[:3]): r[3:] for r in doc["rows_plans"]}
    assert [tuple(s) for s in doc["rows_shapes"]] == list(ROWS_TABLE)
    for (n, s, c), want in ROWS_TABLE.items():
        CG = c // (4 if c % 4 == 0 else 1)
        assert rec[(s * CG, CG, n)] == list(want), (n, s, c)
        assert (n * s * CG, CG, 1) in rec, (n, s, c)                 # the same shape with per-channel coefficients
    assert len(doc["iteration_rows"]) >= 10 and all(tuple(r) in rec for r in doc["iteration_rows"])
    both = set()
    for (G, CG, ny), want in rec.items():
        form, gx = rows_plan(G, CG, ny)
        assert [form, gx] == want, (G, CG, ny)
        q = CG // math.gcd(CG, 256)
        assert form == int(G >= 16384 and q <= 32), (G, CG, ny)
        if form:
            assert gx >= 1 and gx % q == 0 and gx * ny <= 8192 + q, (G, CG, ny, gx)
        both.add(form)
    assert both == {0, 1}


def test_bad_plan_requests_are_argument_errors():
    out = (ctypes.c_int * 8)()
    for args in ((0, 1, 4, 2), (1, 0, 4, 2), (1, 1, 0, 2), (1, 1, 4, 0), (1, 1, 4, 5)):
        assert lib.cn_nc_reduce_plan(*args, 0, 0, ctypes.byref(out)) == CN_EINVAL, args
    assert lib.cn_nc_reduce_plan(1, 1, 4, 2, 0, 0, None) == CN_EINVAL
    out2 = (ctypes.c_int * 2)()
    for args in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.cn_nc_rows_plan(*args, ctypes.byref(out2)) == CN_EINVAL, args
