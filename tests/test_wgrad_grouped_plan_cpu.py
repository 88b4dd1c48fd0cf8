"""The plan of the grouped filter gradient (csrc/conv_dispatch.hip: plan_conv_wgrad_group, reported by cn_conv_wgrad_grouped_plan
without a device): pinned for the ResNet-50 trunk's 52 deferred layers at n = 8 and n = 16 (tests/golden/wgrad_grouped_plan.json, 256
CUs), and for every list -- the trunk's and those of the GPU test -- the properties a launch depends on."""
import json
import os

import pytest

from tests import wgrad_edge_cases as W
from tests import wgrad_grouped_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_grouped_plan.json")


def _lists():
    out = {"trunk-n%d" % n: [g for _, g in C.trunk_jobs(n)] for n in (8, 16)}
    out.update({name: [W.geom(c) for c, _ in lst] for name, lst in C.LISTS.items()})
    return out


@pytest.mark.parametrize("n", [8, 16])
def test_the_trunk_plan_is_the_committed_one(n):
    jobs = C.trunk_jobs(n)
    assert len(jobs) == 52
    plan, info = C.plan([g for _, g in jobs])
    want = json.load(open(GOLDEN))[str(n)]
    assert list(info) == want["info"]
    got = [[name] + [q[f] for f in C.FIELDS] for (name, _), q in zip(jobs, plan)]
    for a, b in zip(got, want["jobs"]):
        assert a == b, "plan of %s: %s, committed %s (fields: %s)" % (a[0], a[1:], b[1:], ", ".join(C.FIELDS))
    # what the rule is for: a handful of launches, most layers unsplit or in a few slices
    assert info[0] <= 5
    assert sum(1 for q in plan if q["slices"] <= 8) >= 40


@pytest.mark.parametrize("name", list(_lists()))
@pytest.mark.parametrize("solo", [False, True])
def test_every_launch_of_a_plan_is_sound(name, solo):
    geoms = _lists()[name]
    plan, (launches, most, arg_bytes, block_bytes) = C.plan(geoms, solo)
    assert arg_bytes <= block_bytes, "a launch's job struct exceeds the argument block"
    assert launches >= 1 and {q["launch"] for q in plan} == set(range(launches))
    for g, q in zip(geoms, plan):
        bi, bn, kb = C.TILE[q["tile"]]
        m, count = C.rows_of(g), C.ktot(g) * g.cout
        assert q["stages"] == (3 if q["tile"] == 3 else 4)
        assert (q["tiles_x"], q["tiles_y"]) == (-(-C.ktot(g) // bi), -(-g.cout // bn))
        # slices x rows cover M, no slice is empty, a slice is whole K steps
        assert q["rows"] % kb == 0 and q["slices"] >= 1
        assert q["slices"] * q["rows"] >= m > (q["slices"] - 1) * q["rows"], (name, q, m)
        padded = -(-q["slices"] // 8) * 8 if q["slices"] >= 8 else q["slices"]
        assert q["wgs"] == padded * q["tiles_x"] * q["tiles_y"]
        assert q["ws_floats"] == (q["slices"] * count if q["slices"] > 1 else 0)
    for l in range(launches):
        js = sorted((q for q in plan if q["launch"] == l), key=lambda q: q["first_wg"])
        assert 1 <= len(js) <= most, "launch %d holds %d jobs" % (l, len(js))
        assert len({(q["tile"], q["stages"]) for q in js}) == 1, "launch %d mixes tile configurations" % l
        nxt = 0
        for q in js:                      # the workgroup ranges tile [0, grid) without gap or overlap
            assert q["first_wg"] == nxt, "launch %d: a job starts at %d, the one before ends at %d" % (l, q["first_wg"], nxt)
            nxt += q["wgs"]
        assert 0 < nxt < 2 ** 31


def test_a_job_planned_alone_has_the_plan_of_the_single_launch():
    """solo: tile, slices and rows of cn_conv_wgrad_plan for the entry cn_conv_wgrad_ws_slabs (routes 4 | 8 | 16, slabs left to the caller)"""
    import ctypes
    from confignet_amd._lib import lib
    for name, geoms in _lists().items():
        plan, _ = C.plan(geoms, solo=True)
        for g, q in zip(geoms, plan):
            out = (ctypes.c_longlong * 12)()
            assert lib.cn_conv_wgrad_plan(ctypes.byref(g), 0, 0, 1, 4 | 8 | 16, 0, out) == 0 and out[0] == 3
            assert (q["tile"], q["slices"], q["rows"], q["wgs"]) == (out[1], out[2], out[3], out[5]), (name, q, list(out))


def test_the_gpu_lists_cover_every_way_a_job_can_lie_in_a_launch():
    plans = {name: C.plan([W.geom(c) for c, _ in lst]) for name, lst in C.LISTS.items()}
    shares, info = plans["shares"]
    assert info[0] == 1, "the shares list is ONE launch"
    slices = sorted(q["slices"] for q in shares)
    assert slices[0] == 1 and any(2 <= s < 8 for s in slices) and any(s >= 8 and s % 8 == 0 for s in slices)
    padded = [q for q in shares if q["slices"] >= 8 and q["slices"] % 8]
    assert padded and any(o["first_wg"] > p["first_wg"] for p in padded for o in shares), "padded ids inside the grid, not at its end"
    mixed, info = plans["mixed"]
    assert len({q["tile"] for q in mixed}) >= 2 and info[0] >= 2                      # two tile configurations -> more than one launch
    assert any(q["slices"] > 1 for q in mixed) and any(q["slices"] == 1 for q in mixed)
    assert len(C.LISTS["thirty"]) == 30 > plans["thirty"][1][1] and plans["thirty"][1][0] == 2
    assert len(C.LISTS["one"]) == 1 and plans["one"][1][0] == 1
    assert {acc for lst in C.LISTS.values() for _, acc in lst} == {0, 1}
    # Ktot and cout that are no multiples of the tile
    assert any(C.ktot(W.geom(c)) == 144 and W.geom(c).cout == 96 for c, _ in C.LISTS["mixed"])


def test_a_job_the_kernel_does_not_take_is_refused():
    from confignet_amd import ops
    from confignet_amd.dnn_models.real_encoder import C7
    with pytest.raises(Exception, match="does not take"):
        ops.conv_wgrad_grouped_plan([C7.geom((8, 256, 256, 3), 64)])
