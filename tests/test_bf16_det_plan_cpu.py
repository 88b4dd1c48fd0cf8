"""The plan of the bf16 filter gradient in deterministic mode, checked without a GPU through cn_conv_wgrad_plan (csrc/conv_dispatch.hip:
plan_conv_wgrad, bf16 arm): the launch is the default mode's launch -- route, tile, slices, rows, family, grid, no caller workspace,
zero pass -- and the only thing the mode changes is what FOLLOWS the launch (out[10]): with more than one row slice the slices'
slabs in the stream's deterministic workspace are added in slice order by cn_sum_parts.  Also here: the slabs of today's slice rule
never exceed that workspace, and the order-sensitive inputs of tests/test_bf16_det_wgrad_gpu.py are what they claim to be."""
import json
import os
import random

import pytest
import torch

from confignet_amd._lib import CnConvGeom
from tests import bf16_det_cases as B
from tests import wgrad_edge_cases as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plans.json")
FIELDS = [n for n, _ in CnConvGeom._fields_]
DET_WS_FLOATS = 16 << 20          # csrc/common.h: CN_DET_WS_FLOATS, the deterministic workspace of one stream


def _geometries():
    """(name, geometry): every layer of the golden table, the bf16 entries of the edge table and its two XCD-ordered shapes"""
    out = []
    for e in json.load(open(GOLDEN))["layers"]:
        g = CnConvGeom()
        for name, v in zip(FIELDS, e["g"]):
            setattr(g, name, v)
        out.append((e["name"], g))
    out += [("table " + n, W.geom(W.TABLE[n])) for n in W.BF16_TABLE]
    out += [("xcd %d" % i, W.geom(c)) for i, c in enumerate(W.BF16_XCD)]
    return out


@pytest.fixture(scope="module")
def geoms():
    return _geometries()


def test_the_deterministic_launch_is_the_default_launch(geoms):
    """fields 0 .. 9 (route, tile, slices, rows, family, grid, caller workspace, zero pass) and 11 (stages) do not depend on the mode"""
    taken = 0
    for name, g in geoms:
        (rc0, p0), (rc1, p1) = B.bf16_plan(g, 0), B.bf16_plan(g, 1)
        assert rc0 == rc1 and p0[:10] == p1[:10] and p0[11] == p1[11], (name, p0, p1)
        if p0[0] == B.BF16_ROUTE:
            assert p0[8] == 0 and p0[9] == 1, (name, p0)          # no caller workspace, a zero pass when the target is written
            taken += 1
    assert taken >= 100


def test_the_slab_sum_follows_exactly_the_launches_of_more_than_one_slice(geoms):
    """out[10] = 1 (cn_sum_parts) in deterministic mode where the bf16 kernel runs more than one row slice, 0 everywhere else"""
    summed = single = wide = 0
    for name, g in geoms:
        (_, p0), (_, p1) = B.bf16_plan(g, 0), B.bf16_plan(g, 1)
        assert p0[10] == 0, (name, p0)
        assert p1[10] == (B.SUM_PARTS if p1[0] == B.BF16_ROUTE and p1[2] > 1 else 0), (name, p1)
        if p1[0] == B.BF16_ROUTE:
            summed += p1[2] > 1
            single += p1[2] == 1
            wide += p1[2] >= 64
    # both arms are there, and so is cn_sum_parts' wide scheme (from 64 parts up)
    assert summed >= 50 and single >= 1 and wide >= 1, (summed, single, wide)


def test_the_slabs_of_the_slice_rule_never_exceed_the_stream_workspace(geoms):
    """slices x Ktot x cout <= 2^24 floats over 1 .. 64 taps, 8 .. 2048 channels and 2^8 .. 2^22 rows: the replay of the rule by hand
    (tests/wgrad_edge_cases.py) over the whole sweep, and the plan itself wherever the library takes the geometry (tensors below
    2^31 elements) -- where the two must also agree, so the clamp in bf16_wgrad_slices changed no plan.  A launch of ONE slice writes
    no slab (one writer per element: its filter may be larger than the workspace, as 5 taps x 2048 x 2048 is) and counts as 0."""
    g = CnConvGeom()
    for name in FIELDS:
        setattr(g, name, 1)
    g.nd, g.up = 2, 0
    largest, asked = 0, 0
    for taps, cin, cout, m in B.sweep():
        slices = W.bf16_planned_splits(B.SweepGeom(taps, cin, cout, m))[0]
        floats = slices * taps * cin * cout if slices > 1 else 0
        assert floats <= DET_WS_FLOATS, (taps, cin, cout, m, slices)
        largest = max(largest, floats)
        if m * max(cin, cout) < 2 ** 31 - 1:
            g.n, g.k_w, g.p_w, g.cin, g.cout = m, taps, (taps - 1) // 2, cin, cout
            rc, p = B.bf16_plan(g, 1)
            assert rc == 0 and p[0] == B.BF16_ROUTE and p[2] == slices, (taps, cin, cout, m, slices, p)
            asked += 1
    assert largest == 12582912          # (1 x 1, 128 -> 96 channels, 2^20 rows: 1024 slices, 0.75 of the workspace)
    assert asked >= 300000
    for name, gg in geoms:
        rc, p = B.bf16_plan(gg, 1)
        if p[0] == B.BF16_ROUTE and p[2] > 1:
            assert p[2] * W.ktot(gg) * gg.cout <= DET_WS_FLOATS, (name, p)


@pytest.mark.parametrize("case", W.BF16_XCD, ids=["16-slices", "22-slices"])
def test_the_order_sensitive_inputs_are_order_sensitive(case):
    """A check of the GPU test's inputs, not of the product: the fp32 sum of the slice partials in slice order differs from the sum
    in reversed order, and from each of twenty random orders, in at least a tenth of the filter elements."""
    rows, slices = B.rows_and_slices(case)
    assert (rows, slices) == ((256, 16) if case[0][0] == 16 else (288, 22))
    x, gy = B.order_inputs(case)
    parts = B.slice_partials(x, gy, case)
    assert torch.equal(sum(parts), W.reference(x, gy, case))          # (float64: exact)
    in_order = B.emulate(parts, range(slices))
    assert not torch.equal(in_order.double(), sum(parts))              # the fp32 sum does round
    rev = B.fraction_different(in_order, B.emulate(parts, reversed(range(slices))))
    print("%d slices: reversed order differs in %.0f %% of the elements" % (slices, 100 * rev))
    assert rev >= 0.1, rev
    rnd = random.Random(7)
    for _ in range(20):
        order = list(range(slices))
        rnd.shuffle(order)
        if order != list(range(slices)):
            f = B.fraction_different(in_order, B.emulate(parts, order))
            assert f >= 0.1, (order, f)
    prior = B.order_prior(in_order.shape)
    assert B.fraction_different(B.emulate(parts, range(slices), prior), B.emulate(parts, reversed(range(slices)), prior)) >= 0.1
