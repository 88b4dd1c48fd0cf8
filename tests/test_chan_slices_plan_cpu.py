"""How the two per-channel training reductions (cn_dwconv3x3_wgrad, cn_bn_train_bwd_reduce) slice their rows, checked without a GPU
through cn_chan_slices_plan (csrc/chan_slices.h: chan_slices_plan is the function both calls decide with).
tests/golden/chan_slices_plans.json holds RECORDED plans: what the two functions that csrc/depthwise.hip and csrc/bn_train.hip each
carried before give, as tests/chan_slices_cases.py transcribes them -- never generated from the function it pins.  The shapes are
every depthwise and BatchNormalization layer of MobileNetV2 at 256 x 256 (batch 32 and 1), the shapes of the two GPU edge-test
files, and both sides of every boundary of the rule."""
import ctypes
import json

import pytest

from confignet_amd._lib import lib
from tests import chan_slices_cases as C

CN_EINVAL = -1


def report(rows, c, min_rows):
    """[TX, TY, channel blocks, slices, rows per slice]"""
    out = (ctypes.c_int * 5)()
    assert lib.cn_chan_slices_plan(rows, c, min_rows, ctypes.byref(out)) == 0, (rows, c, min_rows)
    return list(out)


@pytest.fixture(scope="module")
def doc():
    return json.load(open(C.GOLDEN))


def test_the_recorded_plans(doc):
    assert doc["fields"] == C.FIELDS
    asked = {tuple(r[:3]) for r in doc["plans"]}
    assert len(asked) == len(doc["plans"])
    dw, bn = [tuple(s) for s in doc["dw_layers"]], [tuple(s) for s in doc["bn_layers"]]
    assert dw[-2 * len(C.DW_EDGE_SHAPES):] == [s + (stride,) for s in C.DW_EDGE_SHAPES for stride in (1, 2)]
    assert bn[-len(C.BN_REDUCE_SHAPES):] == C.BN_REDUCE_SHAPES
    assert len(dw) - 2 * len(C.DW_EDGE_SHAPES) == 2 * 17 and len(bn) - len(C.BN_REDUCE_SHAPES) == 2 * 52     # the network, at two batch sizes
    assert set(C.golden_requests(dw, bn)) == asked
    for r in doc["plans"]:
        assert report(*r[:3]) == r[3:], r


def test_the_report_is_the_transcription_around_every_recorded_shape(doc):
    seen = set()
    for rows, c, min_rows in (r[:3] for r in doc["plans"]):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                q = (rows + dr, c + dc, min_rows)
                if q[0] > 0 and q[1] > 0 and q not in seen:
                    seen.add(q)
                    assert report(*q) == C.transcribed_plan(*q), q
    assert len(seen) > 4 * len(doc["plans"])


def test_the_invariants_of_every_plan(doc):
    sliced = capped = 0
    for rows, c, min_rows in (r[:3] for r in doc["plans"]):
        TX, TY, cb, slices, per_slice = report(rows, c, min_rows)
        cgs, what = C.cgs_of(c), (rows, c, min_rows)
        assert TX * TY == 256 and TX <= 64 and TX & (TX - 1) == 0, what
        assert cb * TX >= cgs > (cb - 1) * TX, what
        assert (slices - 1) * per_slice < rows <= slices * per_slice, what
        assert slices * cb <= max(1024, cb), what
        sliced += slices > 1
        capped += rows > max(1024 // cb, 1) * max(4 * TY, min_rows)         # more rows than the cap's slices hold at the floor
    assert sliced >= 100 and capped >= 20


def test_the_splits_the_design_notes_quote():
    # batch 32, stride 1: 25 slices for the 7 x 7 x 960 layer (1568 pixels / 64, evened out to 63 per slice), 1024 of 512 for 128 x 128 x 32
    assert report(32 * 7 * 7, 960, C.DW_MIN_ROWS) == [64, 4, 4, 25, 63]
    assert report(32 * 128 * 128, 32, C.DW_MIN_ROWS) == [8, 32, 1, 1024, 512]
    assert lib.cn_dwconv3x3_wgrad_slices(32, 7, 7, 960, 1) == 25 and lib.cn_dwconv3x3_wgrad_slices(32, 128, 128, 32, 1) == 1024


def test_the_slices_entries_are_the_report(doc):
    for s in map(tuple, doc["dw_layers"]):
        assert lib.cn_dwconv3x3_wgrad_slices(*s) == report(C.dw_pixels(*s), s[3], C.DW_MIN_ROWS)[3], s
    for m, c in doc["bn_layers"]:
        assert lib.cn_bn_train_bwd_slices(m, c) == report(m, c, C.BN_MIN_ROWS)[3], (m, c)
    for rows, c, min_rows in (r[:3] for r in doc["plans"]):          # (the boundary requests as calls: n = rows pixels of 1 x 1)
        got = lib.cn_dwconv3x3_wgrad_slices(rows, 1, 1, c, 1) if min_rows == C.DW_MIN_ROWS else lib.cn_bn_train_bwd_slices(rows, c)
        assert got == report(rows, c, min_rows)[3], (rows, c, min_rows)


def test_bad_plan_requests_are_argument_errors():
    out = (ctypes.c_int * 5)()
    for args in ((0, 4, 0), (1, 0, 0), (1, 4, -1)):
        assert lib.cn_chan_slices_plan(*args, ctypes.byref(out)) == CN_EINVAL, args
    assert lib.cn_chan_slices_plan(1, 4, 0, None) == CN_EINVAL
    assert lib.cn_chan_slices_plan(1 << 42, 4, 0, ctypes.byref(out)) == CN_EINVAL       # 2^32 rows per slice: more than the report's int
