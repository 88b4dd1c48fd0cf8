"""Every derived form of a convolution filter, called through `lib` at the smallest shapes that reach each edge
(tests/filter_prep_cases.py: the references, the tables and what each row reaches): cn_conv_weight_tflip, cn_conv_weight_prep_bf16,
cn_conv_wino_filter, cn_conv_wino4_filter, cn_upfold_weights, cn_upfold_wgrad and cn_sumpool2; the upsample-folded layer on the kernel
extents no network has; and the cache that hands the copies out (ops._weight_cache_lookup) on the device.

Every output is a view into a larger allocation, pre-filled with a sentinel, 256 sentinel floats in front of it and behind it.  After a
call the guards are intact, no sentinel is left inside the output and the inputs are unchanged.  The permutations, the bf16 rounding
(compared as bit patterns, on the cast table), F(2x2) on multiples of 4, the class filters, their scatter-back and the sum pool are
compared with torch.equal: tests/test_filter_prep_cases_cpu.py holds (sum of |terms|) 2^k < 2^24 on each of them.

The Winograd transforms on real values are held at
    |got - ref| <= c 2^-24 (|G| |g| |G|^T),      c = 4 for F(2x2), 8 for F(4x4)  (times 1 + 2^-10 for the second-order terms)
c = the roundings one term passes through in the two stages (tests/filter_prep_cases.py: WINO_ROUNDINGS, counted from the statements
of the kernels: per stage the two adds for F(2x2); a rounded constant, its product and two adds for F(4x4)).  The bound is derived, not
tuned; the largest observed error / bound per transform and layout is in profiles/filter_prep_errors.txt, written once at the end of
this file's run when FILTER_PREP_ERRORS names a path."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_edge_cases as C
from tests import filter_prep_cases as FP
from tests.test_conv_edges_gpu import GuardedOut, upfold_layer_exact
from tests.test_ops_gpu import upfold_layer_close
from tests.test_wgrad_edges_gpu import GUARD, UNWRITTEN, Guarded

CN_EINVAL, CN_EUNSUPPORTED = -1, -3
_RATIOS = {}               # (transform, layout) -> (largest error / bound, where)
_RAN = []


def _lib():
    from confignet_amd._lib import lib
    return lib


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i3(v):
    return (ctypes.c_int * 3)(*v)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _written(out, what):
    """guards intact, and no float of the output still holds the sentinel"""
    assert out.intact(), what + ": a guard was written"
    assert not bool((out.view == UNWRITTEN).any()), what + ": part of the output was never written"


def _same(got, want, what):
    assert torch.equal(got, want), "%s: %d of %d elements differ, first at %s" % (
        what, int((got != want).sum()), got.numel(), (got != want).reshape(-1).nonzero()[:4].reshape(-1).tolist())


def test_the_guard_is_the_one_of_the_other_edge_suites():
    g = Guarded(5, UNWRITTEN)
    assert g.buf.numel() == 5 + 2 * GUARD and g.intact() and bool((g.view == UNWRITTEN).all())


# ---- the tap-flipped copy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FP.FLAT_CASES, ids=_ids)
def test_tflip_is_the_reversed_transposed_filter(case):
    t, ci, co = case
    w64 = FP.index_coded(case)
    w, before = _dev(w64), _dev(w64)
    out = GuardedOut((t, co, ci))
    assert _lib().cn_conv_weight_tflip(_p(w), _p(out.out), t, ci, co, _s()) == 0
    _written(out, "tflip %s" % (case,))
    _same(out.out, _dev(FP.tflip(w64)), "tflip %s" % (case,))
    assert torch.equal(w, before)


# ---- the bf16 operand copies ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FP.FLAT_CASES, ids=_ids)
def test_the_bf16_copies_round_to_nearest_even_in_both_layouts(case):
    """both outputs, wf alone, wd alone (the NULL side stays untouched); bit patterns, NaNs included: the kernel's quiet NaN is the
    model's"""
    t, ci, co = case
    u = FP.table_patterns(t, ci, co)
    w = torch.from_numpy(u.view(np.int32)).cuda()
    before = w.clone()
    wf_want, wd_want = (torch.from_numpy(a.view(np.int16)).cuda() for a in FP.prep_bf16(u))
    for use_f, use_d in ((True, True), (True, False), (False, True)):
        what = "bf16 copies of %s, wf %s, wd %s" % (case, use_f, use_d)
        wf, wd = GuardedOut((t, co, ci), torch.bfloat16), GuardedOut((t, ci, co), torch.bfloat16)
        rc = _lib().cn_conv_weight_prep_bf16(_p(w), _p(wf.out) if use_f else None, _p(wd.out) if use_d else None, t, ci, co, _s())
        assert rc == 0, what
        for used, out, want, name in ((use_f, wf, wf_want, "wf"), (use_d, wd, wd_want, "wd")):
            if used:
                _written(out, what)
                _same(out.out.view(torch.int16), want, what + ", " + name)
            else:
                assert out.untouched(), what + ": the absent output was written"
        assert torch.equal(w, before), what
    if t * ci * co >= 327680:                                              # (the whole table, its NaNs included, went through)
        assert bool(((wd_want.int() & 0x7FFF) > 0x7F80).any())


# ---- Winograd ----------------------------------------------------------------------------------------------------------------------------
def _wino_call(m, w, out, ci, co, dgrad):
    fn = _lib().cn_conv_wino_filter if m == 2 else _lib().cn_conv_wino4_filter
    return fn(_p(w), _p(out.out), ci, co, int(dgrad), _s())


def _wino_shape(m, ci, co, dgrad):
    return ((m + 2) ** 2, co, ci) if dgrad else ((m + 2) ** 2, ci, co)


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("pair", FP.WINO_PAIRS + [FP.WINO_CAP_PAIR], ids=_ids)
def test_f2x2_of_multiples_of_four_is_exact(pair, dgrad):
    ci, co = pair
    w64 = FP.small_ints((3, 3, ci, co), FP.flat_seed(ci, co), step=4.0)
    w, before = _dev(w64), _dev(w64)
    out = GuardedOut(_wino_shape(2, ci, co, dgrad))
    assert _wino_call(2, w, out, ci, co, dgrad) == 0
    what = "F(2x2) %s %s" % (pair, "data gradient" if dgrad else "forward")
    _written(out, what)
    _same(out.out, _dev(FP.wino_filter(w64, 2, dgrad)), what)
    assert torch.equal(w, before)


def _note(key, ratio, where):
    if key not in _RATIOS or not ratio <= _RATIOS[key][0]:
        _RATIOS[key] = (ratio, where)


def _within(m, dgrad, w64, got, what, kind):
    """every element within the derived bound; the largest error / bound goes to the record"""
    ref, bound = FP.wino_filter(w64, m, dgrad), FP.wino_bound(w64, m, dgrad)
    err = np.abs(got.double().cpu().numpy() - ref)
    assert np.isfinite(err).all(), what
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    _note(("F(%dx%d)" % (m, m), "data gradient" if dgrad else "forward", kind), ratio, what)
    assert ratio <= 1.0, "%s: error / bound %.3f at %s" % (what, ratio, np.unravel_index(np.argmax(err - bound), err.shape))


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("m", [2, 4])
def test_a_one_hot_filter_fills_one_column_with_two_columns_of_G(m, dgrad):
    """a single 1 at (tap, ci, co), every tap, three channel positions, cin != cout: everything outside column (k, n) = (ci, co) --
    (co, ci) for the data gradient -- is exactly 0, and the planes of the column are the outer product of two columns of G (the
    flipped tap's for the data gradient) within the rounding bound"""
    ci_n, co_n = FP.WINO_ONEHOT_PAIR
    G = FP.WINO[m][0]
    out = GuardedOut(_wino_shape(m, ci_n, co_n, dgrad))
    for a in range(3):
        for b in range(3):
            for ci, co in FP.WINO_ONEHOT_AT:
                what = "F(%dx%d) %s, one-hot at tap (%d, %d) ci %d co %d" % (m, m, "data gradient" if dgrad else "forward", a, b, ci, co)
                w64 = np.zeros((3, 3, ci_n, co_n))
                w64[a, b, ci, co] = 1.0
                out.reset()
                assert _wino_call(m, _dev(w64), out, ci_n, co_n, dgrad) == 0
                _written(out, what)
                got = out.out.clone()
                col = got[:, co, ci].clone() if dgrad else got[:, ci, co].clone()
                if dgrad:
                    got[:, co, ci] = 0.0
                else:
                    got[:, ci, co] = 0.0
                assert not bool(got.any()), what + ": a value outside the column"
                fa, fb = (2 - a, 2 - b) if dgrad else (a, b)
                want = np.outer(G[:, fa], G[:, fb]).reshape(-1)
                bound = FP.WINO_ROUNDINGS[m] * 2.0 ** -24 * FP.WINO_SLACK * np.abs(want)
                err = np.abs(col.double().cpu().numpy() - want)
                assert (err <= bound).all(), what + ": %s" % (err / np.maximum(bound, 1e-300)).max()
                _within(m, dgrad, w64, out.out, what, "one-hot")


@pytest.mark.parametrize("dgrad", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("m,pair", [(m, p) for m in (2, 4) for p in FP.WINO_REAL_PAIRS] + [(4, FP.WINO_CAP_PAIR)], ids=_ids)
def test_the_transform_of_real_filters_stays_within_the_rounding_bound(m, pair, dgrad):
    """standard-normal filters; (4, 1023 x 1026): past the 4096-block cap of cn_conv_wino4_filter, a ragged last block on the second
    trip (F(2x2) past its cap: the exact test above)"""
    ci, co = pair
    w64 = np.random.RandomState(FP.flat_seed(m, ci, co)).standard_normal((3, 3, ci, co)).astype(np.float32).astype(np.float64)
    w, before = _dev(w64), _dev(w64)
    out = GuardedOut(_wino_shape(m, ci, co, dgrad))
    what = "F(%dx%d) %s %s" % (m, m, pair, "data gradient" if dgrad else "forward")
    assert _wino_call(m, w, out, ci, co, dgrad) == 0
    _written(out, what)
    _within(m, dgrad, w64, out.out, what, "normal")
    assert torch.equal(w, before)


# ---- the class filters of an upsample-folded layer and their scatter-back ---------------------------------------------------------------
def _upfold_rows():
    rows = [(nd, ks, tuple(FP.same_pad(k) for k in ks), ci, co) for nd, ks, ci, co in FP.UPFOLD_EXTENTS + FP.UPFOLD_CHANNELS]
    rows += [(nd, ks, pads, 3, 5) for nd, ks, pads in FP.UPFOLD_PADS]
    return rows


def _cap_rows(table):
    return [(nd, ks, tuple(FP.same_pad(k) for k in ks), c, c) for nd, ks, c in table]


@pytest.mark.parametrize("row", _upfold_rows() + _cap_rows(FP.UPFOLD_WEIGHTS_CAP), ids=_ids)
def test_upfold_weights_gives_the_class_sums_in_both_layouts(row):
    """both outputs, wf alone, wd alone; k2_out and pad2_out; the 2-D call passes k3 = (1, kh, kw)"""
    nd, ks, pads, ci, co = row
    w64 = FP.small_ints(tuple(ks) + (ci, co), FP.flat_seed(*ks, ci, co))
    wf64, wd64, k2, pad2 = FP.upfold_weights(w64, pads)
    w, before = _dev(w64), _dev(w64)
    k3, p3 = _i3((1,) * (3 - nd) + tuple(ks)), _i3(FP.pads3_of(nd, pads))
    wf_want, wd_want = _dev(wf64), _dev(wd64)
    for use_f, use_d in ((True, True), (True, False), (False, True)):
        what = "upfold_weights %s, wf %s, wd %s" % (row, use_f, use_d)
        wf, wd = GuardedOut(wf64.shape), GuardedOut(wd64.shape)
        k2_out, p2_out = _i3((-9, -9, -9)), _i3((-9, -9, -9))
        rc = _lib().cn_upfold_weights(_p(w), _p(wf.out) if use_f else None, _p(wd.out) if use_d else None, nd, k3, p3, ci, co, k2_out, p2_out, _s())
        assert rc == 0, what
        assert tuple(k2_out) == (1,) * (3 - nd) + k2 and tuple(p2_out) == (0,) * (3 - nd) + pad2, (what, tuple(k2_out), tuple(p2_out))
        for used, out, want, name in ((use_f, wf, wf_want, "wf"), (use_d, wd, wd_want, "wd")):
            if used:
                _written(out, what)
                _same(out.out, want, what + ", " + name)
            else:
                assert out.untouched(), what + ": the absent output was written"
        assert torch.equal(w, before), what
    # the size outputs are optional
    wd = GuardedOut(wd64.shape)
    assert _lib().cn_upfold_weights(_p(w), None, _p(wd.out), nd, k3, p3, ci, co, None, None, _s()) == 0
    _same(wd.out, wd_want, "upfold_weights %s without size outputs" % (row,))


@pytest.mark.parametrize("row", _upfold_rows() + _cap_rows(FP.UPFOLD_WGRAD_CAP), ids=_ids)
def test_upfold_wgrad_is_the_adjoint_scatter_in_all_three_modes(row):
    """write over the sentinel; atomic add and single-writer add into a tensor of small integers"""
    nd, ks, pads, ci, co = row
    k2 = tuple(FP.upfold_axis(k, p)[1] for k, p in zip(ks, pads))
    g64 = FP.small_ints(k2 + (co, ci), FP.flat_seed(*ks, ci, co) + 1)
    gw64 = FP.upfold_wgrad(g64, ks, pads)
    prior64 = FP.small_ints(gw64.shape, 5, lim=5)
    g2, before = _dev(g64), _dev(g64)
    k3, p3 = _i3((1,) * (3 - nd) + tuple(ks)), _i3(FP.pads3_of(nd, pads))
    out = GuardedOut(gw64.shape)
    for mode, want in ((0, gw64), (1, gw64 + prior64), (2, gw64 + prior64)):
        what = "upfold_wgrad %s mode %d" % (row, mode)
        out.reset()
        if mode:
            out.out.copy_(_dev(prior64))
        assert _lib().cn_upfold_wgrad(_p(g2), _p(out.out), nd, k3, p3, ci, co, mode, _s()) == 0, what
        _written(out, what)
        _same(out.out, _dev(want), what)
        assert torch.equal(g2, before), what


# ---- the sum pool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [FP.F32, FP.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("row", FP.SUMPOOL, ids=_ids)
def test_sumpool2_sums_the_children_and_rounds_once(row, dt):
    nd, n, d, h, w, c = row
    tdt = torch.bfloat16 if dt == FP.BF16 else torch.float32
    gu64 = FP.sumpool_input(row, dt)
    gu = _dev(gu64).to(tdt)
    assert torch.equal(gu.double().cpu(), torch.from_numpy(gu64))
    before = gu.clone()
    want = _dev(FP.sumpool2(gu64, dt)).to(tdt)
    out = GuardedOut(tuple(want.shape), tdt)
    what = "sumpool2 %s %s" % (row, "bf16" if dt else "f32")
    assert _lib().cn_sumpool2(_p(gu), _p(out.out), nd, n, d, h, w, c, dt, _s()) == 0, what
    _written(out, what)
    _same(out.out, want, what)
    assert torch.equal(gu, before), what


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_the_outputs_untouched():
    lib = _lib()
    w = _dev(FP.index_coded((9, 4, 4)))
    out, out2 = GuardedOut((36 * 16,)), GuardedOut((36 * 16,))
    k33, p33 = _i3((1, 3, 3)), _i3((0, 1, 1))
    calls = {
        "tflip taps 0": lambda: lib.cn_conv_weight_tflip(_p(w), _p(out.out), 0, 4, 4, _s()),
        "tflip cin 0": lambda: lib.cn_conv_weight_tflip(_p(w), _p(out.out), 9, 0, 4, _s()),
        "tflip cout 0": lambda: lib.cn_conv_weight_tflip(_p(w), _p(out.out), 9, 4, 0, _s()),
        "tflip w NULL": lambda: lib.cn_conv_weight_tflip(None, _p(out.out), 9, 4, 4, _s()),
        "tflip out NULL": lambda: lib.cn_conv_weight_tflip(_p(w), None, 9, 4, 4, _s()),
        "prep taps 0": lambda: lib.cn_conv_weight_prep_bf16(_p(w), _p(out.out), _p(out2.out), 0, 4, 4, _s()),
        "prep cin 0": lambda: lib.cn_conv_weight_prep_bf16(_p(w), _p(out.out), _p(out2.out), 9, 0, 4, _s()),
        "prep cout 0": lambda: lib.cn_conv_weight_prep_bf16(_p(w), _p(out.out), _p(out2.out), 9, 4, 0, _s()),
        "prep w NULL": lambda: lib.cn_conv_weight_prep_bf16(None, _p(out.out), _p(out2.out), 9, 4, 4, _s()),
        "prep both outputs NULL": lambda: lib.cn_conv_weight_prep_bf16(_p(w), None, None, 9, 4, 4, _s()),
        "sumpool2 c % 4": lambda: lib.cn_sumpool2(_p(w), _p(out.out), 2, 1, 1, 1, 1, 6, FP.F32, _s()),
        "sumpool2 nd 4": lambda: lib.cn_sumpool2(_p(w), _p(out.out), 4, 1, 1, 1, 1, 4, FP.F32, _s()),
        "sumpool2 dtype 2": lambda: lib.cn_sumpool2(_p(w), _p(out.out), 2, 1, 1, 1, 1, 4, 2, _s()),
        "sumpool2 gu NULL": lambda: lib.cn_sumpool2(None, _p(out.out), 2, 1, 1, 1, 1, 4, FP.F32, _s()),
        "sumpool2 gx NULL": lambda: lib.cn_sumpool2(_p(w), None, 2, 1, 1, 1, 1, 4, FP.F32, _s()),
        "upfold_weights nd 4": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 4, k33, p33, 4, 4, None, None, _s()),
        "upfold_weights extent 5": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 2, _i3((1, 5, 3)), p33, 4, 4, None, None, _s()),
        "upfold_weights extent 1 on a used axis": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 2, _i3((1, 1, 3)), p33, 4, 4, None, None, _s()),
        "upfold_weights extent 1 in depth, 3-D": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 3, k33, p33, 4, 4, None, None, _s()),
        "upfold_weights cin 0": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 2, k33, p33, 0, 4, None, None, _s()),
        "upfold_weights cout 0": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 2, k33, p33, 4, 0, None, None, _s()),
        "upfold_weights w NULL": lambda: lib.cn_upfold_weights(None, _p(out.out), _p(out2.out), 2, k33, p33, 4, 4, None, None, _s()),
        "upfold_weights both outputs NULL": lambda: lib.cn_upfold_weights(_p(w), None, None, 2, k33, p33, 4, 4, None, None, _s()),
        "upfold_weights k3 NULL": lambda: lib.cn_upfold_weights(_p(w), _p(out.out), _p(out2.out), 2, None, p33, 4, 4, None, None, _s()),
        "upfold_wgrad nd 4": lambda: lib.cn_upfold_wgrad(_p(w), _p(out.out), 4, k33, p33, 4, 4, 0, _s()),
        "upfold_wgrad extent 5": lambda: lib.cn_upfold_wgrad(_p(w), _p(out.out), 2, _i3((1, 3, 5)), p33, 4, 4, 0, _s()),
        "upfold_wgrad extent 1 on a used axis": lambda: lib.cn_upfold_wgrad(_p(w), _p(out.out), 2, _i3((1, 3, 1)), p33, 4, 4, 0, _s()),
        "upfold_wgrad cin 0": lambda: lib.cn_upfold_wgrad(_p(w), _p(out.out), 2, k33, p33, 0, 4, 0, _s()),
        "upfold_wgrad gw2 NULL": lambda: lib.cn_upfold_wgrad(None, _p(out.out), 2, k33, p33, 4, 4, 0, _s()),
        "upfold_wgrad gw NULL": lambda: lib.cn_upfold_wgrad(_p(w), None, 2, k33, p33, 4, 4, 0, _s()),
        "upfold_wgrad pads NULL": lambda: lib.cn_upfold_wgrad(_p(w), _p(out.out), 2, k33, None, 4, 4, 0, _s()),
    }
    for m, fn in ((2, lib.cn_conv_wino_filter), (4, lib.cn_conv_wino4_filter)):
        for dgrad in (0, 1):
            calls["F(%dx%d) cin 0, dgrad %d" % (m, m, dgrad)] = lambda fn=fn, dgrad=dgrad: fn(_p(w), _p(out.out), 0, 4, dgrad, _s())
            calls["F(%dx%d) cout 0, dgrad %d" % (m, m, dgrad)] = lambda fn=fn, dgrad=dgrad: fn(_p(w), _p(out.out), 4, 0, dgrad, _s())
            calls["F(%dx%d) w NULL, dgrad %d" % (m, m, dgrad)] = lambda fn=fn, dgrad=dgrad: fn(None, _p(out.out), 4, 4, dgrad, _s())
            calls["F(%dx%d) u NULL, dgrad %d" % (m, m, dgrad)] = lambda fn=fn, dgrad=dgrad: fn(_p(w), None, 4, 4, dgrad, _s())
    before = w.clone()
    for what, call in calls.items():
        assert call() == CN_EINVAL, what
        torch.cuda.synchronize()
        assert out.untouched() and out2.untouched(), what + ": an output was written"
    assert torch.equal(w, before)
    assert len(calls) >= 45


# ---- the layer on the extents no network has -------------------------------------------------------------------------------------------
def _folded(case):
    from confignet_amd import ops
    return ops.upfold_class_taps(ops.ConvSpec(case[1], up=1).geom(case[0], case[2])) <= 64


@pytest.mark.parametrize("case", FP.UPFOLD_EXTENT_CASES, ids=lambda c: _ids(c[1]))
def test_the_layer_gives_the_integer_result_on_every_extent(case):
    """F.conv(x, w, b, ConvSpec(k, up=1)) on integers: forward with bias and LeakyReLU, data gradient, filter gradient and bias gradient
    equal the float64 reference.  Extents whose class filters stay within 64 taps run folded; (4,4,4) and (3,3,4) -- 125 and 80 class
    taps, more than the tap mask of the implicit-GEMM gathers holds -- must take the unfolded path, and give the same result there."""
    xs, k, cout = case
    upfold_layer_exact("extent %s" % (k,), (xs, k, cout, 1, 1, None), folded=_folded(case))


@pytest.mark.parametrize("case", FP.UPFOLD_EXTENT_CASES, ids=lambda c: _ids(c[1]))
def test_the_layer_in_bf16_on_every_extent(case):
    """the bf16 body of tests/test_ops_gpu.py: test_upsample_folded_conv_collapsed_per_parity_class at its tolerance"""
    upfold_layer_close(case, "bf16", folded=_folded(case))


def test_what_the_tables_admit_is_what_upfold_ok_admits():
    from confignet_amd import ops
    kept = {k: ops.upfold_ok(ops.ConvSpec(k, up=1).geom((1, 2, 3, 3, 8), 8)) for k in FP.UPFOLD_KS[3]}
    assert {k for k, ok in kept.items() if not ok} == {k for k in FP.UPFOLD_KS[3] if np.prod([e + 1 if e >= 3 else 3 for e in k]) > 64}
    assert all(ops.upfold_ok(ops.ConvSpec(k, up=1).geom((1, 3, 5, 8), 8)) for k in FP.UPFOLD_KS[2])
    assert [_folded(c) for c in FP.UPFOLD_EXTENT_CASES] == [True, True, True, True, True, True, False, False]


# ---- filters of more than 64 taps ------------------------------------------------------------------------------------------------------
LONG = {"vec": ((1, 6, 14, 16), (5, 13), 16, 1, 0, None), "scalar": ((1, 6, 14, 8), (5, 13), 8, 1, 0, None)}      # 65 taps


def test_a_filter_past_64_taps_is_refused_by_the_vectorised_gather_and_exact_on_the_scalar_one():
    """the implicit-GEMM gathers on cin % 16 == 0 (and the bf16 family) walk a 64-bit tap mask: a 65-tap filter is refused there, nothing
    written; the scalar gather (cin = 8) counts reduction elements and gives the integer result"""
    from confignet_amd import ops
    lib = _lib()
    case = LONG["vec"]
    g, inp = C.geom(case), C.integer_inputs(LONG["vec"])
    d = {k: v.float().cuda() for k, v in inp.items()}
    out = GuardedOut(ops.geom_out_shape(g))
    assert lib.cn_conv_fwd(ctypes.byref(g), _p(d["x"]), _p(d["w"]), _p(d["bias"]), _p(out.out), 1, C.SLOPE, _s()) == CN_EUNSUPPORTED
    assert lib.cn_conv_dgrad(ctypes.byref(g), _p(d["gy"]), _p(ops.weight_tflip(d["w"])), _p(out.out), _s()) == CN_EUNSUPPORTED
    assert lib.cn_conv_dgrad_w(ctypes.byref(g), _p(d["gy"]), _p(d["w"]), _p(out.out), _s()) == CN_EUNSUPPORTED
    both = torch.zeros((2, d["w"].numel()), device="cuda", dtype=torch.bfloat16)
    out16 = GuardedOut(ops.geom_out_shape(g), torch.bfloat16)
    assert lib.cn_conv_fwd_bf16(ctypes.byref(g), _p(d["x"].to(torch.bfloat16)), _p(both[0]), _p(d["bias"]), _p(out16.out), 1, C.SLOPE, _s()) == CN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert out.untouched() and out16.untouched()
    case = LONG["scalar"]
    g, inp = C.geom(case), C.integer_inputs(case)
    assert float(C.exact_bound(case, "fwd", inp).max()) < 2 ** 24
    d = {k: v.float().cuda() for k, v in inp.items()}
    out = GuardedOut(ops.geom_out_shape(g))
    assert lib.cn_conv_fwd(ctypes.byref(g), _p(d["x"]), _p(d["w"]), _p(d["bias"]), _p(out.out), 1, C.SLOPE, _s()) == 0
    _written(out, "65 taps, cin 8")
    _same(out.out, C.reference(case, "fwd", inp).float().cuda(), "65 taps, cin 8")


# ---- the cache on the device -----------------------------------------------------------------------------------------------------------
class _Counted:
    def __init__(self, make):
        self.make, self.calls = make, 0

    def __call__(self, w):
        self.calls += 1
        return self.make(w)


def _small_net(seed, trainable=True):
    from confignet_amd import nn
    net = nn.Net()
    net.add_weight("w", np.random.RandomState(seed).randint(-3, 4, (3, 3, 8, 4)).astype(np.float32), trainable=trainable)
    return net.finalize()


def _tflip_of(w):
    return _dev(FP.tflip(w.detach().double().cpu().numpy().reshape(-1, w.shape[-2], w.shape[-1]))).view(w.shape[:-2] + (w.shape[-1], w.shape[-2]))


def test_two_streams_keep_two_live_copies_of_one_filter():
    """forward on A, forward on B, then A, then B: two derivations, not four, and both entries are there afterwards"""
    from confignet_amd import ops
    w = _dev(FP.index_coded((3, 3, 8, 4)))
    make = _Counted(ops.weight_tflip)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    for s in (a, b, a, b):
        with torch.cuda.stream(s):
            got.append(ops._weight_cache_lookup(w, "_cn_tflip", make))
    torch.cuda.synchronize()
    assert make.calls == 2
    assert got[0] is got[2] and got[1] is got[3] and got[0] is not got[1]
    entries = getattr(w, "_cn_tflip")
    assert isinstance(entries, dict) and set(entries) == {a.cuda_stream, b.cuda_stream}
    assert entries[a.cuda_stream][1] is got[0] and entries[b.cuda_stream][1] is got[1]
    for t in got[:2]:
        assert torch.equal(t, _tflip_of(w))
    # a change of the tensor drops BOTH streams' copies
    w.add_(1)
    with torch.cuda.stream(a):
        new = ops._weight_cache_lookup(w, "_cn_tflip", make)
    torch.cuda.synchronize()
    assert make.calls == 3 and set(getattr(w, "_cn_tflip")) == {a.cuda_stream} and torch.equal(new, _tflip_of(w))


def test_an_optimiser_step_rederives_that_networks_copies_and_no_other():
    """ops.adam_step writes the arena through a raw pointer (torch's version counter stands still): Net.mark_updated() is what makes the
    next weight_tflip see the new values, and a second network keeps its copies"""
    from confignet_amd import ops
    net, other = _small_net(1), _small_net(2)
    w, v = net.weights[0], other.weights[0]
    make = _Counted(ops.weight_tflip)
    t0, u0 = ops._weight_cache_lookup(w, "_cn_tflip", make), ops._weight_cache_lookup(v, "_cn_tflip", make)
    assert torch.equal(t0, _tflip_of(w)) and make.calls == 2
    version = w._version
    net.grad_arena.fill_(1.0)
    m, vv = torch.zeros_like(net.arena), torch.zeros_like(net.arena)
    ops.adam_step(net.arena, net.grad_arena, m, vv, None, torch.tensor([0.5], device="cuda"), 0.0, 0.9, 1e-7)
    net.mark_updated()
    torch.cuda.synchronize()
    assert w._version == version                                           # (why the epoch is needed)
    t1 = ops._weight_cache_lookup(w, "_cn_tflip", make)
    assert make.calls == 3 and t1 is not t0
    assert torch.equal(t1, _tflip_of(w)) and not torch.equal(t1, t0)
    assert ops._weight_cache_lookup(w, "_cn_tflip", make) is t1
    assert ops._weight_cache_lookup(v, "_cn_tflip", make) is u0 and make.calls == 3
    assert len(getattr(w, "_cn_tflip")) == 1


def test_a_frozen_networks_copy_is_made_once_and_shared_by_every_stream():
    from confignet_amd import ops
    net = _small_net(3, trainable=False)
    assert net.n_trainable == 0
    w = net.weights[0]
    make = _Counted(ops.weight_tflip)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        first = ops._weight_cache_lookup(w, "_cn_tflip", make)
    with torch.cuda.stream(b):
        second = ops._weight_cache_lookup(w, "_cn_tflip", make)
    third = ops._weight_cache_lookup(w, "_cn_tflip", make)
    torch.cuda.synchronize()
    assert first is second and second is third and make.calls == 1
    assert torch.equal(first, _tflip_of(w))
    net.set_weights([np.ones((3, 3, 8, 4), np.float32)])                     # (bumps the epoch)
    again = ops._weight_cache_lookup(w, "_cn_tflip", make)
    torch.cuda.synchronize()
    assert make.calls == 2 and again is not first and torch.equal(again, _tflip_of(w))


def test_a_frozen_filter_first_used_inside_a_capture_gets_a_graph_private_copy():
    """one single-stream capture: a copy made while capturing lives in that graph's pool and is not remembered; once made eagerly,
    the copy is the one a later capture refers to"""
    from confignet_amd import ops
    net = _small_net(4, trainable=False)
    w = net.weights[0]
    make = _Counted(ops.weight_tflip)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inside = ops._weight_cache_lookup(w, "_cn_tflip", make)
        ops._weight_cache_lookup(w, "_cn_tflip", make)
    assert make.calls == 2 and getattr(w, "_cn_tflip", None) is None
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(inside, _tflip_of(w))
    eager = ops._weight_cache_lookup(w, "_cn_tflip", make)
    assert make.calls == 3 and getattr(w, "_cn_tflip")[1] is eager
    second = torch.cuda.CUDAGraph()
    with torch.cuda.graph(second):
        again = ops._weight_cache_lookup(w, "_cn_tflip", make)
        plus = again + 1.0
    second.replay()
    torch.cuda.synchronize()
    assert again is eager and make.calls == 3 and torch.equal(plus, _tflip_of(w) + 1.0)


# ---- the record ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _ran():
    yield
    _RAN.append(1)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """Once, when the last test of this file has run: the Winograd ratios of THIS process, with the number of test cases that ran in it"""
    yield
    path = os.environ.get("FILTER_PREP_ERRORS")
    if not path or not _RATIOS:
        return
    with open(path, "w") as f:
        f.write("tests/test_filter_prep_gpu.py on one MI355X, written once at the end of the run (FILTER_PREP_ERRORS names the path): what the\n"
                "tests of that one process measured -- %d test cases of the file ran in it.\n\n" % len(_RAN))
        f.write("cn_conv_wino_filter / cn_conv_wino4_filter against the float64 G g G^T.  ratio = the largest |got - ref| / (c 2^-24 (1 + 2^-10)\n"
                "(|G| |g| |G|^T)) over the elements of every launch of the row, c = 4 for F(2x2) and 8 for F(4x4) (the roundings one term passes\n"
                "through in the two stages); one-hot: a single 1 per filter, every tap and three channel positions on 5 x 3 channels; normal:\n"
                "standard-normal filters on %s channels%s.  The tests hold every ratio at <= 1.\n\n"
                % (", ".join("%d x %d" % p for p in FP.WINO_REAL_PAIRS), " (F(4x4): and %d x %d, past the grid cap)" % FP.WINO_CAP_PAIR))
        f.write("%-8s %-14s %-8s %10s   %s\n" % ("kernel", "layout", "filters", "ratio", "largest at"))
        for (k, lay, kind), (r, w) in sorted(_RATIOS.items()):
            f.write("%-8s %-14s %-8s %10.3e   %s\n" % (k, lay, kind, r, w))
