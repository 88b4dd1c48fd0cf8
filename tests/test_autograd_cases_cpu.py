"""The reference side of the autograd-layer tests (tests/autograd_cases.py), on the CPU: the float64 statements against finite
differences (so the reference itself is pinned, as tests/test_norm_tail_reference_cpu.py does for the tangent tail), the exactness
and margin preconditions of every exact case at every order the GPU test asks for, and the completeness of the table."""
import functools

import pytest
import torch

from confignet_amd import ops
from tests import autograd_cases as A
from tests import conv_edge_cases as CE


def _own_statement(name):
    """conv2:* and conv3:* differentiate the statement of conv:<geometry>:none further: one finite-difference check serves them"""
    return not name.startswith(("conv2:", "conv3:"))


CHECKED = [n for n in A.TABLE if _own_statement(n) and A.TABLE[n].values]


@functools.lru_cache(maxsize=None)
def _reference(name):
    return A.reference(A.TABLE[name])


@pytest.mark.parametrize("name", CHECKED)
def test_statement_against_finite_differences(name):
    case = A.TABLE[name]
    t = A.inputs_as(case, torch.float64)
    leaves = [t[k].clone().requires_grad_(True) for k in case.diff]

    def fn(*vals):
        tt = dict(t)
        tt.update(zip(case.diff, vals))
        ys = case.statement(tt)
        return tuple(y for y in ys if y is not None)
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)
    if case.order >= 2 or case.guard == "either":
        assert torch.autograd.gradgradcheck(fn, leaves, eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


@pytest.mark.parametrize("name", A.EXACT)
def test_exact_cases_stay_exact_in_fp32(name):
    """every partial sum, at every order the GPU test asks for, is a multiple of the case's unit below 2^24 units"""
    case = A.TABLE[name]
    bound = A.absolute_bound(case)
    assert bound / case.unit < 2 ** 24, (name, bound, case.unit)
    ref = _reference(name)
    for k, v in ref.items():
        if v is None:
            continue
        q = v / case.unit
        assert bool((q == q.round()).all()), (name, k, "not a multiple of the unit %g" % case.unit)
        assert float(v.abs().max()) <= bound, (name, k, "above the bound of the absolute statement")
        assert bool((v.float().double() == v).all()), (name, k)


@pytest.mark.parametrize("name", [n for n in A.EXACT if A.TABLE[n].pre is not None or A.TABLE[n].pools is not None])
def test_no_branch_decision_is_near(name):
    case = A.TABLE[name]
    t = A.inputs_as(case, torch.float64)
    for v in (case.pre(t) if case.pre is not None else []):
        assert float(v.abs().min()) >= 1.0, (name, float(v.abs().min()))
    for x, k, s, pad in (case.pools(t) if case.pools is not None else []):
        assert not A.pool_has_tie(x, k, s, pad), name


def test_every_function_class_is_in_the_table():
    defined, listed = A.function_classes(), A.classes_in_table()
    assert len(defined) >= 30, sorted(defined)                  # 29 in functional.py and GlobalBatchMoments in losses.py today
    assert defined <= listed, sorted(defined - listed)
    assert listed <= defined, sorted(listed - defined)          # (a renamed class must not leave a dead row)
    for cls in A.HELD:
        assert cls in defined


def test_raw_kernel_backwards_are_all_guarded_cases():
    """every Function whose backward calls a kernel directly has a case that differentiates its gradient again"""
    guarded = set()
    for name in A.GUARDED:
        guarded.update(A.TABLE[name].classes)
    for cls in A.RAW_BACKWARD + ("AdaInFn", "LinearActFn", "MlpBankFn", "DiscrTailFn", "ChannelAffineActFn", "ConvFn"):
        assert cls in guarded, cls


@pytest.mark.parametrize("name", A.CONV_GEOMS)
def test_convolution_geometries_stay_off_winograd(name):
    """F(4x4) is not exact and F(2x2) only with filters that are multiples of 4: no geometry of the table takes either, forward or
    data gradient; f and g are the ones the collapsed upsample form takes."""
    case = CE.TABLE[name]
    g = CE.geom(case)
    for cin, cout in ((g.cin, g.cout), (g.cout, g.cin)):
        assert not ops._wino4_ok(g, cin, cout) and not ops._wino_ok(g, cin, cout)
    assert ops.upfold_ok(g) == (name in ("f", "g"))


@pytest.mark.parametrize("kernel,folded", [((3, 3, 3), True), ((2, 3, 4), True), ((3, 3, 4), False), ((4, 4, 4), False)])
def test_upfold_ok_stops_where_the_class_filters_pass_64_taps(kernel, folded):
    """f's geometry with other 3-D extents: 4 x 4 x 4 = 64 and 3 x 4 x 5 = 60 class taps are taken, 4 x 4 x 5 = 80 and 5 x 5 x 5 = 125
    are not (the implicit-GEMM gathers hold the live taps of a tile in a 64-bit mask) and run unfolded"""
    xs, _, cout, stride, up, epad = CE.TABLE["f"]
    assert ops.upfold_ok(CE.geom((xs, kernel, cout, stride, up, epad))) == folded


def test_the_comparison_notices_a_cut_graph_and_a_swapped_operand():
    """the instrument itself: a statement whose first gradient is detached before the second level, and a transposed operand"""
    case = A.TABLE["sqdiff_sum"]
    ref = _reference("sqdiff_sum")
    assert A.compare(case, ref, ref) == []
    cut = dict(ref)
    cut["d2/a"], cut["d2/c0"] = None, torch.zeros_like(ref["d2/c0"])
    fails = A.compare(case, cut, ref)
    assert len(fails) == 2 and "absent" in fails[0], fails
    case = A.TABLE["matmul:11"]
    ref = _reference("matmul:11")
    wrong = dict(ref)
    wrong["d1/a"] = ref["d1/a"].t().contiguous().reshape(ref["d1/a"].shape)
    assert any(f.startswith("d1/a") for f in A.compare(case, wrong, ref))


def test_real_cases_have_a_yardstick_for_every_quantity():
    for name in A.REAL:
        case = A.TABLE[name]
        if not case.values:
            continue
        ref, yard = A.yardstick(case)
        for k, v in ref.items():
            if not A.is_zero(v):
                assert 0.0 < yard[k] < 1e-4, (name, k, yard[k])
