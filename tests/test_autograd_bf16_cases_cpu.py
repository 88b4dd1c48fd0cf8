"""The preconditions of the bf16 autograd table (tests/autograd_bf16_cases.py), on the CPU: every case's inputs are stored exactly in
bf16, no branch decision is near, nothing the product may store in bf16 leaves 256 units and nothing else 2^24, the float64
reference survives the storage types it is compared in and is not trivially zero, and the table is complete.  With these,
tests/test_autograd_bf16_gpu.py compares by torch.equal."""
import os

import pytest
import torch

from confignet_amd import ops
from tests import autograd_bf16_cases as B
from tests import autograd_cases as A
from tests import conv_edge_cases as CE

BF16 = torch.bfloat16
NAMES = list(B.TABLE)


def _through_bf16(v):
    return v.to(torch.float32).to(BF16).to(torch.float64)


def _activation_bound(case, storage=None, absolute=None):
    """(largest activation-typed quantity, largest quantity) of the ladder on absolute values"""
    storage = B.quantity_storage(case) if storage is None else storage
    absolute = A.absolute_ladder(case) if absolute is None else absolute
    act = [float(v.max()) for k, v in absolute.items() if v is not None and v.numel() and storage[k] == BF16]
    if case.quad:
        # RowScaleFn's 2 * g, stored in the type of the first gradient g it scales, never a quantity of the ladder
        act += [2.0 * float(v.max()) for k, v in absolute.items() if k.startswith("d1/") and v is not None and storage[k] == BF16]
    return max(act + [0.0]), max([float(v.max()) for v in absolute.values() if v is not None and v.numel()] + [0.0])


def _nonzero_fractions(case, ref):
    return {k: float((v != 0).double().mean()) for k, v in ref.items() if k.startswith("d1/") and v is not None}


def _violations(case, ref=None):
    """every way the case misses the condition (strings); ref: the quantities to judge instead of the case's own reference"""
    out = []
    act, every = _activation_bound(case)
    if not act <= B.STEPS * case.unit:
        out.append("an activation-typed quantity reaches %g > 256 * %g under the absolute ladder" % (act, case.unit))
    if not every < 2 ** 24 * case.unit:
        out.append("a quantity reaches %g >= 2^24 * %g" % (every, case.unit))
    fr = _nonzero_fractions(case, B.reference(case) if ref is None else ref)
    if not fr:
        out.append("no first gradient at all")
    out += ["%s: %.2f of its entries nonzero, under a quarter" % (k, f) for k, f in fr.items() if f < 0.25]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_condition_holds(name):
    case = B.TABLE[name]
    assert _violations(case) == [], name
    storage, ref = B.quantity_storage(case), B.reference(case)
    assert set(storage.values()) <= {BF16, torch.float32}
    for k, v in case.inputs().items():
        if v.dtype != torch.uint8:
            assert torch.equal(_through_bf16(v), v), (name, k, "an input bf16 does not hold")
    for k, v in ref.items():
        if v is None:
            continue
        q = v / case.unit
        assert bool((q == q.round()).all()), (name, k, "not a multiple of the unit %g" % case.unit)
        assert torch.equal(v.to(torch.float32).double(), v), (name, k)
        if storage[k] == BF16:
            assert torch.equal(_through_bf16(v), v), (name, k, "the reference itself does not survive bf16 storage")


@pytest.mark.parametrize("name", [n for n in NAMES if B.TABLE[n].pre is not None or B.TABLE[n].pools is not None])
def test_no_branch_decision_is_near_with_the_sparse_draw(name):
    case = B.TABLE[name]
    t = A.inputs_as(case, torch.float64)
    for v in (case.pre(t) if case.pre is not None else []):
        assert float(v.abs().min()) >= 1.0, (name, float(v.abs().min()))
    for x, k, s, pad in (case.pools(t) if case.pools is not None else []):
        assert not A.pool_has_tie(x, k, s, pad), name
        assert float(x.abs().max()) <= B.STEPS


def test_the_sparse_draw_keeps_the_conventions_and_the_density():
    v = A.ints("probe", (64, 64), lim=3, sparse=(0.125, 1))
    assert set(v.unique().tolist()) == {-1.0, 0.0, 1.0} and 0.09 < float((v != 0).double().mean()) < 0.16
    assert not bool((A.ints("probe", (64, 64), lim=3, nonzero=True, sparse=(0.125, 1)) == 0).any())
    assert bool((A.ints("probe", (64, 64), lim=3, even=True, sparse=(0.5, 3)) % 2 == 0).all())
    assert bool((A.ints("probe", (64, 64), lim=3, odd=True, sparse=(0.5, 3)) % 2 == 1).all())
    assert torch.equal(A.ints("probe", (5, 7)), A.ints("probe", (5, 7)))                      # the dense draw is what it was
    assert A.ints("probe", (64, 64), lim=3).abs().max() == 3 and A._SPARSE is None
    case = B.TABLE["conv:c:lrelu"]
    t = case.inputs()
    assert bool((t["w"] % 2 == 0).all()) and bool((t["bias"] % 2 == 1).all()) and float(t["w"].abs().max()) == 2.0
    assert abs(float((t["x"] != 0).double().mean()) - case.density) < 0.03


def test_the_condition_notices_a_raised_density_and_zeroed_cotangents():
    """the instrument: the same case at twice .. eight times its density leaves 256 units; with its cotangents zeroed the
    reference has no nonzero first gradient"""
    case = B.TABLE["conv:c:lrelu"]
    dense = B.view(case.base, 8 * case.density, 1)
    assert any("256" in v for v in _violations(dense)), _violations(dense)
    zeroed = {k: (torch.zeros_like(v) if (k.startswith("d") and v is not None) else v) for k, v in B.reference(case).items()}
    assert len([v for v in _violations(case, zeroed) if "under a quarter" in v]) == 3
    r1 = B.TABLE["conv2:e3s2:gx:quad:igo"]
    assert any("256" in v for v in _violations(B.view(r1.base, 2 * r1.density, 1, order=2)))


def test_roles_and_storage_come_from_the_predicates():
    st = B.input_storage(B.TABLE["conv:c:none"])
    assert st == {"x": BF16, "w": torch.float32, "bias": torch.float32}
    assert B.input_storage(B.TABLE["conv:e3s2:none"])["x"] == torch.float32            # the image: 3 channels
    assert B.expected_storage(B.TABLE["conv:e3s2:none"]) == (BF16,) and B.expected_storage(B.TABLE["conv:k3:relu"]) == (torch.float32,)
    assert B.expected_storage(B.TABLE["conv_dgrad:up2k4"]) == (BF16,) and B.expected_storage(B.TABLE["conv_wgrad:a"]) == (torch.float32,)
    assert B.input_storage(B.TABLE["linear:bias"]) == {"x": BF16, "w": torch.float32, "b": torch.float32}
    assert set(B.input_storage(B.TABLE["mlp_bank:all"]).values()) == {torch.float32}
    assert B.expected_storage(B.TABLE["nc_lin:c8:nc:b"]) == (BF16,) and B.expected_storage(B.TABLE["chan_affine3:210"]) == (torch.float32,)
    assert ops.ACT_DTYPE == torch.float32                                                     # (bf16_mode restores what it found)
    for name in NAMES:
        case = B.TABLE[name]
        assert set(B.roles(case)) == set(case.inputs()) and set(case.diff) <= set(case.inputs())
        # what the storage rule says with the threshold moved is another answer wherever an activation has 5 .. 8 channels
        for k, v in case.inputs().items():
            if B.roles(case)[k] == "activation" and v.dtype != torch.uint8:
                assert B.input_storage(case)[k] == (BF16 if v.shape[-1] > 4 else torch.float32)


def test_every_storage_arm_of_the_convolutions_is_reached():
    """the geometries are in the arm they are listed under, by the predicates of ops.py in bf16 mode"""
    with B.bf16_mode():
        for arm, names in B.CONV_ARMS.items():
            for n in names:
                g = CE.geom(B.GEOMS[n])
                got = ("bf16 family" if ops._bf16_conv_ok(g) else "image layer" if g.cin == 3 else
                       "thin output" if ops._act_out_dtype(g.cout) == torch.float32 else "fp32 family, cast on each side")
                assert got == arm, (n, got, arm)
        cast = [CE.geom(B.GEOMS[n]) for n in B.CONV_ARMS["fp32 family, cast on each side"]]
        assert any(g.cout % 8 and not g.cin % 8 for g in cast) and any(g.cin % 8 for g in cast)
        assert {ops.upfold_ok(CE.geom(B.GEOMS[n])) for n in ("f", "g")} == {True} and CE.geom(B.GEOMS["f"]).nd == 3
        assert B.GEOMS["up2k4"][4] == 1 and not ops.upfold_ok(CE.geom(B.GEOMS["up2k4"]))      # ConvDgradFn with sumpool2
    keep = (ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS)
    ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS = 0, 0.0, 0
    try:
        g2, g4 = CE.geom(B.GEOMS["w2"]), CE.geom(B.GEOMS["w4"])
        for cin, cout in ((16, 64), (64, 16)):
            assert (ops._wino_ok(g2, cin, cout) and not ops._wino4_ok(g2, cin, cout)) == (cout == 64)
            assert ops._wino4_ok(g4, cin, cout) == (cout == 64)
    finally:
        ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS = keep
    assert len(B.R1) >= 3 and {B.arm_of(n) for n in B.R1} >= {"bf16 family", "fp32 family, cast on each side", "image layer"}
    for n in B.R1:
        assert B.TABLE[n].density >= 1 / 16 and B.TABLE[n].order == 2 and B.TABLE[n].quad and B.TABLE[n].igo


def test_expected_families_follow_the_predicates_and_the_plans():
    fam = {n: B.expected_families(B.TABLE[n]) for n in B.CONV}
    for n, f in fam.items():
        arm = B.arm_of(n)
        if arm == "bf16 family":
            assert f == {"fwd": "igemm_bf16", "dgrad": "igemm_bf16", "wgrad": "igemm_bf16_wgrad"}, (n, f)
        else:
            assert "igemm_bf16" not in f.values() and "wino_fwd" not in f.values(), (n, f)
            assert any(v is not None for v in f.values()), (n, f)       # (the thin kernels are outside the profiled families)
    # the image layers' own kernels report the family of the fp32 kernels they stand in for: the conversions tell the arms apart
    casts = {n: B.expected_casts(B.TABLE[n]) for n in B.CONV}
    assert all(casts[n] == {"fwd": 0, "dgrad": 0} for n in B.CONV if B.arm_of(n) == "bf16 family")
    assert casts["conv:a:none"] == {"fwd": 2, "dgrad": 2} and casts["conv:k3:none"] == {"fwd": 1, "dgrad": 1}
    assert casts["conv:e3s2:none"] == {"fwd": 0, "dgrad": 0}
    assert casts["conv:e3s1:none"] == casts["conv:e7:none"] == {"fwd": 0, "dgrad": 1}        # cn_conv_dgrad_dt refuses them: the fallback
    assert ops.MIXED_FIRST_LAYERS                           # (the setting the expectations are written for)
    for n in B.CONV:
        if B.arm_of(n) == "image layer":
            assert B.expected_casts(B.TABLE[n], mixed=False) == {"fwd": 1, "dgrad": 1}, n


@pytest.mark.parametrize("geom", B.RES_GEOMS)
def test_the_residual_forms_meet_the_condition(geom):
    case, inp = B.GEOMS[geom], B.res_inputs(geom)
    g = CE.geom(case)
    assert g.s_h == 1 and g.up == 0 and B.act_dtype(g.cin) == BF16 and B.act_dtype(g.cout) == BF16
    for request in ("res", "dgrad_w_res"):
        assert float(CE.exact_bound(case, request, inp).max()) <= B.STEPS, (geom, request)
        ref = CE.reference(case, request, inp)
        assert torch.equal(_through_bf16(ref), ref) and float((ref != 0).double().mean()) >= 0.25, (geom, request)
    assert all(torch.equal(_through_bf16(v), v) for v in inp.values())


def test_every_function_class_is_in_the_table_or_held():
    defined, covered = B.bf16_reachable_classes(), B.classes_covered()
    assert len(defined) >= 30
    assert defined <= covered, sorted(defined - covered)
    assert covered <= defined, sorted(covered - defined)
    tabled = set()
    for c in B.TABLE.values():
        tabled.update(c.classes)
    for cls, where in B.HELD.items():
        assert cls not in tabled, (cls, "is in the table: no longer held elsewhere")
        path = where.split(" ")[0]
        assert path.startswith("tests/") and os.path.exists(os.path.join(os.path.dirname(os.path.dirname(A.__file__)), path)), where
    # every exact row of the fp32 table is here at first order, or is a convolution row its geometry's rows stand for, or is listed
    for name in A.EXACT:
        base = A.TABLE[name]
        if name in B.TABLE or name.startswith(("conv2:", "conv3:")) or not base.values:
            continue
        geom = name.split(":")[1] if name.startswith("conv") else None
        assert name in B.LEFT_OUT or base.igo or geom in B.LEFT_OUT, name
