"""The bf16-storage view of the autograd-layer table (tests/autograd_cases.py), for tests/test_autograd_bf16_cases_cpu.py and
tests/test_autograd_bf16_gpu.py.  Plain Python: nothing here touches a device.

What is under test is the Python of confignet_amd/ops.py that decides, per call, which kernel family runs and where a tensor changes
storage type (_act_out_dtype, _unify, cast / f32, _bf16_conv_ok, MIXED_FIRST_LAYERS, the fp32-only guards) as the Functions of
confignet_amd/functional.py drive it with ops.set_activation_dtype("bf16").

THE CONDITION.  bf16 carries 8 significant bits: k * u with u a power of two and |k| <= 256 is stored exactly.  Every case here
reuses a statement and a product of the fp32 table, with inputs and cotangents redrawn SPARSE (A.sparse_inputs: magnitudes 1 .. lim,
a fraction `density` of the entries nonzero, the table's conventions kept: even filter and odd bias where an activation is fused,
nonzero where it stands alone, distinct values per channel for the pools) so that
  * every activation-typed quantity of the ladder on absolute values is <= 256 * unit (nothing the product stores in bf16 rounds),
  * every other quantity is < 2^24 * unit (fp32 holds each partial sum in any order).
Then the bf16 product equals the float64 statement bit for bit, in default and in deterministic mode; tests/
test_autograd_bf16_cases_cpu.py proves the condition case by case, and that no reference is trivially zero.

ROLES.  Each input is an `activation` -- stored as ops._act_out_dtype(channels) says in bf16 mode: bf16 above 4 channels, else
fp32 -- or a `parameter`: filters, biases, gammas, dense weights, (n, c) coefficients, scales, and the (N, F) latents of the MLP
Functions, which the product keeps in fp32 (ops.py: ACT_DTYPE) and whose grouped GEMM takes nothing else; in lrelu_mask_mul:fp32g
the gradient operand too, as it arrives from a dense layer.  Cotangents take their
output's storage type (expected_storage).

ORDER.  First order, plus the one second-order statement the product runs in bf16: the R1 penalty through ConvFn twice
(conv2:<geometry>:gx:quad:igo).  There the product stores one more activation than the ladder shows -- RowScaleFn's 2 * gx, in
gx's type -- which the CPU test bounds as well.

OUT OF THIS TABLE (they stay where they are):
  * the real-valued cases (norms, GAN losses, regression): tests/test_norm_tails_gpu.py and tests/test_stream_edges_gpu.py hold
    their bf16 values;
  * order 2 and above other than the R1 set; the conv2: / conv3: rows of the fp32 table are, at first order, the conv:<geometry>:none
    row again and are not repeated;
  * LEFT_OUT below: geometries that cannot meet the condition, with the reason."""
import contextlib
import copy
import ctypes

import torch

from confignet_amd import ops
from confignet_amd._lib import CN_BF16, CN_EUNSUPPORTED, CN_F32, lib
from tests import autograd_cases as A
from tests import conv_edge_cases as CE
from tests import test_conv_plan_cpu as P

BF16, F32 = torch.bfloat16, torch.float32
STEPS = 256                      # |k| <= 256: what bf16 stores exactly in units of a power of two

# ---- convolution geometries (tests/conv_edge_cases.py: TABLE), by the storage arm of ops.conv_fwd / conv_dgrad / conv_wgrad they
# are here for, and the density of their draw.  The density is the largest of 1, 1/2, 1/4, 1/8, 1/16 at which the LeakyReLU row
# (unit 1/4: the tightest) meets the condition.
CONV_ARMS = {
    "bf16 family": ("c", "d", "j24", "l32", "n96", "f", "g", "w2", "w4"),
    "fp32 family, cast on each side": ("a", "i52", "c12"),
    "image layer": ("e3s1", "e3s2", "e3s2even", "e7"),
    "thin output": ("k1", "k3", "up2k4"),
}
DENSITY = {
    "a": 1 / 8, "c": 1 / 8, "d": 1 / 8, "j24": 1 / 8, "l32": 1 / 8, "n96": 1 / 8, "f": 1 / 32, "g": 1 / 16, "i52": 1 / 4, "c12": 1 / 4,
    "e3s1": 1.0, "e3s2": 1.0, "e3s2even": 1.0, "e7": 1 / 4, "k1": 1 / 2, "k3": 1 / 4, "up2k4": 1 / 4, "w2": 1 / 8, "w4": 1 / 8,
}
DIRECT = ("a", "g", "up2k4")        # ConvDgradFn (g, up2k4: with sumpool2), ConvWgradFn, ConvNoBiasFromGeomFn applied by themselves
# the first Winograd shapes of tests/conv_edge_cases.py: F(2x2) / F(4x4) launches in fp32 mode once WINO_MIN_WGS, WINO_MIN_FILL and
# WINO4_MIN_WGS are zero (as the fp32 tests set them); in bf16 mode they must stay off the fp32 launch
WINO_GEOMS = {"w2": (CE.WINO_SHAPES[0][0], (3, 3), CE.WINO_SHAPES[0][1], 1, 0, None),
              "w4": (CE.WINO4_SHAPES[0][0], (3, 3), CE.WINO4_SHAPES[0][1], 1, 0, None)}
# a cin that is no multiple of 8: the table's own (j6, cin 6) is no multiple of 4 either and the library refuses its data
# gradient in every mode; this is j6 with both channel counts doubled
CAST_GEOMS = {"c12": ((3, 5, 7, 12), (3, 3), 24, 1, 0, None)}
GEOMS = dict(CE.TABLE, **WINO_GEOMS, **CAST_GEOMS)
# ops.conv_fwd_res / ops.conv_dgrad_res (no Function wraps them: the hand-written ResNet passes call them): in bf16 mode both fall
# back to convolution + nc_lin2; one geometry of the bf16 family and one cast around the fp32 family, stride 1, with their density
RES_GEOMS = {"n96": 1 / 8, "a": 1 / 8}
R1_GEOMS = ("c", "l32", "i52", "c12", "e3s2")       # two of the bf16 family, two cast around the fp32 family, one image layer
R1_DENSITY = {"c": 1 / 16, "l32": 1 / 16, "i52": 1 / 8, "c12": 1 / 8, "e3s2": 1 / 4}
LEFT_OUT = {
    "m": "cin 512: the absolute ladder reaches 97 at a density of 1/8 and the first gradients thin out below it",
    "h": "1x1 with stride 2: three quarters of d y / d x are zero by the geometry, the reference cannot have a quarter of its entries nonzero",
    "h144": "as h",
    "j6": "cin 6 is no multiple of 4: the library refuses the data gradient in every mode (c12 stands in its arm)",
    "b": "1x1 output from a 1x1 input: all taps but the centre are padding, d y / d w is zero on 8 taps of 9",
    "a (R1 set only)": "d (row_sumsq) / d c reaches 258 > 256 under the absolute ladder at a density of 1/16; i52 and c12 take its arm",
    "maxpool:k2s2p0": "a 2x2 / 2 pool of 7 x 9 passes its cotangent to 12 of 63 positions: under a quarter by the geometry; k3s2p1 stays",
}

# ---- the other cases: every exact row of the fp32 table at first order
PARAMETERS = {                   # case-name prefix -> the inputs that are parameters (every other input is an activation)
    "conv:": ("w", "bias"), "conv2:": ("w", "bias"), "conv_dgrad:": ("w",), "conv_wgrad:": (), "conv_nobias:": ("w",),
    "matmul:": ("b",), "linear:": ("w", "b"), "linear_act:": ("w", "b"), "mlp_r1:": ("x", "w0", "b0", "w1", "b1"),
    "mlp_bank:": None,           # None: all of them (latents and weights)
    "lrelu": (), "lrelu_mask_mul": (), "lrelu_mask_mul:fp32g": ("g",), "nc_sumdot:": (), "nc_lin:": ("a1", "a2", "b"), "channel_affine_act:": ("a", "b"),
    "maxpool:": (), "chan_affine3:": (), "sqdiff_sum": (), "mse_sum": (), "sqdiff_group:": (), "row_sumsq": (), "row_scale": ("s",),
    "masked_diff": (),
}
# (density, lim) of the draw where the table's own lim leaves 256 units; everywhere else every entry is nonzero, up to the row's lim
DRAW = {"linear_act:lrelu": (1.0, 1)}      # at lim 3 the gradient into the bf16 x reaches 84 = 336 units of 1/4
# Function classes that can receive a bf16 tensor and whose bf16 values another file holds
HELD = {
    "AdaInFn": "tests/test_norm_tails_gpu.py (real-valued; test_bf16_adain_on_a_constant_channel, the family in bf16 storage)",
    "DiscrTailFn": "tests/test_norm_tails_gpu.py (real-valued; test_bf16_statistics_of_the_tails)",
    "DualTailFn": "tests/test_norm_tails_gpu.py (real-valued; section 4: the family in bf16 storage)",
    "DualTailBatchedFn": "tests/test_norm_tails_gpu.py (real-valued; cn_nc_reduce_dact in bf16 storage)",
    "Rotate3dFn": "tests/test_rotate3d_edges_gpu.py (real-valued: trilinear weights; a bf16 grid is a cast on each side of the fp32 "
                  "kernel, seen by the generator comparisons of tests/test_bf16_gpu.py only)",
    "GanLossFn": "tests/test_stream_edges_gpu.py (real-valued; scores are fp32)",
    "GanLossGroupFn": "tests/test_stream_edges_gpu.py (real-valued; fp32 scores only: functional.gan_losses)",
    "EulerMatrixFn": "tests/test_rotate3d_edges_gpu.py (angles are fp32 latents)",
    "GlobalBatchMoments": "tests/test_autograd_gpu.py (real-valued; (N, F) latents, fp32)",
}


@contextlib.contextmanager
def bf16_mode():
    """ops.ACT_DTYPE = bf16 while the storage predicates are asked (pure Python: no device, no library call)"""
    prev = ops.ACT_DTYPE
    ops.set_activation_dtype(BF16)
    try:
        yield
    finally:
        ops.set_activation_dtype(prev)


def act_dtype(channels):
    with bf16_mode():
        return ops._act_out_dtype(channels)


def _prefix(name):
    hits = [p for p in PARAMETERS if name == p or (p.endswith(":") and name.startswith(p))]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def view(base, density, lim, order=1, name=None):
    """the bf16 view of a row of the fp32 table: same statement and product, sparse inputs and cotangents, its own order"""
    c = copy.copy(base)
    c.base, c.density, c.sparse, c.order, c.ref = base, density, (density, lim), order, None
    c.name = base.name if name is None else name
    c.inputs = lambda: A.sparse_inputs(base, density, lim)
    if order == 1:
        c.quad = False
    return c


def roles(case):
    """{input: "activation" | "parameter"}"""
    params = PARAMETERS[_prefix(case.name)]
    return {k: ("parameter" if (params is None or k in params) else "activation") for k in case.inputs()}


def input_storage(case):
    """{input: dtype} the operand is handed to the product in (uint8 masks stay what they are)"""
    r = roles(case)
    return {k: (v.dtype if v.dtype == torch.uint8 else F32 if r[k] == "parameter" else act_dtype(v.shape[-1])) for k, v in case.inputs().items()}


def geometry(case):
    """the conv_edge_cases entry of a convolution case, or None"""
    parts = case.name.split(":")
    return GEOMS[parts[1]] if parts[0] in ("conv", "conv2", "conv_dgrad", "conv_wgrad", "conv_nobias") else None


def expected_storage(case):
    """the dtype of every level-0 output, from the ops predicates: what a convolution stores is _act_out_dtype(its channels) (the
    bf16 family takes only layers for which that is bf16), dense layers and reductions give fp32, an elementwise map keeps the type
    _unify gives its activation operands, 3-channel maps are computed in fp32"""
    kind = _prefix(case.name)
    st = input_storage(case)
    acts = [st[k] for k, r in roles(case).items() if r == "activation" and st[k] != torch.uint8]
    unified = BF16 if BF16 in acts else F32
    ge = geometry(case)
    if kind in ("conv:", "conv2:", "conv_nobias:"):
        return (act_dtype(ge[2]),)
    if kind == "conv_dgrad:":
        with bf16_mode():
            assert not ops._bf16_conv_ok(CE.geom(ge)) or ops._act_out_dtype(ge[0][-1]) == BF16
        return (act_dtype(ge[0][-1]),)
    if kind in ("conv_wgrad:", "matmul:", "linear:", "linear_act:", "mlp_r1:", "sqdiff_sum", "mse_sum", "sqdiff_group:", "row_sumsq"):
        return (F32,)
    if kind == "mlp_bank:":
        return (F32, F32, F32)
    if kind == "nc_sumdot:":
        return (F32, F32)
    if kind == "nc_lin:":                  # (the offset alone: ops.nc_lin2 asks _act_out_dtype for the channel count)
        return (unified if acts else act_dtype(case.inputs()["b"].shape[-1]),)
    if kind in ("chan_affine3:", "masked_diff"):
        return (F32,)                      # ops.chan_affine3_fwd / masked_diff compute in fp32 (3 channels: fp32 storage anyway)
    assert kind in ("lrelu", "lrelu_mask_mul", "lrelu_mask_mul:fp32g", "channel_affine_act:", "maxpool:", "row_scale"), kind
    return (unified,)


def quantity_storage(case):
    """{quantity of the ladder: dtype}: outputs as expected_storage says, a gradient in the type of what it is a gradient of"""
    ins, outs = input_storage(case), expected_storage(case)
    ref = reference(case)
    st = {}
    for q in ref:
        if q.startswith("y"):
            st[q] = outs[int(q[1:])]
        else:
            k = q.split("/", 1)[1]
            st[q] = ins[k] if k in ins else outs[int(k[1:])]
    return st


def reference(case):
    """the float64 ladder of the case's statement, computed once per view"""
    if case.ref is None:
        case.ref = A.reference(case)
    return case.ref


def res_inputs(name):
    """the sparse draw of conv_edge_cases.integer_inputs (x, w, bias, res, gy, resx) for a geometry of RES_GEOMS"""
    return A.sparse_conv_ints(GEOMS[name], RES_GEOMS[name], 1)


# ---- profile families ----------------------------------------------------------------------------------------------------------
def _family(index):
    return None if index < 0 else ops.PROF_FAMILIES[index]


def _code(dtype):
    return CN_BF16 if dtype == BF16 else CN_F32


def fwd_arm(g, has_bias, act, x_dtype, mixed=True):
    """(profile family, storage conversions) of ops.conv_fwd on geometry g in bf16 mode (call inside bf16_mode): the conversions
    are the calls of ops.cast that change a type -- the operand on its way into the fp32 family, the result on its way out.
    mixed: the image layers on the kernels that read / write both storage types (the product's setting, ops.MIXED_FIRST_LAYERS = True:
    what the tests expect; False: what the fallback would show)"""
    if ops._bf16_conv_ok(g):
        return "igemm_bf16", int(x_dtype != BF16)
    casts, out = int(x_dtype != F32), ops._act_out_dtype(g.cout)
    if out == BF16 and mixed and g.cin == 3:
        rc, p = P.plan(g, 0, int(has_bias), act, 0, 0, CN_F32, CN_BF16)
        if rc == 0:
            return _family(p[4]), casts
        assert rc == CN_EUNSUPPORTED, rc
    rc, p = P.plan(g, 0, int(has_bias), act, 0, 0, CN_F32, CN_F32)
    assert rc == 0, rc
    return _family(p[4]), casts + int(out != F32)


def dgrad_arm(g, gy_dtype, mixed=True):
    """(profile family, storage conversions) of ops.conv_dgrad"""
    if ops._bf16_conv_ok(g):
        return "igemm_bf16", int(gy_dtype != BF16)
    gd, out = P.dgrad_geom(g), ops._act_out_dtype(g.cin)
    if gy_dtype == BF16 and mixed and g.cin == 3:
        rc, p = P.plan(gd, 0, 0, ops.ACT_NONE, 0, 0, CN_BF16, CN_F32)
        if rc == 0:
            return _family(p[4]), int(out != F32)
        assert rc == CN_EUNSUPPORTED, rc
    casts = int(gy_dtype != F32) + int(out != F32)
    if ops.DGRAD_FROM_W:
        rc, p = P.plan(gd, 1, 0, ops.ACT_NONE, 0, 0, CN_F32, CN_F32)
        if rc == 0:
            return _family(p[4]), casts
        assert rc == CN_EUNSUPPORTED, rc
    rc, p = P.plan(gd, 0, 0, ops.ACT_NONE, 0, 0, CN_F32, CN_F32)
    assert rc == 0, rc
    return _family(p[4]), casts


def wgrad_family(g, gy_dtype):
    """the family ops.conv_wgrad launches (cn_conv_wgrad_dt: x in bf16 where the bf16 kernels take the layer, gy as stored where
    a kernel reads that next to x, else in x's type)"""
    x_dt, gy_dt = (CN_BF16 if ops._bf16_conv_ok(g) else CN_F32), _code(gy_dtype)
    out = (ctypes.c_longlong * 12)()
    rc = lib.cn_conv_wgrad_plan(ctypes.byref(g), x_dt, gy_dt, 0, 0xffffffff, -1, out)
    if rc == CN_EUNSUPPORTED and gy_dt != x_dt:
        rc = lib.cn_conv_wgrad_plan(ctypes.byref(g), x_dt, x_dt, 0, 0xffffffff, -1, out)
    assert rc == 0, rc
    return _family(out[4])


def _arms(case, mixed=True):
    ge = geometry(case)
    g = CE.geom(ge)
    act = {"none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU, "relu": ops.ACT_RELU}[case.name.split(":")[2]]
    with bf16_mode():
        y_dtype = ops._act_out_dtype(g.cout)
        if ops.upfold_ok(g):
            # the collapsed form runs three convolutions on the class filters' geometries, whose channel counts are g's: only the
            # bf16 family's answer is known without those geometries
            assert ops._bf16_conv_ok(g), "a collapsed geometry outside the bf16 family: extend expected_families"
            return {"fwd": ("igemm_bf16", 0), "dgrad": ("igemm_bf16", 0), "wgrad": ("igemm_bf16_wgrad", 0)}
        return {"fwd": fwd_arm(g, True, act, ops._act_out_dtype(g.cin), mixed), "dgrad": dgrad_arm(g, y_dtype, mixed), "wgrad": (wgrad_family(g, y_dtype), None)}


def expected_families(case):
    """{"fwd", "dgrad", "wgrad"} -> the profile family ConvFn's forward, its data gradient and its filter gradient must report
    for a conv:<geometry>:<activation> case (None: a launch outside the profiled families), from ops._bf16_conv_ok and the plan
    queries of the library (cn_conv_fwd_plan, cn_conv_wgrad_plan)."""
    return {k: v[0] for k, v in _arms(case).items()}


def expected_casts(case, mixed=True):
    """{"fwd", "dgrad"} -> the storage conversions (calls of ops.cast that change a type) of the forward and of the data gradient.
    The image layers' own kernels (MIXED_FIRST_LAYERS) report the family of the fp32 kernels they replace: what tells the two arms
    apart is that they convert nothing."""
    return {k: v[1] for k, v in _arms(case, mixed).items() if k != "wgrad"}


# ---- the table -----------------------------------------------------------------------------------------------------------------
TABLE = {}


def _put(c):
    assert c.name not in TABLE, c.name
    TABLE[c.name] = c


def _build():
    scratch = {}

    def add(*a, **kw):
        c = A.Case(*a, **kw)
        scratch[c.name] = c
    geoms = [n for names in CONV_ARMS.values() for n in names]
    A.conv_cases(geoms, DIRECT, add, table=GEOMS)
    for n in geoms:
        for tag in ("none", "lrelu", "relu"):
            _put(view(scratch["conv:%s:%s" % (n, tag)], DENSITY[n], 1))
    for n in DIRECT:
        for kind in ("conv_dgrad", "conv_wgrad", "conv_nobias"):
            _put(view(scratch["%s:%s" % (kind, n)], DENSITY[n], 1))
    for n in R1_GEOMS:
        _put(view(scratch["conv2:%s:gx:quad:igo" % n], R1_DENSITY[n], 1, order=2))
    for name in A.EXACT:
        base = A.TABLE[name]
        if name.startswith(("conv:", "conv2:", "conv3:", "conv_dgrad:", "conv_wgrad:", "conv_nobias:")) or not base.values:
            continue
        if base.igo or name in LEFT_OUT:
            continue                       # mlp_r1:pieces: second order through the dense Functions, fp32 latents: the fp32 table's
        _put(view(base, *DRAW.get(name, (1.0, base.lim))))
    # an fp32 gradient (arriving from a dense layer) meets a bf16 activation: ops._unify takes both to bf16
    _put(view(A.TABLE["lrelu_mask_mul"], 1.0, 3, name="lrelu_mask_mul:fp32g"))


_build()
CONV = [n for n in TABLE if n.startswith("conv:")]
R1 = [n for n in TABLE if n.startswith("conv2:")]


def arm_of(name):
    g = name.split(":")[1]
    return next(arm for arm, names in CONV_ARMS.items() if g in names)


def classes_covered():
    out = set(HELD)
    for c in TABLE.values():
        out.update(c.classes)
    return out


def bf16_reachable_classes():
    """the Function classes a bf16 tensor can reach: every class of functional.py and losses.py -- none of them asserts fp32 on
    all its tensor inputs before an activation-sized operand could arrive, so all are either in the table or held"""
    return A.function_classes()
