"""Case table, inputs, float64 statements and bounds of the autograd-layer tests (tests/test_autograd_cases_cpu.py,
tests/test_autograd_gpu.py).  Plain Python: nothing here touches a device.

What is under test is confignet_amd/functional.py (and the Python of ops.py it drives): the torch.autograd.Function classes whose
backward passes are written in terms of each other.  A case names

  * a STATEMENT: a function of CPU tensors written with ordinary torch operators (oracle.ref_ops, tests.conv_edge_cases for the
    convolutions, plain expressions elsewhere), valid in float64 (the reference) and in float32 (the yardstick);
  * the PRODUCT: the same function through the Functions, on device tensors;
  * the inputs, which of them are differentiated, and the order.

Both go through the same LADDER (ladder()): outputs y; g1 = grad(y, inputs, c0) with cotangents c0 that are leaves themselves;
g2 = grad(g1, inputs + c0, e1); g3 = grad(g2, inputs + c0, e2) -- no arithmetic between the levels, so on the device nothing runs but
the Functions.  A quantity that is None (no path) counts as zero on either side; a reference quantity that is not zero must come
back, so a backward that cuts the graph (a raw kernel's result under create_graph) fails instead of passing as a silent zero.

EXACT cases.  The statements of the conv, matmul, lrelu sets, the nc set, the pools, the masked difference, the squared-difference
sum, the row maps, ChanAffine3Fn (scale 128, integer offsets), ChannelAffineActFn and the MLPs are multilinear or piecewise linear.
With integer inputs and cotangents (|.| <= lim), slope 0.25 and every pre-activation at |v| >= 1 (filters even, biases odd where the
activation is fused; nonzero integers where it stands alone) every term of every sum, at every order, is a multiple of the case's
`unit` (1 / 4 per LeakyReLU mask that can multiply it, the loss scale where there is one).  The same ladder on the absolute values
(subtractions turned into additions, activations into the identity) bounds every partial sum: while that bound / unit < 2^24,
fp32 holds each partial sum exactly in ANY order, and the device result must equal the float64 one bit for bit (torch.equal), in
default and in deterministic mode.  tests/test_autograd_cases_cpu.py checks the bound, the unit and the margins of every case.

REAL-VALUED cases (rsqrt, sqrt, softplus, division, means over a count that is no power of two) take the rule of
tests/test_norm_tails_gpu.py unchanged: error relative to max |reference| of the quantity, bound = MULT = 32 x yardstick (the float32
CPU run of the statement against its float64 run; second derivatives: the second-order statement's own), never above 2e-4 on
outputs and 5e-4 on gradients.  Inputs are drawn in float32.
  moved here from the exact list: SqDiffGroupSumFn with sizes (2, 3) -- its scale 1 / (3 * per) is no power of two.

HELD ELSEWHERE (HELD): classes whose values another file holds; here only what that file does not (the create_graph guard)."""
import zlib

import numpy as np
import torch

from confignet_amd import ops
from oracle import ref_ops as O
from tests import conv_edge_cases as CE
from tests import norm_tail_ref as NR

SLOPE = 0.25
REAL_SLOPE = 0.3
MULT = 32.0
CAP_OUT, CAP_GRAD = 2e-4, 5e-4
ACT_NONE, ACT_LRELU, ACT_RELU = ops.ACT_NONE, ops.ACT_LRELU, ops.ACT_RELU
CONV_GEOMS = ("a", "c", "e3s2", "h", "k1", "f", "g")
DENSE = (5, 9, 7)                  # (m, k, n)
NC_SHAPES = ((2, 3, 5, 6), (2, 3, 5, 8))       # c = 6: scalar kernels, c = 8: float4 kernels

# classes whose values are held by another file (the arms named there are not repeated here)
HELD = {
    "Rotate3dFn": "tests/test_rotate3d_edges_gpu.py (values and first-order gradients); here: the create_graph guard",
    "EulerMatrixFn": "tests/test_rotate3d_edges_gpu.py; here: the create_graph guard",
    "DualTailFn": "tests/test_norm_tails_gpu.py (forward, backward with its second-order terms, every None arm)",
    "DualTailBatchedFn": "tests/test_norm_tails_gpu.py (both arms of its backward)",
    "AdaInFn": "tests/test_norm_tails_gpu.py (both dispatch arms, offset and constant inputs); here: the create_graph guard",
}
# arms of classes in the table that another file holds and this one does not repeat
ARMS_ELSEWHERE = {
    "DiscrTailFn": "gy + gstyle, gstyle = None, gy = None with want_style on: tests/test_norm_tails_gpu.py; here: want_style off, the guard",
    "ChannelAffineActFn": "x + a + b at c % 4 == 0 (one pass) and c = 6 (separate passes), real-valued: tests/test_norm_tails_gpu.py; "
                          "here: the same arms bit for bit on integers, the x-only arm, the guard",
}


# Functions whose backward is a plain kernel call guarded by functional._first_order_only (a _RefuseFn node)
RAW_BACKWARD = ("MaxPoolFn", "ChanAffine3Fn", "Rotate3dFn", "EulerMatrixFn", "SqDiffSumFn", "SqDiffGroupSumFn", "MaskedDiffFn", "GanLossFn",
                "GanLossGroupFn")


class Case:
    """One row of the table.  statement(t, absolute=False) and product(F, t) take a dict name -> tensor and return a tuple of
    tensors (None: an output the case does not have)."""

    def __init__(self, name, classes, inputs, diff, statement, product, order=1, exact=True, unit=1.0, first=None, used=None,
                 quad=False, igo=False, guard=None, pre=None, pools=None, lim=3, note=""):
        self.name, self.classes, self.inputs, self.diff = name, tuple(classes), inputs, tuple(diff)
        if guard is not None and any(c in RAW_BACKWARD for c in classes):
            self.classes += ("_RefuseFn",)        # the node that refuses their second derivative
        self.statement, self.product, self.order, self.exact, self.unit = statement, product, order, exact, unit
        self.first = tuple(first) if first is not None else self.diff       # what the first level differentiates
        self.used = used                   # per output: False = its cotangent is absent
        self.quad = quad                   # level 2 is row_sumsq(g).sum() instead of <g, e>
        self.igo = igo                     # the first pass of the product runs under F.input_grads_only()
        self.guard = guard                 # "raises": level 2 of the product must raise; "either": be right or raise
        self.pre, self.pools, self.lim, self.note = pre, pools, lim, note
        self.values = not all(c in HELD for c in self.classes)      # False: the values are another file's, here only the guard

    def __repr__(self):
        return "Case(%s)" % self.name


# ---- drawing --------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


_SPARSE = None          # (density, lim) while the inputs of a sparse view of a case are drawn (sparse_inputs), else None


def _thin(key, shape, density, lim):
    """the sparse draw: magnitudes 1 .. lim, random signs, a fraction `density` of the entries kept, zero elsewhere"""
    rng = _rng("sparse", key)
    mag = rng.integers(1, lim + 1, size=shape).astype(np.float64)
    sign = np.where(rng.integers(0, 2, size=shape) > 0, 1.0, -1.0)
    return np.where(rng.random(size=shape) < density, mag * sign, 0.0)


def ints(key, shape, lim=3, nonzero=False, even=False, odd=False, sparse=None):
    """integers in [-lim, lim]; sparse = (density, lim): the sparse draw instead (also while sparse_inputs draws a case's inputs).
    The conventions hold in both: even / odd are applied after the draw, nonzero turns a zero into a one."""
    sparse = _SPARSE if sparse is None else sparse
    if sparse is not None:
        v = _thin(key, shape, sparse[0], min(lim, sparse[1]))
    else:
        v = _rng("int", key).integers(-lim, lim + 1, size=shape).astype(np.float64)
    if even:
        v = 2.0 * v
    if odd:
        v = 2.0 * v + 1.0
    if nonzero:
        v[v == 0] = 1.0
    return torch.from_numpy(np.asarray(v))


def reals(key, shape, scale=1.0, offset=0.0):
    v = _rng("real", key).standard_normal(size=shape).astype(np.float32) * np.float32(scale) + np.float32(offset)
    return torch.from_numpy(np.asarray(v, dtype=np.float64))


def distinct(key, shape, positive=False):
    """distinct integers (no tie in any pool window), centred on zero; positive: 1 .. n (no zero of a padded border wins or ties)"""
    n = int(np.prod(shape))
    if _SPARSE is not None:
        # the sparse view: distinct within each channel only (a pool never compares two channels), so that no value passes the
        # count of positions of one channel
        c, rng = shape[-1], _rng("perm", key)
        per = n // c
        cols = [rng.permutation(per) - (-1 if positive else per // 2) for _ in range(c)]
        return torch.from_numpy(np.stack(cols, axis=-1).astype(np.float64).reshape(shape))
    return torch.from_numpy((_rng("perm", key).permutation(n) - (-1 if positive else n // 2)).astype(np.float64).reshape(shape))


def conv_ints(case, lim=3):
    """CE.integer_inputs of a conv_edge_cases entry; while sparse_inputs draws: the sparse draw of the same tensors"""
    i = CE.integer_inputs(case, lim=lim)
    if _SPARSE is None:
        return i
    return {k: torch.from_numpy(_thin(("conv", case, k), tuple(v.shape), _SPARSE[0], min(lim, _SPARSE[1]))) for k, v in i.items()}


def sparse_conv_ints(case, density, lim=1):
    """conv_ints of a conv_edge_cases entry in the sparse draw"""
    global _SPARSE
    prev, _SPARSE = _SPARSE, (density, lim)
    try:
        return conv_ints(case, lim)
    finally:
        _SPARSE = prev


def sparse_inputs(case, density, lim=1):
    """case.inputs() with every integer draw replaced by the sparse one"""
    global _SPARSE
    prev, _SPARSE = _SPARSE, (density, lim)
    try:
        return case.inputs()
    finally:
        _SPARSE = prev


def cotangent(case, level, index, shape, real):
    key = (case.name, "cot", level, index)
    lim = min(case.lim, 2) if case.quad else case.lim
    return reals(key, shape) if real else ints(key, shape, lim=lim, sparse=getattr(case, "sparse", None))


# ---- the ladder -----------------------------------------------------------------------------------------------------------------
def _grad(outs, targets, cots, create_graph):
    live = [(o, c) for o, c in zip(outs, cots) if o is not None and o.requires_grad]
    if not live:
        return [None] * len(targets)
    return list(torch.autograd.grad([o for o, _ in live], targets, [c for _, c in live], create_graph=create_graph, allow_unused=True))


def ladder(case, fn, t, make, order=None, absolute=False, first_pass=None, row_sumsq=None, make_cot=None):
    """The quantities of `case` from fn(t): {"y<j>", "d1/<input>", "d2/<input>", "d2/c<j>", "d3/..."} -> tensor | None.
    make(tensor64) turns a drawn float64 CPU tensor into the operand type (dtype, device); first_pass: a context manager factory
    for level 1 (F.input_grads_only); row_sumsq: the product's own row_sumsq for quad cases; make_cot(j, tensor64): the same as
    make for the cotangent of output j where that depends on the output (its storage type)."""
    order = case.order if order is None else order
    real = not case.exact
    for k in case.diff:
        t[k].requires_grad_(True)
    ys = fn(t)
    ys = ys if isinstance(ys, (tuple, list)) else (ys,)
    out = {}
    outs, c0 = [], []
    for j, y in enumerate(ys):
        if y is None:
            continue
        out["y%d" % j] = y.detach()
        if case.used is not None and not case.used[j]:
            continue
        c = cotangent(case, 1, j, tuple(y.shape), real)
        c = c.abs() if absolute else c
        c = (make(c) if make_cot is None else make_cot(j, c)).requires_grad_(order > 1)
        outs.append(y)
        c0.append(("c%d" % j, c))
    firsts = [t[k] for k in case.first]
    if first_pass is not None:
        with first_pass():
            g = _grad(outs, firsts, [c for _, c in c0], order > 1)
    else:
        g = _grad(outs, firsts, [c for _, c in c0], order > 1)
    for k, gi in zip(case.first, g):
        out["d1/" + k] = gi
    targets = [(k, t[k]) for k in case.diff] + c0
    for level in range(2, order + 1):
        if case.quad and level == 2:
            live = [gi for gi in g if gi is not None and gi.requires_grad]
            if not live:
                break
            sq = row_sumsq if row_sumsq is not None else (lambda v: (v * v).sum(dim=1))
            loss = sum(sq(gi.reshape(gi.shape[0], -1)).sum() for gi in live)
            g = list(torch.autograd.grad(loss, [v for _, v in targets], create_graph=level < order, allow_unused=True))
        else:
            es = []
            for i, gi in enumerate(g):
                e = None
                if gi is not None:
                    e = cotangent(case, level, i, tuple(gi.shape), real)
                    e = make(e.abs() if absolute else e)
                es.append(e)
            if not any(gi is not None and gi.requires_grad for gi in g):
                break
            g = _grad(g, [v for _, v in targets], es, level < order)
        for (k, _), gi in zip(targets, g):
            out["d%d/%s" % (level, k)] = gi
    return {k: (None if v is None else v.detach()) for k, v in out.items()}


def inputs_as(case, dtype, absolute=False):
    t = case.inputs()
    return {k: (v if v.dtype == torch.uint8 else (v.abs() if absolute else v).to(dtype).clone()) for k, v in t.items()}


def reference(case, dtype=torch.float64, order=None):
    t = inputs_as(case, dtype)
    return ladder(case, lambda t_: case.statement(t_), t, lambda v: v.to(dtype).clone(), order)


def absolute_ladder(case, order=None):
    """the ladder on absolute values (subtractions as additions, activations as the identity), quantity by quantity"""
    t = inputs_as(case, torch.float64, absolute=True)
    return ladder(case, lambda t_: case.statement(t_, absolute=True), t, lambda v: v.clone(), order, absolute=True)


def absolute_bound(case, order=None):
    """max over every quantity of the ladder on absolute values: no partial sum of the case, at any order, is larger"""
    q = absolute_ladder(case, order)
    return max([float(v.abs().max()) for v in q.values() if v is not None and v.numel()] + [0.0])


def is_zero(v):
    return v is None or not bool(v.any())


def yardstick(case):
    """(reference, {quantity: relative error of the float32 CPU run}) of a real-valued case"""
    r64, r32 = reference(case, torch.float64), reference(case, torch.float32)
    yard = {}
    for k, v in r64.items():
        if is_zero(v):
            yard[k] = 0.0
        else:
            w = r32.get(k)
            yard[k] = NR.rel_err(torch.zeros_like(v) if w is None else w, v)
    # scalar outputs of one case (the losses of GanLossGroupFn's heads) share one yardstick, the largest of theirs: a scalar's own
    # float32 error is ONE draw of a rounding error, not a spread.  Measured on an MI355X before this rule: the 7-score head of
    # gan_loss_group came out 7.3e-08 off (about one fp32 rounding of the stored scalar, 2^-24 = 6.0e-08) while the CPU's float32
    # run happened to land 2.1e-09 from the float64 value, a bound of 6.6e-08 -- below what an fp32 result can be held to; the
    # other heads' own yardsticks are 1.3e-07, 5.5e-08 and 5.1e-08.
    scalars = [k for k, v in r64.items() if k.startswith("y") and not is_zero(v) and v.dim() == 0]
    if len(scalars) > 1:
        pooled = max(yard[k] for k in scalars)
        for k in scalars:
            yard[k] = pooled
    return r64, yard


def bound_of(quantity, yard):
    return min(MULT * yard, CAP_OUT if quantity.startswith("y") else CAP_GRAD)


def compare(case, got, ref, yard=None, rows=None):
    """The failures (strings) of the product's quantities `got` against the reference's `ref`; rows: a list that receives
    (case, quantity, order, yardstick, bound, observed) of every quantity compared."""
    fails = []
    for k in sorted(set(got) | set(ref)):
        g, r = got.get(k), ref.get(k)
        g = None if g is None else g.detach().cpu().double()
        order = 0 if k.startswith("y") else int(k[1])
        if is_zero(r):
            obs = 0.0 if g is None else float(g.abs().max()) if g.numel() else 0.0
            if rows is not None:
                rows.append((case.name, k, order, 0.0, 0.0, obs))
            if obs != 0.0:
                fails.append("%s: the reference is zero or absent, got max |.| = %.3e" % (k, obs))
            continue
        if g is None:
            fails.append("%s: absent (None, or cut from the graph) where the reference reaches %.3e" % (k, float(r.abs().max())))
            continue
        if tuple(g.shape) != tuple(r.shape):
            fails.append("%s: shape %s, reference %s" % (k, tuple(g.shape), tuple(r.shape)))
            continue
        err = NR.rel_err(g, r)
        y, bound = (0.0, 0.0) if case.exact else (yard[k], bound_of(k, yard[k]))
        if rows is not None:
            rows.append((case.name, k, order, y, bound, err))
        if case.exact:
            if not torch.equal(g, r):
                fails.append("%s: %d of %d elements differ, largest error %.3e of the maximum" % (k, int((g != r).sum()), g.numel(), err))
        elif not err <= bound:
            fails.append("%s: error %.3e of its maximum, bound %.3e (yardstick %.3e)" % (k, err, bound, y))
    return fails


# ---- statements -----------------------------------------------------------------------------------------------------------------
def _mask(v, neg=SLOPE):
    return torch.where(v.detach() > 0, torch.ones((), dtype=v.dtype), torch.full((), neg, dtype=v.dtype))


def _act(v, act, absolute=False):
    if absolute or act == ACT_NONE:
        return v
    return O.leaky_relu(v, SLOPE) if act == ACT_LRELU else O.relu(v)


def _spec(case):
    _, k, _, stride, up, epad = case
    return ops.ConvSpec(k, stride=stride, up=up, explicit_pad=epad)


def _bcast(v, x):
    return v.reshape(v.shape[0], *([1] * (x.dim() - 2)), v.shape[-1])


def _nc_sum(v, pc):
    return v.sum(dim=tuple(range(0, v.dim() - 1))).reshape(1, -1) if pc else v.sum(dim=tuple(range(1, v.dim() - 1)))


def conv_statement(case, x, w, b):
    """conv_edge_cases._conv; a filter with one output channel is run as two copies of it and the first kept (torch's CPU double
    backward refuses the permuted one-channel filter: "grad_weight must be contiguous")"""
    if w.shape[-1] != 1:
        return CE._conv(case, x, w, b)
    return CE._conv(case, x, torch.cat([w, w], dim=-1), None if b is None else torch.cat([b, b]))[..., :1]


def dgrad_statement(case, gy, w):
    """d conv / d x applied to gy as a function of (gy, w): autograd through the convolution at x = 0 (it is linear in x)"""
    x = torch.zeros(case[0], dtype=w.dtype, requires_grad=True)
    return torch.autograd.grad(conv_statement(case, x, w, None), x, gy, create_graph=True)[0]


def wgrad_statement(case, x, gy):
    w = torch.zeros(CE.filter_shape(case), dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(conv_statement(case, x, w, None), w, gy, create_graph=True)[0]


def mlp2(x, w0, b0, w1, b1, absolute=False):
    return O.dense(_act(O.dense(x, w0, b0), ACT_LRELU, absolute), w1, b1)


def regression_statement(out, labels, weight):
    """normalized_latent_regression (confignet_second_stage.py:96-107) with the statistics of the whole batch"""
    l_mean, o_mean = labels.mean(dim=0, keepdim=True), out.mean(dim=0, keepdim=True)
    l_var = ((labels - l_mean) ** 2).mean(dim=0, keepdim=True)
    den = torch.sqrt(l_var + 1e-3)
    den = torch.cat((den[:, :-3], torch.ones((1, 3), dtype=den.dtype)), dim=1)
    return (((l_mean + (labels - l_mean) / den) - (o_mean + (out - o_mean) / den)) ** 2).mean() * weight


# ---- the table ------------------------------------------------------------------------------------------------------------------
TABLE = {}


def _add(*a, **kw):
    c = Case(*a, **kw)
    assert c.name not in TABLE, c.name
    TABLE[c.name] = c
    return c


def _conv_inputs(name, fused, lim=3, table=CE.TABLE):
    case = table[name]

    def make():
        i = conv_ints(case, lim=lim)
        x, w, b = i["x"], i["w"], i["bias"]
        if fused:                        # even filter, odd bias: every pre-activation is an odd integer
            w, b = 2.0 * w, 2.0 * b + 1.0
        return {"x": x, "w": w, "bias": b}
    return make


def conv_cases(names, direct, _add, table=CE.TABLE):
    """the rows of the geometries `names` (ConvFn with each activation, its second-order statements) and of `direct` (ConvDgradFn,
    ConvWgradFn, ConvNoBiasFromGeomFn applied by themselves) through _add; tests/autograd_bf16_cases.py builds its own geometries'
    rows with it (table: where the geometries are looked up)"""
    _conv_inputs = lambda name, fused, lim=3: globals()["_conv_inputs"](name, fused, lim, table)
    for name in names:
        case = table[name]
        spec = _spec(case)
        for act, tag in ((ACT_NONE, "none"), (ACT_LRELU, "lrelu"), (ACT_RELU, "relu")):
            fused = act != ACT_NONE
            stmt = lambda t, absolute=False, case=case, act=act: (_act(conv_statement(case, t["x"], t["w"], t["bias"]), act, absolute),)
            prod = lambda F, t, spec=spec, act=act: (F.conv(t["x"], t["w"], t["bias"], spec, act, SLOPE if act == ACT_LRELU else 0.0),)
            pre = (lambda t, case=case: [conv_statement(case, t["x"], t["w"], t["bias"])]) if fused else None
            _add("conv:%s:%s" % (name, tag), ["ConvFn", "ConvDgradFn", "ConvWgradFn"], _conv_inputs(name, fused), ("x", "w", "bias"), stmt, prod,
                 order=1, guard="raises" if fused else None, pre=pre, unit=0.25 if act == ACT_LRELU else 1.0,
                 note="first order, all seven requires_grad subsets" + ("; collapsed form" if name in ("f", "g") else ""))
        stmt = lambda t, absolute=False, case=case: (conv_statement(case, t["x"], t["w"], t["bias"]),)
        prod = lambda F, t, spec=spec: (F.conv(t["x"], t["w"], t["bias"], spec),)
        cls = ["ConvFn", "ConvDgradFn", "ConvNoBiasFromGeomFn", "ConvWgradFn"]
        for igo in (False, True):
            sfx = ":igo" if igo else ""
            _add("conv2:%s:gx%s" % (name, sfx), cls, _conv_inputs(name, False), ("x", "w", "bias"), stmt, prod, order=2, first=("x",), igo=igo,
                 note="<d y / d x . c, e> to x, w, bias, c")
            qlim = 1 if name in ("f", "g") else 2          # (the quadratic statement: 1 where the reduction is longest)
            _add("conv2:%s:gx:quad%s" % (name, sfx), cls, _conv_inputs(name, False, qlim), ("x", "w", "bias"), stmt, prod, order=2, first=("x",), igo=igo,
                 quad=True, lim=qlim, note="row_sumsq(d y / d x . c).sum() to x, w, bias, c (the R1 statement)")
        _add("conv2:%s:gw" % name, cls, _conv_inputs(name, False), ("x", "w", "bias"), stmt, prod, order=2, first=("w",),
             note="<d y / d w . c, e> to x, w, bias, c: ConvWgradFn.backward")
        _add("conv2:%s:all" % name, cls, _conv_inputs(name, False), ("x", "w", "bias"), stmt, prod, order=2,
             note="every first gradient at once, the bias gradient included")
    for name in direct:
        case = table[name]

        def gy_w(case=case):
            i = conv_ints(case, lim=3)
            return {"gy": i["gy"], "w": i["w"]}

        def x_gy(case=case):
            i = conv_ints(case, lim=3)
            return {"x": i["x"], "gy": i["gy"]}

        def x_w(case=case):
            i = conv_ints(case, lim=3)
            return {"x": i["x"], "w": i["w"]}
        _add("conv_dgrad:%s" % name, ["ConvDgradFn", "ConvNoBiasFromGeomFn", "ConvWgradFn"], gy_w, ("gy", "w"),
             lambda t, absolute=False, case=case: (dgrad_statement(case, t["gy"], t["w"]),),
             lambda F, t, case=case: (F.ConvDgradFn.apply(t["gy"], t["w"], CE.geom(case)),), order=2)
        _add("conv_wgrad:%s" % name, ["ConvWgradFn", "ConvDgradFn", "ConvNoBiasFromGeomFn"], x_gy, ("x", "gy"),
             lambda t, absolute=False, case=case: (wgrad_statement(case, t["x"], t["gy"]),),
             lambda F, t, case=case: (F.ConvWgradFn.apply(t["x"], t["gy"], CE.geom(case), CE.filter_shape(case)),), order=2)
        _add("conv_nobias:%s" % name, ["ConvNoBiasFromGeomFn", "ConvDgradFn", "ConvWgradFn"], x_w, ("x", "w"),
             lambda t, absolute=False, case=case: (conv_statement(case, t["x"], t["w"], None),),
             lambda F, t, case=case: (F.ConvNoBiasFromGeomFn.apply(t["x"], t["w"], CE.geom(case)),), order=2)


def _conv_cases():
    conv_cases(CONV_GEOMS, ("a", "g"), _add)
    case_a = CE.TABLE["a"]
    _add("conv3:a", ["ConvFn", "ConvDgradFn", "ConvNoBiasFromGeomFn", "ConvWgradFn"], _conv_inputs("a", False), ("x", "w", "bias"),
         lambda t, absolute=False: (conv_statement(case_a, t["x"], t["w"], t["bias"]),), lambda F, t: (F.conv(t["x"], t["w"], t["bias"], _spec(case_a)),),
         order=3, lim=2, note="third-order spot check")


def _dense_cases():
    m, k, n = DENSE
    for ta in (False, True):
        for tb in (False, True):
            def make(ta=ta, tb=tb):
                return {"a": ints(("mm", ta, tb, "a"), (k, m) if ta else (m, k)), "b": ints(("mm", ta, tb, "b"), (n, k) if tb else (k, n))}
            _add("matmul:%d%d" % (ta, tb), ["MatmulFn"], make, ("a", "b"),
                 lambda t, absolute=False, ta=ta, tb=tb: ((t["a"].t() if ta else t["a"]) @ (t["b"].t() if tb else t["b"]),),
                 lambda F, t, ta=ta, tb=tb: (F.MatmulFn.apply(t["a"], t["b"], ta, tb),), order=3 if (ta and tb) else 2)
    for bias in (True, False):
        def make(bias=bias):
            t = {"x": ints("lin:x", (m, k)), "w": ints("lin:w", (k, n))}
            if bias:
                t["b"] = ints("lin:b", (n,))
            return t
        _add("linear:%s" % ("bias" if bias else "nobias"), ["LinearFn", "MatmulFn"], make, ("x", "w", "b") if bias else ("x", "w"),
             lambda t, absolute=False: (O.dense(t["x"], t["w"], t.get("b")),), lambda F, t: (F.linear(t["x"], t["w"], t.get("b")),), order=2)

    def mlp_inputs(rows, lim):
        # even weights, odd biases: the hidden pre-activation is an odd integer
        return lambda: {"x": ints(("r1", rows, "x"), (rows, k), lim=lim), "w0": ints(("r1", "w0"), (k, n), lim=lim, even=True),
                        "b0": ints(("r1", "b0"), (n,), lim=lim, odd=True), "w1": ints(("r1", "w1"), (n, 3), lim=lim), "b1": ints(("r1", "b1"), (3,), lim=lim)}
    pre = lambda t: [O.dense(t["x"], t["w0"], t["b0"])]
    stmt = lambda t, absolute=False: (mlp2(t["x"], t["w0"], t["b0"], t["w1"], t["b1"], absolute),)
    prod = lambda F, t: (F.linear(F.lrelu(F.linear(t["x"], t["w0"], t["b0"]), SLOPE), t["w1"], t["b1"]),)
    _add("mlp_r1:pieces", ["LinearFn", "MatmulFn", "LreluFn", "LreluMaskMulFn", "RowSumSqFn", "RowScaleFn"], mlp_inputs(m, 2),
         ("x", "w0", "b0", "w1", "b1"), stmt, prod, order=2, first=("x",), igo=True, quad=True, unit=1.0 / 64, pre=pre, lim=2,
         note="the R1 statement of the latent discriminator at 5 rows: row_sumsq(d y / d x . c).sum() under input_grads_only")

    def r1_stmt(t, absolute=False):
        y = mlp2(t["x"], t["w0"], t["b0"], t["w1"], t["b1"], absolute)
        return (O.r1_penalty(y, t["x"]),)

    def r1_prod(F, t):
        from confignet_amd import losses
        y = F.linear(F.lrelu(F.linear(t["x"], t["w0"], t["b0"]), SLOPE), t["w1"], t["b1"])
        return (losses.gradient_regularization(y, t["x"]),)
    _add("mlp_r1:penalty", ["LinearFn", "MatmulFn", "LreluFn", "LreluMaskMulFn", "RowSumSqFn", "RowScaleFn"], mlp_inputs(8, 1),
         ("x", "w0", "b0", "w1", "b1"), r1_stmt, r1_prod, order=1, unit=1.0 / 128, pre=pre, lim=1,
         note="losses.gradient_regularization itself (the product path), 8 rows so that its mean is a division by a power of two; every "
              "term is a multiple of 5 / 128 (masks 1 / 16, the scale 10 * 0.5 / 8), held in units of 1 / 128 so that 5 k < 2^24 too")

    def la_inputs():
        return {"x": ints("la:x", (m, k)), "w": ints("la:w", (k, n), even=True), "b": ints("la:b", (n,), odd=True)}
    _add("linear_act:lrelu", ["LinearActFn"], la_inputs, ("x", "w", "b"),
         lambda t, absolute=False: (_act(O.dense(t["x"], t["w"], t["b"]), ACT_LRELU, absolute),),
         lambda F, t: (F.linear(t["x"], t["w"], t["b"], ACT_LRELU, SLOPE),), order=1, guard="raises", unit=0.25,
         pre=lambda t: [O.dense(t["x"], t["w"], t["b"])])

    # MlpBankFn: MLP 0 and 1 take the same z tensor, MLP 2 has other widths and a z that does not require grad
    widths = ((k, n, 4), (k, 6, 5), (7, 3, 6))

    def bank_inputs():
        t = {"z0": ints("bank:z0", (m, k)), "z2": ints("bank:z2", (m, 7))}
        for i, (d_in, d_h, d_out) in enumerate(widths):
            t["w0_%d" % i], t["b0_%d" % i] = ints(("bank:w0", i), (d_in, d_h), even=True), ints(("bank:b0", i), (d_h,), odd=True)
            t["w1_%d" % i], t["b1_%d" % i] = ints(("bank:w1", i), (d_h, d_out)), ints(("bank:b1", i), (d_out,))
        return t
    zs = ("z0", "z0", "z2")
    wnames = [n_ % i for i in range(3) for n_ in ("w0_%d", "b0_%d", "w1_%d", "b1_%d")]
    bank_stmt = lambda t, absolute=False: tuple(mlp2(t[zs[i]], *[t[wnames[4 * i + j]] for j in range(4)], absolute) for i in range(3))
    bank_prod = lambda F, t: tuple(F.mlp_bank([t[z] for z in zs], [[t[wnames[4 * i + j]] for j in range(4)] for i in range(3)], SLOPE))
    bank_pre = lambda t: [O.dense(t[zs[i]], t[wnames[4 * i]], t[wnames[4 * i + 1]]) for i in range(3)]
    for tag, used in (("all", (True, True, True)), ("unused1", (True, False, True)), ("unused2", (True, True, False)), ("only2", (False, False, True))):
        _add("mlp_bank:%s" % tag, ["MlpBankFn"], bank_inputs, ["z0"] + wnames, bank_stmt, bank_prod, order=1, used=used, pre=bank_pre, unit=0.25,
             guard="raises" if tag == "all" else None, note="against three separate dense statements; z2 does not require grad")


def _act_nc_cases():
    shape = (3, 5, 7)
    _add("lrelu", ["LreluFn", "LreluMaskMulFn"], lambda: {"x": ints("lrelu:x", shape, nonzero=True)}, ("x",),
         lambda t, absolute=False: (_act(t["x"], ACT_LRELU, absolute),), lambda F, t: (F.lrelu(t["x"], SLOPE),), order=3, unit=0.25,
         pre=lambda t: [t["x"]])
    _add("lrelu_mask_mul", ["LreluMaskMulFn"], lambda: {"g": ints("lmm:g", shape), "y": ints("lmm:y", shape, nonzero=True)}, ("g",),
         lambda t, absolute=False: (t["g"] if absolute else t["g"] * _mask(t["y"]),), lambda F, t: (F.LreluMaskMulFn.apply(t["g"], t["y"], SLOPE),),
         order=3, unit=0.25, pre=lambda t: [t["y"]])
    for shp in NC_SHAPES:
        c, n = shp[-1], shp[0]
        for pc in (False, True):
            for with_b in (False, True):
                for utag, used in (("both", (True, True)), ("s1", (True, False)), ("s2", (False, True))):
                    def make(shp=shp, with_b=with_b):
                        t = {"a": ints(("sd", shp, "a"), shp, lim=2)}
                        if with_b:
                            t["b"] = ints(("sd", shp, "b"), shp, lim=2)
                        return t

                    def stmt(t, absolute=False, pc=pc):
                        b = t.get("b", t["a"])
                        return _nc_sum(t["a"], pc), _nc_sum(t["a"] * b, pc)
                    _add("nc_sumdot:c%d:%s:%s:%s" % (c, "pc" if pc else "nc", "b" if with_b else "self", utag), ["NcSumDotFn", "NcLinFn"], make,
                         ("a", "b") if with_b else ("a",), stmt, lambda F, t, pc=pc: F.NcSumDotFn.apply(t["a"], t.get("b"), pc),
                         order=2, used=used, lim=2)
            co = (1, c) if pc else (n, c)
            arms = {"x1": ("x1",), "x1a1": ("x1", "a1"), "full": ("x1", "a1", "x2", "a2", "b"), "b": ("b",)}
            for arm, names in arms.items():
                def make(shp=shp, co=co, names=names):
                    return {k_: ints(("lin", shp, k_), shp if k_.startswith("x") else co, lim=2) for k_ in names}

                def stmt(t, absolute=False, shp=shp):
                    ref = torch.zeros(shp, dtype=next(iter(t.values())).dtype)
                    y = ref
                    for x_, a_ in (("x1", "a1"), ("x2", "a2")):
                        if x_ in t:
                            y = y + (t[x_] * _bcast(t[a_], ref) if a_ in t else t[x_])
                    if "b" in t:
                        y = y + _bcast(t["b"], ref)
                    return (y,)
                prod = lambda F, t, pc=pc, shp=shp: (F.NcLinFn.apply(t.get("x1"), t.get("a1"), t.get("x2"), t.get("a2"), t.get("b"), pc,
                                                                    None if "x1" in t else shp),)
                _add("nc_lin:c%d:%s:%s" % (c, "pc" if pc else "nc", arm), ["NcLinFn", "NcSumDotFn"], make, names, stmt, prod, order=2, lim=2)
    # the composites, real-valued
    for shp in NC_SHAPES:
        c, n = shp[-1], shp[0]
        norm_in = lambda shp=shp, c=c: {"x": reals(("cmp", shp, "x"), shp, 1.0, 0.15), "gamma": reals(("cmp", shp, "g"), (c,), 0.5, 1.0),
                                        "beta": reals(("cmp", shp, "b"), (c,), 0.1)}
        _add("instance_norm:c%d" % c, ["NcSumDotFn", "NcLinFn"], norm_in, ("x", "gamma", "beta"),
             lambda t, absolute=False: (O.instance_norm(t["x"], t["gamma"], t["beta"]),),
             lambda F, t: (F.instance_norm(t["x"], t["gamma"], t["beta"]),), order=2, exact=False)
        x_in = lambda shp=shp: {"x": reals(("cmp", shp, "x"), shp, 1.0, 0.15)}

        def style_stmt(t, absolute=False, n=n, c=c):
            mu, sd = O.layer_style(t["x"])
            return (torch.cat([mu.reshape(n, c), sd.reshape(n, c)], dim=1),)
        _add("layer_style:c%d" % c, ["NcSumDotFn", "NcLinFn"], x_in, ("x",), style_stmt, lambda F, t: (F.layer_style(t["x"]),), order=2, exact=False)
        _add("global_avg_pool:c%d" % c, ["NcSumDotFn", "NcLinFn"], x_in, ("x",),
             lambda t, absolute=False: (t["x"].mean(dim=tuple(range(1, t["x"].dim() - 1))),), lambda F, t: (F.global_avg_pool(t["x"]),),
             order=2, exact=False)
        ad_in = lambda shp=shp, n=n, c=c: {"x": reals(("cmp", shp, "x"), shp, 1.0, 0.15), "sb": reals(("cmp", shp, "sb"), (n, 2 * c), 0.5)}
        _add("adain_composite:c%d" % c, ["NcSumDotFn", "NcLinFn"], ad_in, ("x", "sb"), lambda t, absolute=False: (NR.adain(t["x"], t["sb"]),),
             lambda F, t: (F.adain_composite(t["x"], t["sb"]),), order=2, exact=False)


def _fused_cases():
    shp = (2, 6, 10, 8)
    c, n = shp[-1], shp[0]
    _add("adain:guard", ["AdaInFn"], lambda: {"x": reals("ad:x", shp, 1.0, 0.15), "sb": reals("ad:sb", (n, 2 * c), 0.5)}, ("x", "sb"),
         lambda t, absolute=False: (NR.adain(t["x"], t["sb"]),), lambda F, t: (F.adain(t["x"], t["sb"]),), order=1, exact=False, guard="raises",
         note=HELD["AdaInFn"])
    for shp in ((2, 6, 10, 8), (3, 5, 7, 6)):
        tail_in = lambda shp=shp: {"x": reals(("tail", shp, "x"), shp, 1.5, 0.2), "gamma": reals(("tail", shp, "g"), (shp[-1],), 0.5, 1.0),
                                   "beta": reals(("tail", shp, "b"), (shp[-1],), 0.1)}
        _add("discr_tail:nostyle:c%d" % shp[-1], ["DiscrTailFn"], tail_in, ("x", "gamma", "beta"),
             lambda t, absolute=False: (NR.tail(t["x"], t["gamma"], t["beta"], REAL_SLOPE)[0],),
             lambda F, t: (F.DiscrTailFn.apply(t["x"], t["gamma"], t["beta"], False, REAL_SLOPE)[0],), order=1, exact=False,
             guard="raises" if shp[-1] == 8 else None, note=ARMS_ELSEWHERE["DiscrTailFn"])
    for c in (8, 6):
        shp = (2, 5, 7, c)
        for relu in (False, True):
            for res in (False, True):
                def make(shp=shp, c=c, res=res):
                    # even scale and residual, odd offset: the ReLU's argument is an odd integer
                    t = {"x": ints(("caa", shp, "x"), shp), "a": ints(("caa", c, "a"), (c,), even=True), "b": ints(("caa", c, "b"), (c,), odd=True)}
                    if res:
                        t["res"] = ints(("caa", shp, "r"), shp, even=True)
                    return t

                def pre_(t):
                    v = t["x"] * t["a"] + t["b"]
                    return [v + t["res"] if "res" in t else v]
                stmt = lambda t, absolute=False, relu=relu: (_act(pre_(t)[0], ACT_RELU if relu else ACT_NONE, absolute),)
                prod = lambda F, t, relu=relu: (F.channel_affine_act(t["x"], t["a"], t["b"], t.get("res"), relu),)
                tag = "c%d:relu%d:res%d" % (c, relu, res)
                full = ("x", "a", "b") + (("res",) if res else ())
                _add("channel_affine_act:%s:full" % tag, ["ChannelAffineActFn"], make, full, stmt, prod, order=1, pre=pre_ if relu else None,
                     guard="raises" if (relu and res) else None, note="one pass at c = 8, separate passes at c = 6")
                if c == 8:
                    _add("channel_affine_act:%s:xonly" % tag, ["ChannelAffineActFn"], make, ("x",) + (("res",) if res else ()), stmt, prod, order=1,
                         pre=pre_ if relu else None, note="x alone requires grad: the separate passes")


def _pool_loss_cases():
    for k, s, pad in ((2, 2, 0), (3, 2, 1)):
        shp = (2, 7, 9, 6)
        make = lambda k=k, pad=pad: {"x": distinct(("pool", k), shp, positive=pad > 0)}
        _add("maxpool:k%ds%dp%d" % (k, s, pad), ["MaxPoolFn"], make, ("x",), lambda t, absolute=False, k=k, s=s, pad=pad: (O.maxpool(t["x"], k, s, pad),),
             lambda F, t, k=k, s=s, pad=pad: (F.maxpool(t["x"], k, s, pad),), order=2, guard="either",
             pools=lambda t, k=k, s=s, pad=pad: [(t["x"], k, s, pad)])
    off = (3.0, -2.0, 5.0)
    for perm in ((2, 1, 0), (0, 1, 2), (1, 2, 0)):
        _add("chan_affine3:%d%d%d" % perm, ["ChanAffine3Fn"], lambda: {"x": ints("ca3:x", (2, 5, 7, 3))}, ("x",),
             lambda t, absolute=False, perm=perm: (128.0 * t["x"][..., list(perm)] + (torch.tensor(off, dtype=t["x"].dtype).abs() if absolute
                                                                                      else torch.tensor(off, dtype=t["x"].dtype)),),
             lambda F, t, perm=perm: (F.ChanAffine3Fn.apply(t["x"], perm, 128.0, off),), order=2, guard="either")
    shp = (4, 3, 5, 8)
    ab = lambda: {"a": ints("sq:a", shp, lim=2), "b": ints("sq:b", shp, lim=2)}
    sq = lambda t, absolute: (t["a"] + t["b"]) ** 2 if absolute else (t["a"] - t["b"]) ** 2
    _add("sqdiff_sum", ["SqDiffSumFn"], ab, ("a",), lambda t, absolute=False: (0.125 * sq(t, absolute).sum(),),
         lambda F, t: (F.SqDiffSumFn.apply(t["a"], t["b"], 0.125),), order=2, guard="either", unit=0.125, lim=2)
    _add("mse_sum", ["SqDiffSumFn"], lambda: {"a": ints("sq:a", (4, 4, 8, 8), lim=2), "b": ints("sq:b", (4, 4, 8, 8), lim=2)}, ("a",),
         lambda t, absolute=False: (sq(t, absolute).mean(),), lambda F, t: (F.mse_sum(t["a"], t["b"]),), order=1, unit=1.0 / 1024, lim=2,
         note="1024 elements: the mean is a division by a power of two")
    shp5 = (5, 2, 4, 8)              # per = 64
    ab5 = lambda: {"a": ints("sqg:a", shp5, lim=2), "b": ints("sqg:b", shp5, lim=2)}

    def group_stmt(sizes):
        def stmt(t, absolute=False):
            d, outs, n0 = sq(t, absolute), [], 0
            for sz in sizes:
                outs.append(d[n0:n0 + sz].mean().reshape(1))
                n0 += sz
            return (torch.cat(outs),)
        return stmt
    _add("sqdiff_group:1,4", ["SqDiffGroupSumFn"], ab5, ("a",), group_stmt((1, 4)), lambda F, t: (F.mse_group_sums(t["a"], t["b"], (1, 4)),),
         order=2, guard="either", unit=1.0 / 256, lim=2)
    ab5r = lambda: {"a": reals("sqg:ra", shp5), "b": reals("sqg:rb", shp5)}
    _add("sqdiff_group:2,3", ["SqDiffGroupSumFn"], ab5r, ("a",), group_stmt((2, 3)), lambda F, t: (F.mse_group_sums(t["a"], t["b"], (2, 3)),),
         order=2, guard="either", exact=False, note="real-valued: the scale 1 / (3 * 64) is no power of two")
    rs = (5, 24)
    _add("row_sumsq", ["RowSumSqFn", "RowScaleFn"], lambda: {"x": ints("rss:x", rs, lim=2)}, ("x",),
         lambda t, absolute=False: ((t["x"] ** 2).sum(dim=1),), lambda F, t: (F.row_sumsq(t["x"]),), order=3, lim=2)
    _add("row_scale", ["RowScaleFn"], lambda: {"x": ints("rsc:x", rs, lim=2), "s": ints("rsc:s", (5,), lim=2)}, ("x", "s"),
         lambda t, absolute=False: (2.0 * t["x"] * t["s"].reshape(-1, 1),), lambda F, t: (F.RowScaleFn.apply(t["x"], t["s"], 2.0),), order=3, lim=2,
         note="the gradient to s included, and its own derivative")
    eye = (2, 6, 5, 3)

    def eye_in(real):
        def make():
            m = torch.from_numpy((_rng("eye:m").integers(0, 3, size=eye[:3]) > 0).astype(np.uint8))
            draw = reals if real else ints
            return {"gen": draw("eye:gen", eye), "gt": draw("eye:gt", eye), "mask": m}
        return make
    md = lambda t, absolute=False: ((t["gt"] + t["gen"] if absolute else t["gt"] - t["gen"]) * t["mask"].to(t["gen"].dtype).unsqueeze(-1),)
    _add("masked_diff", ["MaskedDiffFn"], eye_in(False), ("gen",), md, lambda F, t: (F.MaskedDiffFn.apply(t["gen"], t["gt"], t["mask"]),),
         order=2, guard="either")

    def eye_prod(F, t):
        from confignet_amd import losses
        return (losses.eye_loss(t["gt"], t["gen"], t["mask"]),)
    _add("eye_loss", ["MaskedDiffFn", "RowSumSqFn", "RowScaleFn"], eye_in(True), ("gen",),
         lambda t, absolute=False: (O.eye_loss(t["gt"], t["gen"], t["mask"]),), eye_prod, order=1, exact=False)
    for label in (1.0, 0.0):
        _add("gan_loss:%d" % label, ["GanLossFn"], lambda: {"s": reals("gan:s", (5, 3), 2.0)}, ("s",),
             lambda t, absolute=False, label=label: (O.gan_d_loss(label, t["s"]),), lambda F, t, label=label: (F.gan_loss(t["s"], label),),
             order=2, exact=False, guard="either")
    heads = ((5, 1), (5, 3), (2, 4), (7,))
    labels = (1.0, 0.0, 1.0, 0.0)
    hin = lambda: {"s%d" % i: reals(("gang", i), h, 2.0) for i, h in enumerate(heads)}
    hstmt = lambda t, absolute=False: tuple(O.gan_d_loss(labels[i], t["s%d" % i]) for i in range(len(heads)))
    hprod = lambda F, t: tuple(F.gan_losses([t["s%d" % i] for i in range(len(heads))], labels))
    for tag, used in (("all", (True,) * 4), ("unused2", (True, True, False, True))):
        _add("gan_loss_group:%s" % tag, ["GanLossGroupFn"], hin, ["s%d" % i for i in range(len(heads))], hstmt, hprod, order=2, exact=False,
             used=used, guard="either", note="heads of different shapes" + ("; head 2 unused" if tag != "all" else ""))
    lat = (6, 9)

    def gbm_prod(F, t):
        from confignet_amd import losses
        return losses.GlobalBatchMoments.apply(t["x"])
    for tag, used in (("both", (True, True)), ("mean", (True, False)), ("var", (False, True))):
        _add("global_batch_moments:%s" % tag, ["GlobalBatchMoments"], lambda: {"x": reals("gbm:x", lat, 1.0, 0.3)}, ("x",),
             lambda t, absolute=False: (t["x"].mean(dim=0), ((t["x"] - t["x"].mean(dim=0, keepdim=True)) ** 2).mean(dim=0)), gbm_prod,
             order=2, exact=False, used=used, note="one rank")

    def reg_prod(F, t):
        from confignet_amd import losses
        return (losses.normalized_latent_regression(t["out"], t["labels"], 0.5, global_statistics=True),)
    _add("normalized_latent_regression:global", ["GlobalBatchMoments"], lambda: {"out": reals("reg:o", lat), "labels": reals("reg:l", lat, 1.0, 0.3)},
         ("out", "labels"), lambda t, absolute=False: (regression_statement(t["out"], t["labels"], 0.5),), reg_prod, order=1, exact=False)


def _held_cases():
    """guards of the classes whose values another file holds: only that a second derivative raises"""
    g, c = 4, 4

    def rot_in():
        return {"grid": reals("rot:g", (1, g, g, g, c)), "angles": reals("rot:a", (1, 3), 0.3)}

    def rot_stmt(t, absolute=False):
        return (O.transform_3d_grid(t["grid"], O.euler_angles_to_matrix(t["angles"])),)
    _add("rotate3d:guard", ["Rotate3dFn", "EulerMatrixFn"], rot_in, ("grid", "angles"), rot_stmt, lambda F, t: (F.rotate3d(t["grid"], t["angles"]),),
         order=1, exact=False, guard="raises", note=HELD["Rotate3dFn"])
    _add("euler_matrix:guard", ["EulerMatrixFn"], lambda: {"angles": reals("eul:a", (2, 3), 0.3)}, ("angles",),
         lambda t, absolute=False: (O.euler_angles_to_matrix(t["angles"]),), lambda F, t: (F.euler_angles_to_matrix(t["angles"]),),
         order=1, exact=False, guard="raises", note=HELD["EulerMatrixFn"])


_conv_cases()
_dense_cases()
_act_nc_cases()
_fused_cases()
_pool_loss_cases()
_held_cases()

EXACT = [n for n, c in TABLE.items() if c.exact]
REAL = [n for n, c in TABLE.items() if not c.exact]
GUARDED = [n for n, c in TABLE.items() if c.guard is not None]


def classes_in_table():
    out = set(HELD)
    for c in TABLE.values():
        out.update(c.classes)
    return out


def function_classes():
    """every torch.autograd.Function subclass defined in confignet_amd/functional.py and confignet_amd/losses.py"""
    from confignet_amd import functional, losses
    out = set()
    for mod in (functional, losses):
        for name, obj in vars(mod).items():
            if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function and obj.__module__ == mod.__name__:
                out.add(name)
    return out


def pool_has_tie(x, k, s, pad):
    xc = x.permute(0, 3, 1, 2)
    if pad:
        xc = torch.nn.functional.pad(xc, [pad, pad, pad, pad])
    win = xc.unfold(2, k, s).unfold(3, k, s).reshape(*xc.shape[:2], -1, k * k)
    top = win.topk(2, dim=-1).values
    return bool((top[..., 0] == top[..., 1]).any())
