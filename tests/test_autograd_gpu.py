"""The autograd layer (confignet_amd/functional.py, GlobalBatchMoments of losses.py and the Python of ops.py they drive: grad_sink /
sink_for, bias_grad, upfold_prepare, the filter cache) against float64 statements, to the order each Function is used at and one
beyond.  Table, statements and bounds: tests/autograd_cases.py; the reference side is pinned on the CPU by
tests/test_autograd_cases_cpu.py.

  1. every case of the table through the same derivative ladder as its float64 statement: exact cases bit for bit, real-valued
     cases at MULT = 32 x their float32 yardstick (never above 2e-4 / 5e-4), in default and in deterministic mode;
  2. the guards: a Function whose backward is a raw kernel call either gives the right second derivative or raises -- a gradient
     that comes back without a graph (a silent zero one level up) fails;
  3. ConvFn's seven requires_grad subsets: what is asked for is exact, what is not asked for is None;
  4. the gradient sink, operand layouts, the filter cache.

What these tests exposed (all fixed in confignet_amd/functional.py with this file):
  * MaxPoolFn, ChanAffine3Fn, Rotate3dFn, SqDiffSumFn, SqDiffGroupSumFn, MaskedDiffFn, GanLossFn, GanLossGroupFn returned their
    kernels' results without a graph under create_graph=True: a second derivative through them was None instead of an error
    (test_a_second_derivative_is_right_or_refused).
  * EulerMatrixFn's guard, torch's once_differentiable, does not hold either: its error node has no edge to the inputs, so
    autograd.grad(..., allow_unused=True) and backward(inputs=...) never execute it and return None (same test, euler_matrix:guard
    and rotate3d:guard).  All nine now tie their results to the cotangents and saved inputs they came from by a node whose
    backward raises (functional._first_order_only), so the refusal is reached from every input.
  * the bias gradients of ConvFn and LinearFn (ops.bias_grad(gy.detach())) cut the graph the same way: d <gb, e> / d c was absent
    (test_exact_case_bit_for_bit: conv2:*:all, linear:bias).  Under create_graph they go through NcSumDotFn now; the first-order
    path is unchanged.
  * RowScaleFn's gradient to s came from ops.mul + a torch sum without a graph: its own derivative was absent
    (test_exact_case_bit_for_bit: row_scale, row_sumsq at order 3).  It goes through NcSumDotFn now.

Measured table (case x quantity x order x yardstick x bound x observed): profiles/autograd_errors.txt, written by this file when
AUTOGRAD_ERRORS names a path.  Extract (MI355X, default mode):
    case                                         quantity   order  yardstick      bound   observed
    instance_norm:c6                             d1/beta        1   1.83e-07   5.87e-06   1.04e-07
    instance_norm:c6                             d1/gamma       1   1.51e-07   4.83e-06   1.09e-07
    instance_norm:c6                             d1/x           1   1.25e-07   4.00e-06   2.09e-07
    instance_norm:c6                             d2/beta        2   0.00e+00   0.00e+00   0.00e+00
    instance_norm:c6                             d2/c0          2   1.25e-07   4.00e-06   1.42e-07
    instance_norm:c6                             d2/gamma       2   8.60e-08   2.75e-06   9.13e-08
    instance_norm:c6                             d2/x           2   1.02e-07   3.27e-06   1.60e-07
    instance_norm:c6                             y0             0   9.00e-08   2.88e-06   1.97e-07
    instance_norm:c8                             d1/beta        1   2.57e-08   8.22e-07   1.21e-07
    instance_norm:c8                             d1/gamma       1   5.53e-08   1.77e-06   1.94e-07
    instance_norm:c8                             d1/x           1   9.65e-08   3.09e-06   1.24e-07
    instance_norm:c8                             d2/beta        2   0.00e+00   0.00e+00   0.00e+00
    instance_norm:c8                             d2/c0          2   1.09e-07   3.49e-06   1.09e-07
    instance_norm:c8                             d2/gamma       2   4.79e-08   1.53e-06   1.26e-07
    instance_norm:c8                             d2/x           2   7.19e-08   2.30e-06   1.47e-07
    instance_norm:c8                             y0             0   1.26e-07   4.02e-06   1.69e-07
    layer_style:c8                               d1/x           1   1.27e-07   4.05e-06   1.96e-07
    layer_style:c8                               d2/c0          2   1.17e-07   3.75e-06   1.91e-07
    layer_style:c8                               d2/x           2   9.71e-08   3.11e-06   1.26e-07
    layer_style:c8                               y0             0   9.91e-08   3.17e-06   9.97e-08
    adain_composite:c6                           d1/sb          1   6.74e-08   2.16e-06   7.99e-08
    adain_composite:c6                           d1/x           1   6.13e-08   1.96e-06   1.28e-07
    adain_composite:c6                           d2/c0          2   9.29e-08   2.97e-06   1.57e-07
    adain_composite:c6                           d2/sb          2   1.19e-07   3.82e-06   2.18e-07
    adain_composite:c6                           d2/x           2   1.34e-07   4.28e-06   1.97e-07
    adain_composite:c6                           y0             0   7.43e-08   2.38e-06   1.17e-07
    global_avg_pool:c6                           d1/x           1   2.14e-08   6.84e-07   9.08e-08
    global_avg_pool:c6                           d2/c0          2   3.28e-08   1.05e-06   6.16e-08
    global_avg_pool:c6                           d2/x           2   0.00e+00   0.00e+00   0.00e+00
    global_avg_pool:c6                           y0             0   5.63e-08   1.80e-06   8.70e-08
    discr_tail:nostyle:c6                        d1/beta        1   1.24e-07   3.96e-06   1.39e-07
    discr_tail:nostyle:c6                        d1/gamma       1   2.22e-07   7.11e-06   2.28e-07
    discr_tail:nostyle:c6                        d1/x           1   1.25e-07   3.99e-06   9.41e-08
    discr_tail:nostyle:c6                        y0             0   1.55e-07   4.95e-06   9.35e-08
    gan_loss:1                                   d1/s           1   8.17e-08   2.61e-06   3.94e-08
    gan_loss:1                                   y0             0   3.48e-08   1.12e-06   6.89e-08
    gan_loss_group:unused2                       d1/s0          1   4.35e-08   1.39e-06   4.86e-08
    gan_loss_group:unused2                       d1/s1          1   5.66e-08   1.81e-06   5.28e-08
    gan_loss_group:unused2                       d1/s2          1   0.00e+00   0.00e+00   0.00e+00
    gan_loss_group:unused2                       d1/s3          1   5.11e-08   1.63e-06   1.30e-07
    gan_loss_group:unused2                       y0             0   1.30e-07   4.16e-06   1.29e-08
    gan_loss_group:unused2                       y1             0   1.30e-07   4.16e-06   5.50e-08
    gan_loss_group:unused2                       y2             0   1.30e-07   4.16e-06   5.09e-08
    gan_loss_group:unused2                       y3             0   1.30e-07   4.16e-06   7.28e-08
    eye_loss                                     d1/gen         1   6.61e-08   2.11e-06   6.61e-08
    eye_loss                                     y0             0   1.40e-08   4.47e-07   1.40e-08
    sqdiff_group:2,3                             d1/a           1   4.38e-08   1.40e-06   4.38e-08
    sqdiff_group:2,3                             y0             0   1.46e-08   4.68e-07   7.88e-08
    global_batch_moments:both                    d1/x           1   1.03e-07   3.28e-06   8.23e-08
    global_batch_moments:both                    d2/c0          2   3.57e-08   1.14e-06   4.54e-08
    global_batch_moments:both                    d2/c1          2   8.61e-08   2.76e-06   8.61e-08
    global_batch_moments:both                    d2/x           2   4.32e-08   1.38e-06   5.51e-08
    global_batch_moments:both                    y0             0   9.08e-08   2.91e-06   2.70e-08
    global_batch_moments:both                    y1             0   1.31e-07   4.19e-06   6.18e-08
    normalized_latent_regression:global          d1/labels      1   1.70e-07   5.43e-06   4.17e-07
    normalized_latent_regression:global          d1/out         1   1.38e-07   4.43e-06   2.82e-07
    normalized_latent_regression:global          y0             0   2.93e-08   9.37e-07   2.93e-08
    conv2:a:gx:quad:igo                          d1/x           1   0.00e+00   0.00e+00   0.00e+00
    conv2:a:gx:quad:igo                          d2/bias        2   0.00e+00   0.00e+00   0.00e+00
    conv2:a:gx:quad:igo                          d2/c0          2   0.00e+00   0.00e+00   0.00e+00
    conv2:a:gx:quad:igo                          d2/w           2   0.00e+00   0.00e+00   0.00e+00
    conv2:a:gx:quad:igo                          d2/x           2   0.00e+00   0.00e+00   0.00e+00
    conv2:a:gx:quad:igo                          y0             0   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               d1/b0          1   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               d1/b1          1   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               d1/w0          1   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               d1/w1          1   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               d1/x           1   0.00e+00   0.00e+00   0.00e+00
    mlp_r1:penalty                               y0             0   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d1/s           1   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d1/x           1   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d2/c0          2   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d2/s           2   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d2/x           2   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d3/c0          3   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d3/s           3   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    d3/x           3   0.00e+00   0.00e+00   0.00e+00
    row_scale                                    y0             0   0.00e+00   0.00e+00   0.00e+00
(966 rows; the 872 with bound 0 -- exact cases and identically zero quantities -- all observed 0; of the other 94 none above 0.17 of its bound: sqdiff_group:2,3 y0)"""
import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import autograd_cases as A
from tests import conv_edge_cases as CE

_ROWS = []
MODES = ["default", "deterministic"]


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("AUTOGRAD_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("%-44s %-10s %5s %10s %10s %10s\n" % ("case", "quantity", "order", "yardstick", "bound", "observed"))
            for r in _ROWS:
                f.write("%-44s %-10s %5d %10.2e %10.2e %10.2e\n" % r)


@pytest.fixture(params=MODES)
def mode(request):
    from confignet_amd import ops
    prev = ops.DETERMINISTIC
    ops.set_deterministic(request.param == "deterministic")
    try:
        yield request.param
    finally:
        ops.set_deterministic(prev)


def dev(v):
    return v.cuda() if v.dtype == torch.uint8 else v.to(torch.float32).cuda().contiguous()


def device_inputs(case):
    return {k: dev(v) for k, v in case.inputs().items()}


def run_product(case, order=None, t=None):
    from confignet_amd import functional as F
    t = device_inputs(case) if t is None else t
    return A.ladder(case, lambda t_: case.product(F, t_), t, dev, order, first_pass=F.input_grads_only if case.igo else None,
                    row_sumsq=F.row_sumsq)


@functools.lru_cache(maxsize=None)
def reference(name):
    case = A.TABLE[name]
    if case.exact:
        return A.reference(case), None
    return A.yardstick(case)


def _upto(q, order):
    return {k: v for k, v in q.items() if k.startswith("y") or int(k[1]) <= order}


def check(case, mode, rows=True):
    """The case's ladder on the device against its reference.  A guarded case whose last level raises is compared below it."""
    ref, yard = reference(case.name)
    order = case.order
    if case.guard == "either":
        try:
            got = run_product(case)
        except RuntimeError:
            order = 1
            got = run_product(case, order=1)
    else:
        got = run_product(case)
    fails = A.compare(case, got, _upto(ref, order), yard, _ROWS if (rows and mode == "default") else None)
    assert not fails, "%s (%s mode): %s" % (case.name, mode, "; ".join(fails))


# =============================================================================================================================
# 1. the table
# =============================================================================================================================
@pytest.mark.parametrize("name", [n for n in A.EXACT if A.TABLE[n].values])
def test_exact_case_bit_for_bit(name, mode):
    check(A.TABLE[name], mode)


@pytest.mark.parametrize("name", [n for n in A.REAL if A.TABLE[n].values])
def test_real_valued_case_at_its_yardstick_bound(name, mode):
    check(A.TABLE[name], mode)


@pytest.mark.parametrize("name", [n for n in A.EXACT if A.TABLE[n].values and len(A.TABLE[n].first) >= 2 and not n.startswith(("conv:", "mlp_r1:"))])
def test_each_input_alone_gets_its_gradient(name):
    """needs_input_grad: with ONE input requiring grad at a time, that input's first gradient is still the exact one (a backward
    that tests the wrong index returns None here).  ConvFn's subsets are section 3."""
    case = A.TABLE[name]
    ref, _ = reference(name)
    for k in case.first:
        one = copy.copy(case)
        one.diff = one.first = (k,)
        got = run_product(one, order=1)
        want = {q: v for q, v in ref.items() if q.startswith("y") or q == "d1/" + k}
        fails = A.compare(one, got, want)
        assert not fails, "%s with %s alone: %s" % (name, k, "; ".join(fails))


def test_collapsed_upsample_takes_the_collapsed_backward_at_first_order_only():
    """f and g: the first-order backward is the collapsed form (upfold_prepare's class filters), the backward under create_graph
    the generic one (ConvDgradFn / ConvWgradFn nodes) -- both exact above; here: that those ARE the two routes."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    for name in ("f", "g"):
        case = A.TABLE["conv:%s:none" % name]
        t = device_inputs(case)
        for k in ("x", "w"):
            t[k].requires_grad_(True)
        calls = []
        real = ops.upfold_prepare
        ops.upfold_prepare = lambda w, g: (calls.append(1), real(w, g))[1]
        try:
            y = case.product(F, t)[0]
            n_fwd = len(calls)
            gx, = torch.autograd.grad(y, t["x"], torch.ones_like(y), retain_graph=True)
            n_first = len(calls)
            gx2, = torch.autograd.grad(y, t["x"], torch.ones_like(y), create_graph=True)
            n_second = len(calls)
        finally:
            ops.upfold_prepare = real
        assert n_fwd == 1 and n_first == 2 and n_second == 2, (n_fwd, n_first, n_second)
        assert gx.grad_fn is None and type(gx2.grad_fn).__name__ == "ConvDgradFnBackward"
        assert torch.equal(gx, gx2.detach())


# =============================================================================================================================
# 2. guards
# =============================================================================================================================
@pytest.mark.parametrize("name", A.GUARDED)
def test_a_second_derivative_is_right_or_refused(name):
    """Take the gradient with create_graph=True, then differentiate a function of it: right against float64 (checked in section 1
    for the cases that are), or a RuntimeError -- never a silent zero, None or constant."""
    case = A.TABLE[name]
    if case.guard == "either":
        ref, yard = reference(name)
        try:
            got = run_product(case, order=2)
        except RuntimeError:
            return
        fails = A.compare(case, got, ref, yard)
        assert not fails, "%s: neither right nor refused: %s" % (name, "; ".join(fails))
        return
    with pytest.raises(RuntimeError):
        run_product(case, order=case.order + 1)


def test_fused_activation_conv_raises_the_documented_error():
    with pytest.raises(RuntimeError, match="double backward through a fused-activation conv is not supported"):
        run_product(A.TABLE["conv:a:lrelu"], order=2)


# =============================================================================================================================
# 3. requires_grad subsets
# =============================================================================================================================
SUBSETS = [s for s in ((x, w, b) for x in (0, 1) for w in (0, 1) for b in (0, 1)) if any(s)]


@pytest.mark.parametrize("act", ["none", "lrelu", "relu"])
@pytest.mark.parametrize("geom", A.CONV_GEOMS)
def test_conv_returns_what_is_asked_for_and_nothing_else(geom, act, mode):
    """the seven non-empty requires_grad subsets of (x, w, bias): each requested gradient exact, each unrequested one None -- from
    the tuple ConvFn.backward itself returns, and under input_grads_only the parameter gradients None as well."""
    from confignet_amd import functional as F
    case = A.TABLE["conv:%s:%s" % (geom, act)]
    ref, _ = reference(case.name)
    c = dev(A.cotangent(case, 1, 0, tuple(ref["y0"].shape), False))
    for subset in SUBSETS:
        t = device_inputs(case)
        for k, on in zip(("x", "w", "bias"), subset):
            t[k].requires_grad_(bool(on))
        y = case.product(F, t)[0]
        assert torch.equal(y.detach().cpu().double(), ref["y0"])
        with torch.no_grad():
            raw = y.grad_fn.apply(c)
            with F.input_grads_only():
                raw_igo = y.grad_fn.apply(c)
        assert len(raw) == 6 and all(r is None for r in raw[3:])
        for i, (k, on) in enumerate(zip(("x", "w", "bias"), subset)):
            if not on:
                assert raw[i] is None and raw_igo[i] is None, (subset, k)
                continue
            assert raw[i] is not None and torch.equal(raw[i].cpu().double(), ref["d1/" + k]), (subset, k)
            if k == "x":
                assert torch.equal(raw_igo[i], raw[i])
            else:
                assert raw_igo[i] is None, (subset, k)


# =============================================================================================================================
# 4. plumbing: the gradient sink, layouts, the filter cache
# =============================================================================================================================
SINK_CASES = {
    "conv:a:none": ("w", "bias"), "conv:a:lrelu": ("w", "bias"), "conv:g:none": ("w", "bias"), "conv:f:relu": ("w", "bias"),
    "linear:bias": ("w", "b"), "linear_act:lrelu": ("w", "b"),
    "mlp_bank:all": tuple(n % i for i in range(3) for n in ("w0_%d", "b0_%d", "w1_%d", "b1_%d")),
    "mlp_bank:unused1": tuple(n % i for i in range(3) for n in ("w0_%d", "b0_%d", "w1_%d", "b1_%d")),
}


@pytest.mark.parametrize("prefill", ["zeroed", "integers"])
@pytest.mark.parametrize("name", sorted(SINK_CASES))
def test_gradient_sink_holds_what_autograd_returns_without_one(name, prefill, mode):
    """Under ops.grad_sink(params) the weight and bias gradients autograd returns are None and the arena slots hold EXACTLY the
    gradients it returns without a sink (= the float64 ones), added to what the slots held before."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    case = A.TABLE[name]
    params = SINK_CASES[name]
    ref, _ = reference(name)
    t = device_inputs(case)
    for k in case.diff:
        t[k].requires_grad_(True)
    before = {}
    for k in params:
        before[k] = torch.zeros_like(t[k]) if prefill == "zeroed" else dev(A.ints(("sink", name, k), tuple(t[k].shape)))
        t[k].grad = before[k].clone()
    ys = case.product(F, t)
    live = [(j, y) for j, y in enumerate(ys) if case.used is None or case.used[j]]
    cots = [dev(A.cotangent(case, 1, j, tuple(y.shape), False)) for j, y in live]
    with ops.grad_sink([t[k] for k in params]):
        grads = torch.autograd.grad([y for _, y in live], [t[k] for k in case.diff], cots, allow_unused=True)
    torch.cuda.synchronize()
    for k, g in zip(case.diff, grads):
        r = ref["d1/" + k]
        if k in params:
            assert g is None, (name, k, "returned although the sink holds its slot")
            want = before[k].cpu().double() + (torch.zeros_like(before[k]).cpu().double() if r is None else r)
            assert torch.equal(t[k].grad.cpu().double(), want), (name, k)
        elif A.is_zero(r):
            assert A.is_zero(g), (name, k)
        else:
            assert torch.equal(g.cpu().double(), r), (name, k)


def _twin_grads(fn, leaves, make_operands):
    """outputs and gradients (w.r.t. the contiguous leaves) of fn(*make_operands(leaves)) with y.sum() as the loss"""
    ls = [l.clone().requires_grad_(True) for l in leaves]
    y = fn(*make_operands(ls))
    y.sum().backward()                      # the cotangent arrives expanded (stride 0)
    return [y.detach()] + [l.grad for l in ls]


def test_views_give_the_bits_of_their_contiguous_twins(mode):
    """x as a channel-slice view, w as a transposed view, the expanded cotangent of y.sum(): ConvFn, LinearFn, MatmulFn"""
    from confignet_amd import functional as F
    case = A.TABLE["conv:a:none"]
    t = device_inputs(case)
    spec = A._spec(CE.TABLE["a"])
    conv = lambda x, w, b: F.conv(x, w, b, spec)
    pad = lambda x: torch.cat([x, x.flip(-1)[..., :5]], dim=-1)                       # a wider tensor whose first channels are x
    plain = _twin_grads(conv, [t["x"], t["w"], t["bias"]], lambda ls: ls)
    views = _twin_grads(conv, [t["x"], t["w"], t["bias"]],
                        lambda ls: [pad(ls[0])[..., :ls[0].shape[-1]], ls[1].transpose(-1, -2).contiguous().transpose(-1, -2), ls[2]])
    ref, _ = reference("conv:a:none")
    assert torch.equal(plain[0].cpu().double(), ref["y0"])
    for a, b in zip(plain, views):
        assert torch.equal(a, b)
    case = A.TABLE["linear:bias"]
    t = device_inputs(case)
    lin = lambda x, w, b: F.linear(x, w, b)
    plain = _twin_grads(lin, [t["x"], t["w"], t["b"]], lambda ls: ls)
    views = _twin_grads(lin, [t["x"], t["w"], t["b"]], lambda ls: [pad(ls[0])[..., :ls[0].shape[-1]], ls[1].t().contiguous().t(), ls[2]])
    for a, b in zip(plain, views):
        assert torch.equal(a, b)
    assert torch.equal(plain[0].cpu().double(), reference("linear:bias")[0]["y0"])
    case = A.TABLE["matmul:10"]
    t = device_inputs(case)
    mm = lambda a, b: F.MatmulFn.apply(a, b, True, False)
    plain = _twin_grads(mm, [t["a"], t["b"]], lambda ls: ls)
    views = _twin_grads(mm, [t["a"], t["b"]], lambda ls: [ls[0].t().contiguous().t(), pad(ls[1])[..., :ls[1].shape[-1]]])
    for a, b in zip(plain, views):
        assert torch.equal(a, b)


@pytest.mark.parametrize("geom", ["g", "f", "a", "h"])
def test_filter_updated_in_place_is_derived_again(geom):
    """A free filter tensor changed in place (w.add_(1)): the collapsed route's class filters (g, f: upfold_prepare, forward and
    backward) and the tap-flipped copy of the data gradient (a, h: the library refuses cn_conv_dgrad_w there) are cached on the
    tensor and must be derived again -- results exact on the new values."""
    from confignet_amd import functional as F
    case = A.TABLE["conv:%s:none" % geom]
    assert (CE.plan_of(CE.TABLE[geom], "dgrad_w")[0] != 0) == (geom in ("a", "h"))
    t = device_inputs(case)
    t["x"].requires_grad_(True)
    c = None
    for step in range(2):
        y = case.product(F, t)[0]
        c = dev(A.cotangent(case, 1, 0, tuple(y.shape), False)) if c is None else c
        gx, = torch.autograd.grad(y, t["x"], c)
        t64 = {k: v.detach().cpu().double() for k, v in t.items()}
        t64["x"].requires_grad_(True)
        y64 = case.statement(t64)[0]
        gx64, = torch.autograd.grad(y64, t64["x"], c.cpu().double())
        assert torch.equal(y.detach().cpu().double(), y64.detach()), (geom, step)
        assert torch.equal(gx.cpu().double(), gx64), (geom, step)
        with torch.no_grad():
            t["w"].add_(1)
