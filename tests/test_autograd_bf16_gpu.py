"""The autograd layer in bf16 storage mode (ops.set_activation_dtype("bf16")) against float64 statements, bit for bit.  What is
under test is the Python of confignet_amd/ops.py that picks, per call, the kernel family and the places where a tensor changes storage
type, as the Functions of confignet_amd/functional.py drive it.  Table, roles, densities and the condition that makes every
comparison exact: tests/autograd_bf16_cases.py; proven case by case on the CPU by tests/test_autograd_bf16_cases_cpu.py.  Every
comparison here is torch.equal.

  1. every case of the table through the derivative ladder of its float64 statement, each operand placed in its role's storage
     type, in default and in deterministic mode; the level-0 outputs in the storage type the ops predicates give, parameter
     gradients in fp32;
  2. the convolution cases on the arm they are there for: the profile families of the forward, the data gradient and the filter
     gradient, and the storage conversions (ops.cast calls that change a type) of the first two;
  3. ConvFn's seven requires_grad subsets on a bf16-family and an image-layer geometry;
  4. the create_graph guards in bf16 mode;
  5. the gradient sink: arena slots with the bits autograd returns without one;
  6. the residual forms (ops.conv_fwd_res, ops.conv_dgrad_res: no Function wraps them) on their bf16-mode route, convolution +
     nc_lin2.

What these tests exposed: no defect -- every case held bit for bit in both modes on an MI355X when the file was added.  What they
notice (each tried once, as a change to ops.py / functional.py, and each failed the test named): the storage threshold moved from
4 to 8 channels (test_more_than_four_channels_are_stored_in_bf16); _unify preferring fp32 (test_bf16_case_bit_for_bit:
lrelu_mask_mul:fp32g, by its output's storage type); MIXED_FIRST_LAYERS off (test_convolution_case_runs_on_its_arm, image layers: the
families are the same as the fallback's, the conversions are not); the bias gradient of _bias_grad scaled by 1.01
(test_bf16_case_bit_for_bit on 40 cases, test_conv_returns_what_is_asked_for_and_nothing_else).  _bf16_conv_ok without its cout
clause was not run: cn_conv_fwd_bf16 refuses such a layer with CN_EUNSUPPORTED before it launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import autograd_bf16_cases as B
from tests import autograd_cases as A
from tests import conv_edge_cases as CE

BF16, F32 = torch.bfloat16, torch.float32
MODES = ["default", "deterministic"]


@pytest.fixture(autouse=True)
def _bf16_mode():
    """bf16 storage, and the Winograd thresholds as the fp32 tests shrink them: w2 / w4 would take F(2x2) / F(4x4) in fp32 mode"""
    from confignet_amd import ops
    keep = (ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS)
    ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS = 0, 0.0, 0
    ops.set_activation_dtype("bf16")
    try:
        yield
    finally:
        ops.set_activation_dtype("f32")
        ops.WINO_MIN_WGS, ops.WINO_MIN_FILL, ops.WINO4_MIN_WGS = keep


@pytest.fixture(params=MODES)
def mode(request):
    from confignet_amd import ops
    prev = ops.DETERMINISTIC
    ops.set_deterministic(request.param == "deterministic")
    try:
        yield request.param
    finally:
        ops.set_deterministic(prev)


def place(v, dtype):
    return v.cuda() if v.dtype == torch.uint8 else v.to(torch.float32).to(dtype).cuda().contiguous()


def device_inputs(case):
    st = B.input_storage(case)
    return {k: place(v, st[k]) for k, v in case.inputs().items()}


def run_product(case, order=None, t=None):
    from confignet_amd import functional as F
    outs = B.expected_storage(case)
    t = device_inputs(case) if t is None else t
    return A.ladder(case, lambda t_: case.product(F, t_), t, lambda v: place(v, F32), order, first_pass=F.input_grads_only if case.igo else None,
                    row_sumsq=F.row_sumsq, make_cot=lambda j, c: place(c, outs[j]))


def check(case, mode):
    ref = B.reference(case)
    got = run_product(case)
    fails = A.compare(case, got, ref)
    storage = B.quantity_storage(case)
    roles = B.roles(case)
    for k, v in got.items():
        if v is None:
            continue
        if k.startswith("y"):
            if v.dtype != storage[k]:
                fails.append("%s: stored as %s, the predicates say %s" % (k, v.dtype, storage[k]))
        elif roles.get(k.split("/", 1)[1]) == "parameter" and v.dtype != F32:
            fails.append("%s: a parameter gradient in %s" % (k, v.dtype))
    assert not fails, "%s (%s mode): %s" % (case.name, mode, "; ".join(fails))


# =============================================================================================================================
# 1. the table
# =============================================================================================================================
@pytest.mark.parametrize("name", list(B.TABLE))
def test_bf16_case_bit_for_bit(name, mode):
    check(B.TABLE[name], mode)


def test_more_than_four_channels_are_stored_in_bf16():
    """the rule itself, written out once (everything else asks ops._act_out_dtype): an offset broadcast to 6 and to 8 channels is a
    bf16 map, a convolution's 3-channel output and the gradient into a 3-channel image are fp32, a 48-channel output is bf16"""
    from confignet_amd import functional as F
    for name, want in (("nc_lin:c6:nc:b", BF16), ("nc_lin:c8:pc:b", BF16), ("conv:k3:none", F32), ("conv:e3s2:none", BF16), ("conv:k1:relu", F32)):
        case = B.TABLE[name]
        t = device_inputs(case)
        for k in case.diff:
            t[k].requires_grad_(True)
        y = case.product(F, t)[0]
        assert y.dtype == want, (name, y.dtype)
        if name == "conv:e3s2:none":
            gx, = torch.autograd.grad(y, t["x"], torch.ones_like(y))
            assert t["x"].dtype == F32 and gx.dtype == F32
    assert B.input_storage(B.TABLE["nc_sumdot:c6:nc:self:both"])["a"] == BF16 and B.input_storage(B.TABLE["conv:k1:none"])["x"] == BF16


# =============================================================================================================================
# 2. the arm a convolution case is there for
# =============================================================================================================================
class _count_casts:
    """counts the calls of ops.cast that change a storage type"""

    def __enter__(self):
        from confignet_amd import ops
        self.real, self.n = ops.cast, 0

        def cast(x, dtype):
            self.n += int(x.dtype != dtype)
            return self.real(x, dtype)
        ops.cast = cast
        return self

    def __exit__(self, *exc):
        from confignet_amd import ops
        ops.cast = self.real


def _families():
    from confignet_amd import ops
    torch.cuda.synchronize()
    got = set(ops.prof_collect_by_family())
    ops.prof_reset()
    return got


@pytest.mark.parametrize("name", B.CONV)
def test_convolution_case_runs_on_its_arm(name, mode):
    """forward, data gradient (x alone requires grad) and filter gradient (w alone) report the families B.expected_families derives
    from ops._bf16_conv_ok and the library's plans, and convert as often as B.expected_casts says: in bf16 mode nothing takes the
    fp32 Winograd launch (w2, w4), the bf16 family converts nothing, the fp32 family converts on each side, and an image layer on
    its own kernels converts nothing where the fp32 kernels of the same family would convert once"""
    from confignet_amd import functional as F
    from confignet_amd import ops
    case = B.TABLE[name]
    want, casts = B.expected_families(case), B.expected_casts(case)
    fused = not name.endswith(":none")
    ref = B.reference(case)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        for leaf, part in (("x", "dgrad"), ("w", "wgrad")):
            t = device_inputs(case)
            t[leaf].requires_grad_(True)
            with _count_casts() as fwd_casts:
                y = case.product(F, t)[0]
            assert _families() == {want["fwd"]} - {None}, (name, "forward")
            assert fwd_casts.n == casts["fwd"], (name, "forward", fwd_casts.n, casts["fwd"])
            c = place(A.cotangent(case, 1, 0, tuple(y.shape), False), y.dtype)
            with _count_casts() as bwd_casts:
                g, = torch.autograd.grad(y, t[leaf], c)
            assert _families() == {want[part]} - {None}, (name, part)
            assert torch.equal(g.cpu().double(), ref["d1/" + leaf]), (name, part)
            if part == "dgrad" and not fused:          # (a fused activation's backward may convert on its own: act_bwd's _unify)
                assert bwd_casts.n == casts["dgrad"], (name, "data gradient", bwd_casts.n, casts["dgrad"])
    finally:
        ops.prof_enable(False)


# =============================================================================================================================
# 3. requires_grad subsets
# =============================================================================================================================
SUBSETS = [s for s in ((x, w, b) for x in (0, 1) for w in (0, 1) for b in (0, 1)) if any(s)]


@pytest.mark.parametrize("act", ["none", "lrelu", "relu"])
@pytest.mark.parametrize("geom", ["c", "e3s2"])
def test_conv_returns_what_is_asked_for_and_nothing_else(geom, act, mode):
    """the seven non-empty requires_grad subsets of (x, w, bias) on a bf16-family and an image-layer geometry: each requested
    gradient exact, each unrequested one None, and under input_grads_only the parameter gradients None as well"""
    from confignet_amd import functional as F
    case = B.TABLE["conv:%s:%s" % (geom, act)]
    ref = B.reference(case)
    out = B.expected_storage(case)[0]
    c = place(A.cotangent(case, 1, 0, tuple(ref["y0"].shape), False), out)
    for subset in SUBSETS:
        t = device_inputs(case)
        for k, on in zip(("x", "w", "bias"), subset):
            t[k].requires_grad_(bool(on))
        y = case.product(F, t)[0]
        assert y.dtype == out and torch.equal(y.detach().cpu().double(), ref["y0"])
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
            assert raw[i].dtype == (t[k].dtype if k == "x" else F32), (subset, k, raw[i].dtype)
            if k == "x":
                assert torch.equal(raw_igo[i], raw[i])
            else:
                assert raw_igo[i] is None, (subset, k)


# =============================================================================================================================
# 4. guards
# =============================================================================================================================
GUARDED = [n for n, c in B.TABLE.items() if c.guard is not None]
REFUSAL = "first-order only|double backward through a fused-activation conv is not supported"


@pytest.mark.parametrize("name", GUARDED)
def test_a_second_derivative_is_refused_in_bf16_mode(name):
    """create_graph=True through a Function whose backward is a plain kernel call, then the derivative of the sum of its first
    gradients: the documented RuntimeError -- never None, never a value without a graph.  (The fp32 table's "either" cases all
    refuse today; a right second derivative would have to be added to the table with its statement.)"""
    from confignet_amd import functional as F
    case = B.TABLE[name]
    outs = B.expected_storage(case)
    t = device_inputs(case)
    for k in case.diff:
        t[k].requires_grad_(True)
    ys = case.product(F, t)
    live = [(j, y) for j, y in enumerate(ys) if y is not None and (case.used is None or case.used[j])]
    cots = [place(A.cotangent(case, 1, j, tuple(y.shape), False), outs[j]).requires_grad_(True) for j, y in live]
    with pytest.raises(RuntimeError, match=REFUSAL):
        gs = torch.autograd.grad([y for _, y in live], [t[k] for k in case.first], cots, create_graph=True, allow_unused=True)
        total = sum(g.float().sum() for g in gs if g is not None and g.requires_grad)
        got = torch.autograd.grad(total, [t[k] for k in case.diff] + cots, allow_unused=True)
        assert False, "%s: a second derivative came back: %s" % (name, [None if g is None else tuple(g.shape) for g in got])


# =============================================================================================================================
# 5. the gradient sink
# =============================================================================================================================
SINK_CASES = {"conv:c:none": ("w", "bias"), "conv:c:lrelu": ("w", "bias"), "conv:g:none": ("w", "bias"), "conv:e3s2:relu": ("w", "bias"),
              "linear:bias": ("w", "b")}


@pytest.mark.parametrize("prefill", ["zeroed", "integers"])
@pytest.mark.parametrize("name", sorted(SINK_CASES))
def test_gradient_sink_holds_the_bits_autograd_returns_without_one(name, prefill, mode):
    """under ops.grad_sink(params) autograd returns None for the filter / dense-weight and bias gradients and their arena slots
    hold exactly the float64 gradients, added to what they held before (small integers: the sums stay exact)"""
    from confignet_amd import functional as F
    from confignet_amd import ops
    case = B.TABLE[name]
    params = SINK_CASES[name]
    ref = B.reference(case)
    t = device_inputs(case)
    for k in case.diff:
        t[k].requires_grad_(True)
    before = {}
    for k in params:
        before[k] = torch.zeros_like(t[k]) if prefill == "zeroed" else place(A.ints(("sink", name, k), tuple(t[k].shape)), F32)
        t[k].grad = before[k].clone()
    y = case.product(F, t)[0]
    c = place(A.cotangent(case, 1, 0, tuple(y.shape), False), B.expected_storage(case)[0])
    with ops.grad_sink([t[k] for k in params]):
        grads = torch.autograd.grad([y], [t[k] for k in case.diff], [c], allow_unused=True)
    torch.cuda.synchronize()
    for k, g in zip(case.diff, grads):
        if k in params:
            assert g is None, (name, k, "returned although the sink holds its slot")
            assert t[k].grad.dtype == F32 and torch.equal(t[k].grad.cpu().double(), before[k].cpu().double() + ref["d1/" + k]), (name, k)
        else:
            assert g.dtype == t[k].dtype and torch.equal(g.cpu().double(), ref["d1/" + k]), (name, k)


# =============================================================================================================================
# 6. the residual forms
# =============================================================================================================================
@pytest.mark.parametrize("geom", B.RES_GEOMS)
def test_residual_forms_fall_back_to_convolution_and_one_pass(geom, mode):
    """ops.conv_fwd_res / ops.conv_dgrad_res in bf16 mode: the fp32 epilogue launches are not taken (their families do not show),
    the result is relu(conv + bias + res) and dgrad + res bit for bit, in the storage type of the convolution's result"""
    from confignet_amd import ops
    case, inp = B.GEOMS[geom], B.res_inputs(geom)
    g = CE.geom(case)
    with B.bf16_mode():
        in_dt, out_dt = ops._act_out_dtype(g.cin), ops._act_out_dtype(g.cout)
        fam = {B.fwd_arm(g, True, ops.ACT_NONE, in_dt)[0], B.dgrad_arm(g, out_dt)[0]} - {None}
    d = {k: place(v, {"x": in_dt, "res": out_dt, "gy": out_dt, "resx": in_dt}.get(k, F32)) for k, v in inp.items()}
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        y = ops.conv_fwd_res(d["x"], d["w"], d["bias"], d["res"], g, ops.ACT_RELU)
        gu = ops.conv_dgrad_res(d["gy"], d["w"], g, d["resx"])
        assert _families() == fam, geom
    finally:
        ops.prof_enable(False)
    assert y.dtype == out_dt and gu.dtype == in_dt
    assert torch.equal(y.cpu().double(), CE.reference(case, "res", inp)), geom
    assert torch.equal(gu.cpu().double(), CE.reference(case, "dgrad_w_res", inp)), geom
