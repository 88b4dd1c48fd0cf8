"""The bf16 filter gradient in deterministic mode (csrc/igemm_bf16.hip: igemm_bf16_wgrad_tr_kernel with a slab per row slice in the
stream's deterministic workspace; csrc/conv_dispatch.hip: run_conv_wgrad adds the slabs in slice order with cn_sum_parts).

Exact pass: the integer inputs of tests/wgrad_edge_cases.py -- the index logic of the slab epilogue (tile edges, the last slice, the
padding workgroups of the XCD-ordered grid, a slab nobody wrote) with no tolerance.  Slice-order pass: inputs whose result is a
function of the order of the cross-slice adds alone (tests/bf16_det_cases.py), held to the bits of the slice-order sum.  Rounding
pass: real values within the fp32 summation bound of tests/test_wgrad_edges_gpu.py, S = the slices."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import bf16_det_cases as B
from tests import test_wgrad_edges_gpu as G          # Guarded, the shared integer references, the rounding bound
from tests import wgrad_edge_cases as W

CASES = {**{n: W.TABLE[n] for n in W.BF16_TABLE}, "xcd-16": W.BF16_XCD[0], "xcd-22": W.BF16_XCD[1]}


@pytest.fixture(autouse=True)
def _deterministic():
    from confignet_amd import ops
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


@functools.lru_cache(maxsize=None)
def _exact(name):
    """(x, gy, float64 reference) on integer inputs: computed once, shared, never changed"""
    if name in W.TABLE:
        return G._exact(name)
    x, gy = W.integer_inputs(CASES[name], seed=17)
    return x, gy, W.reference(x, gy, CASES[name])


@functools.lru_cache(maxsize=None)
def _ordered(name):
    """(x, gy, float64 slice partials) on the order-sensitive inputs"""
    x, gy = B.order_inputs(CASES[name])
    return x, gy, B.slice_partials(x, gy, CASES[name])


def _bf16(t):
    return t.to(torch.bfloat16).cuda()


def _wgrad_bf16(g, x, gy, out, accumulate):
    from confignet_amd import ops
    ops.check(ops.lib.cn_conv_wgrad_bf16(ctypes.byref(g), ops._ptr(x), ops._ptr(gy), ops._fptr(out), int(accumulate), ops._stream()),
              "cn_conv_wgrad_bf16")


def _wgrad_dt(g, x, gy, out, mode):
    from confignet_amd import ops
    nbytes = ctypes.c_size_t(12345)
    ops.check(ops.lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), ops._dt(x), ops._dt(gy), ctypes.byref(nbytes)), "cn_conv_wgrad_dt_workspace_bytes")
    assert nbytes.value == 0          # the slabs live in the stream's workspace, never in the caller's
    ops.check(ops.lib.cn_conv_wgrad_dt(ctypes.byref(g), ops._ptr(x), ops._dt(x), ops._ptr(gy), ops._dt(gy), ops._fptr(out), mode, None, 0, None,
                                       ops._stream()), "cn_conv_wgrad_dt")


def test_the_cases_reach_every_arm_of_the_slab_epilogue():
    """From the slice rule and the tile rule by hand: one slice (no slab), more than one, the XCD-ordered grid with and without padding
    workgroups, a cout below the tile's width, a Ktot that is no multiple of the tile's rows -- and the plan reports the slab sum
    exactly where there is more than one slice."""
    seen = set()
    for name, case in CASES.items():
        g = W.geom(case)
        (slices, xcd), (bm, bn) = W.bf16_planned_splits(g), W.bf16_tile(g)
        rc, p = B.bf16_plan(g, 1)
        assert rc == 0 and p[0] == B.BF16_ROUTE and p[2] == slices and p[10] == (B.SUM_PARTS if slices > 1 else 0), (name, p)
        seen.add("one slice" if slices == 1 else "xcd" if xcd else "slices")
        if xcd and slices % 8:
            seen.add("padded grid")
        if g.cout < bn:
            seen.add("narrow cout")
        if W.ktot(g) % bm:
            seen.add("ragged Ktot")
    assert seen == {"one slice", "slices", "xcd", "padded grid", "narrow cout", "ragged Ktot"}, seen


def _exact_modes(name):
    """cn_conv_wgrad_bf16 (write, accumulate) and cn_conv_wgrad_dt (write, add, zeroed) on integer inputs: the float64 reference
    bit for bit, the guards around the gradient intact"""
    from confignet_amd import ops
    case = CASES[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, ref64 = _exact(name)
    x, gy, ref = _bf16(x64), _bf16(gy64), ref64.float().cuda()
    prior = G._prior(wshape, 5)
    assert bool((prior != 0).any())
    ref_added = (ref64 + prior.cpu().double()).float().cuda()
    gw = G.Guarded(ref.numel(), G.UNWRITTEN)
    out = gw.view.view(wshape)
    runs = [("bf16 write", lambda: _wgrad_bf16(g, x, gy, out, False), None, ref),
            ("bf16 accumulate", lambda: _wgrad_bf16(g, x, gy, out, True), prior, ref_added),
            ("dt write", lambda: _wgrad_dt(g, x, gy, out, ops.WGRAD_WRITE), None, ref),
            ("dt add", lambda: _wgrad_dt(g, x, gy, out, ops.WGRAD_ADD), prior, ref_added),
            ("dt zeroed", lambda: _wgrad_dt(g, x, gy, out, ops.WGRAD_ZEROED), torch.zeros_like(prior), ref)]
    for what, launch, before, want in runs:
        if before is None:
            out.fill_(G.UNWRITTEN)
        else:
            out.copy_(before)
        launch()
        assert torch.equal(out, want), "%s, %s: %s" % (name, what, G._wrong(out, want, g.cout))
        assert gw.intact(), "%s, %s: a guard was written" % (name, what)


@pytest.mark.parametrize("name", list(CASES))
def test_the_deterministic_bf16_filter_gradient_gives_the_integer_result(name):
    _exact_modes(name)


@pytest.mark.parametrize("name", ["xcd-16", "xcd-22"])
def test_the_slabs_are_added_in_slice_order(name):
    """The test of the mode itself: on the order-sensitive inputs the result has the bits of t = 0; t += p_0; ...; t += p_(S-1) in
    fp32, added to the cleared (write) or the prior (accumulate) gradient -- and not those of the reversed order, which differ in
    about half of the elements (tests/test_bf16_det_plan_cpu.py).  Atomics in the order the workgroups finish pass only if all 16 /
    22 slices land in slice order on every one of the 9 216 elements."""
    case = CASES[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, parts = _ordered(name)
    slices = len(parts)
    x, gy = _bf16(x64), _bf16(gy64)
    prior = B.order_prior(wshape)
    for what, before in (("write", None), ("accumulate", prior)):
        want = B.emulate(parts, range(slices), before)
        wrong = B.emulate(parts, reversed(range(slices)), before)
        out = torch.full(wshape, G.UNWRITTEN, device="cuda") if before is None else before.cuda()
        _wgrad_bf16(g, x, gy, out, before is not None)
        got = out.cpu()
        assert torch.equal(got, want), "%s, %s: %.0f %% of the elements are not the slice-order sum" % (name, what, 100 * B.fraction_different(got, want))
        assert B.fraction_different(got, wrong) >= 0.1, (name, what)


def test_no_stale_slab_is_read():
    """The workspace is never cleared: after a 22-slice launch has left partials of the order of 2^20 in it, a smaller filter
    with fewer slices on the same stream must still be exact -- every slab element its sum reads is one its own launch wrote."""
    big, small = CASES["xcd-22"], CASES["F"]
    gb, gs = W.geom(big), W.geom(small)
    (_, sb), (_, ss) = B.rows_and_slices(big), B.rows_and_slices(small)
    assert 1 < ss < sb and W.ktot(gs) * gs.cout < W.ktot(gb) * gb.cout
    xb, gyb = W.integer_inputs(big, seed=19)
    xb, gyb = torch.where(xb >= 0, 3.0, -3.0), torch.where(gyb >= 0, 3.0, -3.0) * 2.0 ** 20
    out = torch.zeros(W.filter_shape(big), device="cuda")
    _wgrad_bf16(gb, _bf16(xb), _bf16(gyb), out, False)
    assert float(out.abs().max()) >= 2.0 ** 20
    _exact_modes("F")


def test_the_same_bits_on_repetition_next_to_another_stream():
    """Three runs of the 22-slice case on one stream while a second stream -- with a workspace of its own -- runs fp32 deterministic
    filter gradients: identical, and equal to the slice-order sum."""
    from confignet_amd import ops
    name = "xcd-22"
    case = CASES[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, parts = _ordered(name)
    want = B.emulate(parts, range(len(parts)))
    x, gy = _bf16(x64), _bf16(gy64)
    other = W.TABLE["I"]
    go = W.geom(other)
    xo64, gyo64, refo = G._exact("I")
    xo, gyo = xo64.float().cuda(), gyo64.float().cuda()
    outs = [torch.full(wshape, G.UNWRITTEN, device="cuda") for _ in range(3)]
    outo = [torch.full(W.filter_shape(other), G.UNWRITTEN, device="cuda") for _ in range(3)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for out, oo in zip(outs, outo):
        with torch.cuda.stream(side):
            ops.check(ops.lib.cn_conv_wgrad(ctypes.byref(go), ops._ptr(xo), ops._ptr(gyo), ops._fptr(oo), 0, ops._stream()), "cn_conv_wgrad")
        _wgrad_bf16(g, x, gy, out, False)
    torch.cuda.synchronize()
    for i, (out, oo) in enumerate(zip(outs, outo)):
        assert torch.equal(out, outs[0]), "run %d differs from run 0 in %.0f %% of the elements" % (i, 100 * B.fraction_different(out, outs[0]))
        assert torch.equal(out.cpu(), want), "run %d: %.0f %% of the elements are not the slice-order sum" % (i, 100 * B.fraction_different(out.cpu(), want))
        assert torch.equal(oo.cpu().double(), refo), "the fp32 filter gradient of the second stream, run %d" % i


# ---- rounding pass ---------------------------------------------------------------------------------------------------------
_RATIOS = {}               # tile -> (largest error / bound, where)


def _note(kernel, tile, ratio, where):
    """tests/test_wgrad_edges_gpu.py's note, restated for the rows of this file: when WGRAD_EDGE_ERRORS names a path, the rows of
    `kernel` in that file's table are replaced by this run's (the other rows and the text around the table stay)."""
    if tile not in _RATIOS or not ratio <= _RATIOS[tile][0]:
        _RATIOS[tile] = (ratio, where)
    path = os.environ.get("WGRAD_EDGE_ERRORS")
    if not path:
        return
    head = "%-8s %-24s %10s   %s\n" % ("kernel", "tile", "ratio", "largest at")
    lines = open(path).readlines() if os.path.exists(path) else [head]
    lines = [ln for ln in lines if not ln.startswith(kernel + " ")]
    at = lines.index(head) + 1 if head in lines else len(lines)
    while at < len(lines) and lines[at].strip():
        at += 1
    lines[at:at] = ["%-8s %-24s %10.3e   %s\n" % (kernel, t, r, w) for t, (r, w) in sorted(_RATIOS.items())]
    with open(path, "w") as f:
        f.writelines(lines)


@pytest.mark.parametrize("name", [n for n in G.ROUNDING_SHAPES if n in W.BF16_TABLE])
def test_the_slab_sum_stays_within_the_fp32_summation_bound(name):
    """Standard-normal inputs rounded to bf16, added to a standard-normal prior value: |got - ref| <= 2 (M + S + 2) 2^-24 A with
    S = the slices whose slabs are added (the bound of tests/test_wgrad_edges_gpu.py, derived there)."""
    case = W.TABLE[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x, gy, ref, A = G._real(name, True)
    prior = torch.randn(wshape, generator=torch.Generator().manual_seed(31))
    out = prior.cuda()
    _wgrad_bf16(g, _bf16(x), _bf16(gy), out, True)
    slices = B.rows_and_slices(case)[1]
    assert slices == W.bf16_planned_splits(g)[0]
    r = G._ratio(out, ref, prior.double(), A, W.rows(g), slices)
    where = "%s, %d slices" % (name, slices)
    print("bf16-det %dx%d %s: error / bound %.3e" % (W.bf16_tile(g) + (where, r)))
    _note("bf16-det", "%dx%d" % W.bf16_tile(g), r, where)
    assert r <= 1.0, (where, r)
