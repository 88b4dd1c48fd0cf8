"""Every tile, stage count, grid layout and slice plan of the filter gradient (csrc/wgrad2.hip), the bf16 filter gradient and the
other routes of ops.conv_wgrad, on the edge geometries of tests/wgrad_edge_cases.py.

Exact pass: integer inputs in [-3, 3].  Every product and partial sum is an integer fp32 holds exactly (9 M < 2^24) in any order of
the adds, so each result is compared with the float64 reference by torch.equal -- no tolerance: one dropped or doubled reduction
row, one wrong padding tap, one slice that ends a row early shows as a whole number.  Tile and workgroup target are forced through
cn_conv_tune, the stage count through cn_conv_loop_select; the profile must show the forced tile's family, the plan the slice count
tests/test_wgrad_edge_cases_cpu.py derives, and the 256 floats in front of and behind the gradient and the workspace (views into
larger allocations) must keep their sentinel.

Rounding pass: what integers cannot show, the accumulate arithmetic on real values.  Standard-normal inputs (rounded to bf16 first
for the bf16 kernel, reference on the rounded values); fp32 accumulation in any order of M products plus S slab (or atomic) adds,
plus at most two more adds for a prior value and an atomic, stays within
    |got - ref|_ij <= 2 (M + S + 2) 2^-24 A_ij,      A = the float64 filter gradient of |x| and |gy|
(the factor 2 allows for truncating intermediate rounding inside the MFMA).  The bound is derived, not tuned; the largest observed
error / bound per tile is in profiles/wgrad_edge_errors.txt, written by this file when WGRAD_EDGE_ERRORS names a path."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import wgrad_edge_cases as W

GUARD = 256                # floats in front of and behind a guarded view (1 KB: the view keeps the allocation's alignment)
GUARD_VALUE = 12345.0
UNWRITTEN = -7777.0        # what a tensor the kernel must WRITE holds before the launch


class Guarded:
    """`n` floats inside a larger allocation, 256 sentinel floats on both sides"""

    def __init__(self, n, fill):
        self.buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, device="cuda", dtype=torch.float32)
        self.view = self.buf[GUARD:GUARD + n]
        self.view.fill_(fill)
        self.want = torch.full((GUARD,), GUARD_VALUE, device="cuda", dtype=torch.float32)

    def intact(self):
        return torch.equal(self.buf[:GUARD], self.want) and torch.equal(self.buf[GUARD + self.view.numel():], self.want)


@functools.lru_cache(maxsize=None)
def _exact(name):
    """(x, gy, float64 reference) of a geometry on integer inputs: computed once, shared by the tests that need it, never changed"""
    case = W.TABLE[name] if name in W.TABLE else {r[0]: r[1] for r in W.ROUTING}[name]
    x, gy = W.integer_inputs(case, seed=11 + sum(case[0]) + case[2])
    return x, gy, W.reference(x, gy, case)


def _wrong(got, ref, cout):
    """which (filter row, output channel) elements differ and by how many whole products"""
    d = (got.double() - ref.double()).reshape(-1, cout).cpu()
    bad = d.nonzero()
    head = ", ".join("(%d, %d): %+g" % (int(r), int(c), float(d[r, c])) for r, c in bad[:8])
    rws, cls = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, 1].tolist()))
    return "%d of %d elements wrong; rows %s..%s (%d), columns %s..%s (%d); first: %s" % (
        len(bad), d.numel(), rws[0], rws[-1], len(rws), cls[0], cls[-1], len(cls), head)


def _prior(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-5, 6, shape, generator=gen).float().cuda()


def _families(shown):
    return {name: v["launches"] for name, v in shown.items()}


@pytest.mark.parametrize("name", list(W.TABLE))
def test_every_tile_stage_count_and_slice_plan_gives_the_integer_result(name):
    """Five tiles x three / four stages x five workgroup targets, each into a fresh tensor, added to a tensor of small integers
    (one slice: the atomic-add epilogue; more: the accumulate of the slab reduction) and written over a sentinel."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = W.TABLE[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, ref64 = _exact(name)
    x, gy, ref = x64.float().cuda(), gy64.float().cuda(), ref64.float().cuda()
    count = ref.numel()
    prior = _prior(wshape, 3)
    ref_added = (ref64 + prior.cpu().double()).float().cuda()
    gw = Guarded(count, UNWRITTEN)
    out = gw.view.view(wshape)
    classes = set()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        for tile in W.TILES:
            for ns in W.STAGES:
                ops.check(lib.cn_conv_loop_select(-1, 0, ns, -1), "cn_conv_loop_select")
                for want in W.WANTS:
                    ops.check(lib.cn_conv_tune(tile[0], 0, want * W.tiles_of(g, tile)), "cn_conv_tune")
                    what = "%s %s stages %s want %d" % (name, tile[1], ns or "default", want)
                    splits = W.planned_splits(g)
                    assert splits == W.replayed_splits(g, tile, want), what
                    classes.add(W.split_class(splits))
                    what += " (%d slices)" % splits
                    slabs = splits * count if splits > 1 else 0
                    ws = Guarded(max(slabs, GUARD), float("nan"))        # (an element of a slab nobody wrote poisons the sum)
                    ops.prof_reset()
                    got = ops.conv_wgrad(x, gy, g, wshape)
                    assert torch.equal(got, ref), what + ", fresh tensor: " + _wrong(got, ref, g.cout)
                    out.copy_(prior)
                    ops.conv_wgrad(x, gy, g, wshape, out=out, accumulate=True, ws=ws.view)
                    assert torch.equal(out, ref_added), what + ", accumulate: " + _wrong(out, ref_added, g.cout)
                    assert gw.intact() and ws.intact(), what + ", accumulate: a guard was written"
                    out.fill_(UNWRITTEN)
                    ws.view.fill_(float("nan"))
                    ops.conv_wgrad(x, gy, g, wshape, out=out, accumulate=False, ws=ws.view)
                    assert torch.equal(out, ref), what + ", write: " + _wrong(out, ref, g.cout)
                    assert gw.intact() and ws.intact(), what + ", write: a guard was written"
                    assert bool(torch.isnan(ws.view[slabs:]).all()), what + ": the workspace was written past its slabs"
                    torch.cuda.synchronize()
                    assert _families(ops.prof_collect_by_family()) == {tile[1]: 3}, what
    finally:
        ops.prof_enable(False)
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    print(name, "split classes", sorted(classes))


@pytest.mark.parametrize("name", [r[0] for r in W.ROUTING] + list(W.TABLE))
def test_the_default_plan_and_the_routing_boundaries_give_the_integer_result(name):
    """The default heuristic on the geometries next to a routing boundary of ops.conv_wgrad: the atomic kernel (Ktot < 64,
    cin % 4 != 0, cout <= 4 on wide inputs, a K = 27 layer past that route's cout limit), the thin route and the K = 27 route --
    the kernel that takes the call is the one the profile shows -- and on the table itself, where the cost model of cn_wgrad2_plan
    picks tile and slices (whichever tile of csrc/wgrad2.hip: the same one for the three calls)."""
    from confignet_amd import ops
    case, families = (W.TABLE[name], None) if name in W.TABLE else {r[0]: r for r in W.ROUTING}[name][1:]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, ref64 = _exact(name)
    x, gy, ref = x64.float().cuda(), gy64.float().cuda(), ref64.float().cuda()
    prior = _prior(wshape, 4)
    ref_added = (ref64 + prior.cpu().double()).float().cuda()
    gw = Guarded(ref.numel(), UNWRITTEN)
    out = gw.view.view(wshape)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        got = ops.conv_wgrad(x, gy, g, wshape)
        assert torch.equal(got, ref), "fresh tensor: " + _wrong(got, ref, g.cout)
        out.copy_(prior)
        ops.conv_wgrad(x, gy, g, wshape, out=out, accumulate=True)
        assert torch.equal(out, ref_added), "accumulate: " + _wrong(out, ref_added, g.cout)
        assert gw.intact(), "accumulate: a guard was written"
        out.fill_(UNWRITTEN)
        ops.conv_wgrad(x, gy, g, wshape, out=out, accumulate=False)
        assert torch.equal(out, ref), "write: " + _wrong(out, ref, g.cout)
        assert gw.intact(), "write: a guard was written"
        torch.cuda.synchronize()
        shown = _families(ops.prof_collect_by_family())
        print(name, shown)
        if families is None:
            assert len(shown) == 1 and set(shown) <= {t[1] for t in W.TILES} and set(shown.values()) == {3}, shown
        else:
            assert shown == {k: 3 * v for k, v in families.items()}
    finally:
        ops.prof_enable(False)


def _bf16_wgrad(g, x, gy, out, accumulate):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    ops.check(lib.cn_conv_wgrad_bf16(ctypes.byref(g), ops._ptr(x), ops._ptr(gy), ops._fptr(out), int(accumulate), ops._stream()),
              "cn_conv_wgrad_bf16")


def _bf16_exact(case, x64, gy64, ref64):
    from confignet_amd import ops
    g, wshape = W.geom(case), W.filter_shape(case)
    x, gy, ref = x64.to(torch.bfloat16).cuda(), gy64.to(torch.bfloat16).cuda(), ref64.float().cuda()
    assert torch.equal(x.double().cpu(), x64)                  # (integers up to 3 are exact in bf16)
    prior = _prior(wshape, 5)
    ref_added = (ref64 + prior.cpu().double()).float().cuda()
    gw = Guarded(ref.numel(), UNWRITTEN)
    out = gw.view.view(wshape)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        _bf16_wgrad(g, x, gy, out, False)
        assert torch.equal(out, ref), "write: " + _wrong(out, ref, g.cout)
        assert gw.intact(), "write: a guard was written"
        out.copy_(prior)
        _bf16_wgrad(g, x, gy, out, True)
        assert torch.equal(out, ref_added), "accumulate: " + _wrong(out, ref_added, g.cout)
        assert gw.intact(), "accumulate: a guard was written"
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == {"igemm_bf16_wgrad": 2}
    finally:
        ops.prof_enable(False)


@pytest.mark.parametrize("name", W.BF16_TABLE)
def test_the_bf16_filter_gradient_gives_the_integer_result(name):
    """cn_conv_wgrad_bf16 (its own tiles, slice rule and fp32 atomics) on every table geometry it takes"""
    _bf16_exact(W.TABLE[name], *_exact(name))


@pytest.mark.parametrize("case", W.BF16_XCD, ids=["16-slices", "22-slices"])
def test_the_bf16_filter_gradient_on_its_xcd_ordered_grid(case):
    """Three 128x32 tiles (Ktot = 288, cout = 32) and a reduction long enough for the bf16 kernel's own slice rule to take the
    XCD-ordered 1-D grid (more than one tile, >= 16 slices).  The rule (target 2560 workgroups / 3 tiles, at most M / 512 slices,
    at least min(M / 256, 86) = one workgroup per CU, rounded down to a multiple of 8 from 16 up; rows per slice rounded up to 32):
      (16, 16, 16, 32): M = 4096 -> 16 slices of 256 rows: a grid of 2 x 8 x 3 workgroups, none of them padding;
      (31, 10, 20, 32): M = 6200 -> 24 asked for, 288 rows each -> 22 slices in a grid padded to 24: six workgroups must leave,
                        and the last slice has 152 rows.
    tests/test_wgrad_edge_cases_cpu.py holds the two counts against the rule."""
    assert W.bf16_planned_splits(W.geom(case)) == ((16, True) if case[0][0] == 16 else (22, True))
    x, gy = W.integer_inputs(case, seed=17)
    _bf16_exact(case, x, gy, W.reference(x, gy, case))


def _routed(g, x, gy, out, mode, ws):
    """cn_conv_wgrad_dt with the workspace its own query asks for, taken from the guarded allocation `ws`"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    nbytes = ctypes.c_size_t(0)
    ops.check(lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), ops._dt(x), ops._dt(gy), ctypes.byref(nbytes)), "cn_conv_wgrad_dt_workspace_bytes")
    assert nbytes.value <= 4 * ws.view.numel()
    ops.check(lib.cn_conv_wgrad_dt(ctypes.byref(g), ops._ptr(x), ops._dt(x), ops._ptr(gy), ops._dt(gy), ops._fptr(out), mode,
                                   ops._ptr(ws.view) if nbytes.value else None, nbytes.value, None, ops._stream()), "cn_conv_wgrad_dt")
    return nbytes.value // 4


@pytest.mark.parametrize("name", [r[0] for r in W.ROUTING] + list(W.TABLE) + ["bf16-" + n for n in W.BF16_TABLE] + ["k27-bf16-gy"])
def test_the_routed_entry_gives_the_integer_result(name):
    """cn_conv_wgrad_dt itself -- every route behind one call -- on the routing boundaries, the table and, with bf16 operands, the
    table entries the bf16 kernel takes (and the K = 27 layer with a bf16 gy next to the fp32 image): written over a sentinel,
    added to small integers, and added to a target the caller declares zero, each equal to the float64 reference bit for bit; the
    guards around the gradient and the workspace keep their sentinel and the workspace is not written past what the query asked for."""
    from confignet_amd import ops
    bf16 = name.startswith("bf16-")
    base = "k27" if name == "k27-bf16-gy" else name[5:] if bf16 else name
    case = W.TABLE[base] if base in W.TABLE else {r[0]: r[1] for r in W.ROUTING}[base]
    g, wshape = W.geom(case), W.filter_shape(case)
    x64, gy64, ref64 = _exact(base)
    x = x64.to(torch.bfloat16 if bf16 else torch.float32).cuda()
    gy = gy64.to(torch.bfloat16 if bf16 or name == "k27-bf16-gy" else torch.float32).cuda()
    ref = ref64.float().cuda()
    prior = _prior(wshape, 6)
    ref_added = (ref64 + prior.cpu().double()).float().cuda()
    gw = Guarded(ref.numel(), UNWRITTEN)
    out = gw.view.view(wshape)
    nbytes = ctypes.c_size_t(0)
    ops.check(ops.lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), ops._dt(x), ops._dt(gy), ctypes.byref(nbytes)), "cn_conv_wgrad_dt_workspace_bytes")
    ws = Guarded(max(nbytes.value // 4, GUARD) + GUARD, float("nan"))
    for mode, before, want in ((ops.WGRAD_WRITE, None, ref), (ops.WGRAD_ADD, prior, ref_added), (ops.WGRAD_ZEROED, torch.zeros_like(prior), ref)):
        what = "%s mode %d" % (name, mode)
        if before is None:
            out.fill_(UNWRITTEN)
        else:
            out.copy_(before)
        ws.view.fill_(float("nan"))
        used = _routed(g, x, gy, out, mode, ws)
        assert torch.equal(out, want), what + ": " + _wrong(out, want, g.cout)
        assert gw.intact() and ws.intact(), what + ": a guard was written"
        assert bool(torch.isnan(ws.view[used:]).all()), what + ": the workspace was written past what the query asked for"


# ---- rounding pass ---------------------------------------------------------------------------------------------------------
ROUNDING_SHAPES = ("D", "F", "I")
_RATIOS = {}               # (kernel, tile) -> (largest error / bound, where)


@functools.lru_cache(maxsize=None)
def _real(name, bf16):
    """(x, gy, float64 reference, A) on standard-normal inputs drawn in fp32 (rounded to bf16 for the bf16 kernel)"""
    case = W.TABLE[name]
    gen = torch.Generator().manual_seed(23 + sum(case[0]))
    x = torch.randn(case[0], generator=gen)
    gy = torch.randn(W.ops.geom_out_shape(W.geom(case)), generator=gen)
    if bf16:
        x, gy = x.to(torch.bfloat16).float(), gy.to(torch.bfloat16).float()
    return x, gy, W.reference(x.double(), gy.double(), case), W.reference(x.double().abs(), gy.double().abs(), case)


def _ratio(got, ref, prior, A, m, s):
    """largest |got - (prior + ref)| / bound over the elements, bound = 2 (M + S + 2) 2^-24 A"""
    assert bool((prior.abs() <= A).all())      # (the prior value is one of the "+ 2" adds: it must not outweigh the sum it joins)
    err = (got.double().cpu() - (ref + prior)).abs()
    return float((err / (2.0 * (m + s + 2) * 2.0 ** -24 * A)).max())


def _note(kernel, tile, ratio, where):
    if (kernel, tile) not in _RATIOS or not ratio <= _RATIOS[(kernel, tile)][0]:
        _RATIOS[(kernel, tile)] = (ratio, where)
    path = os.environ.get("WGRAD_EDGE_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("Rounding pass of tests/test_wgrad_edges_gpu.py, one MI355X (written when WGRAD_EDGE_ERRORS names a path): standard-normal\n"
                    "inputs on the shapes D, F and I of tests/wgrad_edge_cases.py, added to a standard-normal prior value, one launch per tile and\n"
                    "split class.  ratio = the largest |got - ref|_ij / (2 (M + S + 2) 2^-24 A_ij) over the elements of every launch of the tile\n"
                    "(A = float64 filter gradient of |x| and |gy|, S = slab or atomic adds); the test holds every ratio at <= 1.\n\n")
            f.write("%-8s %-24s %10s   %s\n" % ("kernel", "tile", "ratio", "largest at"))
            for (k, t), (r, w) in sorted(_RATIOS.items()):
                f.write("%-8s %-24s %10.3e   %s\n" % (k, t, r, w))


@pytest.mark.parametrize("name", ROUNDING_SHAPES)
def test_the_accumulate_arithmetic_stays_within_the_fp32_summation_bound(name):
    """One launch per tile and split class the shape reaches, added to a prior value of real numbers."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = W.TABLE[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x, gy, ref, A = _real(name, False)
    xd, gyd = x.cuda(), gy.cuda()
    prior = torch.randn(wshape, generator=torch.Generator().manual_seed(29))
    over = []
    try:
        for tile in W.TILES:
            seen = set()
            for want in W.WANTS:
                ops.check(lib.cn_conv_tune(tile[0], 0, want * W.tiles_of(g, tile)), "cn_conv_tune")
                splits = W.planned_splits(g)
                if W.split_class(splits) in seen:
                    continue
                seen.add(W.split_class(splits))
                out = prior.cuda()
                ops.conv_wgrad(xd, gyd, g, wshape, out=out, accumulate=True)
                r = _ratio(out, ref, prior.double(), A, W.rows(g), splits if splits > 1 else 0)
                where = "%s, %d slices" % (name, splits)
                print("%s %s: error / bound %.3e" % (tile[1], where, r))
                _note("fp32", tile[1], r, where)
                if not r <= 1.0:
                    over.append((tile[1], where, r))
    finally:
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    assert not over, over


@pytest.mark.parametrize("name", [n for n in ROUNDING_SHAPES if n in W.BF16_TABLE])
def test_the_bf16_accumulate_arithmetic_stays_within_the_fp32_summation_bound(name):
    """bf16 products are exact in fp32 and the accumulation is fp32: the same bound, with S = the atomic adds of the row slices."""
    case = W.TABLE[name]
    g, wshape = W.geom(case), W.filter_shape(case)
    x, gy, ref, A = _real(name, True)
    prior = torch.randn(wshape, generator=torch.Generator().manual_seed(31))
    out = prior.cuda()
    _bf16_wgrad(g, x.to(torch.bfloat16).cuda(), gy.to(torch.bfloat16).cuda(), out, True)
    splits = W.bf16_planned_splits(g)[0]
    r = _ratio(out, ref, prior.double(), A, W.rows(g), splits)
    where = "%s, %d slices" % (name, splits)
    print("bf16 %dx%d %s: error / bound %.3e" % (W.bf16_tile(g) + (where, r)))
    _note("bf16", "%dx%d" % W.bf16_tile(g), r, where)
    assert r <= 1.0, (where, r)
