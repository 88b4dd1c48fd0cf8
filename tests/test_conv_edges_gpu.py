"""Every route, tile, K split, main loop and epilogue of the forward convolution and the data gradient (csrc/conv_dispatch.hip:
plan_conv_fwd / run_conv_fwd and the kernels behind them), Winograd, the bf16 family and the upsample-folded path, on the edge
geometries of tests/conv_edge_cases.py, through the C ABI.

Exact pass: integer inputs in [-3, 3].  Every product and partial sum is an integer fp32 holds exactly (A < 2^24,
tests/test_conv_edge_cases_cpu.py) in any order of the adds, so each result is compared with the float64 reference by torch.equal --
no tolerance: one wrong padding tap, one dropped K step, one slice that ends early shows as a whole number.  Every output is a view
into a larger allocation, pre-filled with a sentinel, 256 sentinel floats in front of it and behind it: a partial tile, a zero
pass, an atomic tile or a wide store that leaves the output is seen.  With profiling on, the family the plan names -- and nothing
else -- must have launched.  Tile and split are forced through cn_conv_tune, the main loop through cn_conv_loop_select.

Rounding pass: what integers cannot show, the accumulate arithmetic on real values.  Standard-normal inputs; fp32 accumulation of
K products in any order plus S slice adds plus the bias stays within
    |got - ref| <= 2 (K + S + 2) 2^-24 A,      A = the float64 convolution of |x| and |w| plus |bias|
(the factor 2 allows for truncating intermediate rounding inside the MFMA).  The bound is derived, not tuned; the largest observed
error / bound per kernel and tile is in profiles/conv_edge_errors.txt, written once at the end of this file's run when CONV_EDGE_ERRORS names a path (with the
exact-launch counts of that process: the committed record is from a run of the whole file)."""
import collections
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_edge_cases as C
from tests import test_conv_plan_cpu as P
from tests.test_ops_gpu import LOOP_VARIANTS, UPFOLD_CASES
from tests.test_wgrad_edges_gpu import GUARD, UNWRITTEN, Guarded, _wrong

CN_F32, CN_BF16 = P.CN_F32, P.CN_BF16
EXACT = collections.Counter()          # (route or kernel, tile) -> launches compared exactly


class GuardedOut(Guarded):
    """a guarded output of n elements of fp32 or bf16 (two bf16 per guarded float), pre-filled with a sentinel"""

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for e in shape:
            n *= e
        super().__init__(n if dtype == torch.float32 else (n + 1) // 2, UNWRITTEN)
        self.out = self.view.view(shape) if dtype == torch.float32 else self.view.view(torch.bfloat16)[:n].view(shape)

    def reset(self):
        self.view.fill_(UNWRITTEN)

    def untouched(self):
        return self.intact() and bool((self.view == UNWRITTEN).all())


@functools.lru_cache(maxsize=None)
def _inputs(name, kind="int"):
    """device copies of the inputs of a table entry (kind: int / real / stats1 / stats2) and the tap-flipped filter: made once"""
    from confignet_amd import ops
    case = C.TABLE[name] if name in C.TABLE else C.BF16_EXTRA[name]
    if kind.startswith("stats"):
        host = C.stats_inputs(name, int(kind[-1]))
    else:
        host = C.integer_inputs(case, real=kind == "real")
    dev = {k: v.float().cuda() for k, v in host.items()}
    dev["wt"] = ops.weight_tflip(dev["w"])
    torch.cuda.synchronize()
    return host, dev


@functools.lru_cache(maxsize=None)
def _ref(name, request, kind="int"):
    """float64 reference of a request on a table entry, as fp32 on the device: computed once, shared, never changed"""
    case = C.TABLE[name] if name in C.TABLE else C.BF16_EXTRA[name]
    return C.reference(case, request, _inputs(name, kind)[0]).float().cuda()


def _out_shape(case, request):
    from confignet_amd import ops
    g = C.geom(case)
    return ops.geom_in_shape(g, upsampled=True) if C.REQUESTS[request][0] else ops.geom_out_shape(g)


def _call(case, request, d, out, stats=None, stats_mode=1, act=None):
    """the C-ABI call of a request; d: device inputs.  Returns the call's code."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    g, p, s = C.geom(case), ops._ptr, ops._stream()
    G = ctypes.byref(g)
    if request == "fwd":
        return lib.cn_conv_fwd(G, p(d["x"]), p(d["w"]), p(d["bias"]), p(out), P.ACT_LRELU if act is None else act, C.SLOPE, s)
    if request == "res":
        return lib.cn_conv_fwd_res(G, p(d["x"]), p(d["w"]), p(d["bias"]), p(d["res"]), p(out), P.ACT_RELU, 0.0, s)
    if request == "stats":
        return lib.cn_conv_fwd_stats(G, p(d["x"]), p(d["w"]), p(d["bias"]), p(out), P.ACT_LRELU if stats_mode == 1 else P.ACT_NONE, C.SLOPE,
                                     p(stats), stats_mode, C.SLOPE, s)
    if request == "fwd_dt":
        return lib.cn_conv_fwd_dt(G, p(d["x"]), CN_F32, p(d["w"]), p(d["bias"]), p(out), CN_BF16, P.ACT_LRELU, C.SLOPE, s)
    if request == "dgrad":
        return lib.cn_conv_dgrad(G, p(d["gy"]), p(d["wt"]), p(out), s)
    if request == "dgrad_w":
        return lib.cn_conv_dgrad_w(G, p(d["gy"]), p(d["w"]), p(out), s)
    if request == "dgrad_w_res":
        return lib.cn_conv_dgrad_w_res(G, p(d["gy"]), p(d["w"]), p(d["resx"]), p(out), s)
    if request == "dgrad_dt":
        return lib.cn_conv_dgrad_dt(G, p(d["gy16"]), CN_BF16, p(d["wt"]), p(out), CN_F32, s)
    raise KeyError(request)


def _families(shown):
    return {name: v["launches"] for name, v in shown.items()}


def _family_name(plan):
    from confignet_amd import ops
    return None if plan[5] < 0 else ops.PROF_FAMILIES[plan[5]]


def _count(plan):
    EXACT[(C.ROUTE_NAMES[plan[1]], "%dx%d" % C.TILE_OF[plan[2]] if plan[2] >= 0 else "-")] += 1


def _compare(got, ref, what, cols):
    assert torch.equal(got, ref), what + ": " + _wrong(got.float(), ref.float(), cols)


# ---- 1. the default plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.TABLE))
def test_the_default_plan_of_every_request_gives_the_integer_result(name):
    """Every request of tests/test_conv_plan_cpu.py: REQUESTS on the entry: a request that launches writes the integer result over the
    sentinel (a K split through its own zero pass), leaves the guards alone and shows one launch of the family the plan names; a
    request the plan (or the call before it plans) refuses returns that code and writes nothing -- statistics buffer included."""
    from confignet_amd import ops
    case = C.TABLE[name]
    g = C.geom(case)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        for request in C.REQUESTS:
            plan = C.plan_of(case, request)
            launches = plan is not None and plan[0] == 0
            kind = "stats1" if request == "stats" and launches else "int"
            d = dict(_inputs(name, kind)[1])
            d["gy16"] = d["gy"].to(torch.bfloat16)
            bf16_out = request == "fwd_dt"
            shape = _out_shape(case, request)
            y = GuardedOut(shape, torch.bfloat16 if bf16_out else torch.float32)
            st = Guarded(2 * g.n * g.cout, 0.0)
            what = "%s %s plan %s" % (name, request, plan)
            ops.prof_reset()
            rc = _call(case, request, d, y.out, stats=st.view, stats_mode=1)
            torch.cuda.synchronize()
            shown = _families(ops.prof_collect_by_family())
            if not launches:
                assert rc == (P.CN_EUNSUPPORTED if plan is None else plan[0]) and rc != 0, what
                assert y.untouched() and st.intact() and not bool(st.view.any()) and shown == {}, what + ": a refused request wrote"
                continue
            assert rc == 0, what + ": " + ops.lib.cn_last_error_string().decode()
            ref = _ref(name, request, kind)
            _compare(y.out, ref.to(torch.bfloat16) if bf16_out else ref, what, shape[-1])
            assert y.intact() and st.intact(), what + ": a guard was written"
            assert shown == ({} if _family_name(plan) is None else {_family_name(plan): 1}), (what, shown)
            if request == "stats":
                want = C.stats_reference(ref.double().cpu(), 1, g.n).float().cuda()
                _compare(st.view.view(2, g.n, g.cout), want, what + " statistics", g.cout)
            else:
                assert not bool(st.view.any()), what
            _count(plan)
    finally:
        ops.prof_enable(False)


# ---- 2. / 3. forced tiles, splits and loops; deterministic mode --------------------------------------------------------------------
FORCED_NAMES = sorted(set(C.gemm_entries("fwd")) | set(C.gemm_entries("dgrad")))
LOOPS = [(1,) + v for v in LOOP_VARIANTS] + [(0, 0, 0, -1)]      # cn_conv_loop_select: every variant of the LDS-DMA loop, then the loop off


def _forced(name, loops, split_list, deterministic):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = C.TABLE[name]
    d = _inputs(name)[1]
    outs = {req: GuardedOut(_out_shape(case, req)) for req in ("fwd", "dgrad", "dgrad_w")}
    default = {req: C.plan_of(case, req) for req in outs}
    done, expect = set(), collections.Counter()
    was = ops.DETERMINISTIC
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        ops.set_deterministic(deterministic)
        for loop in loops:
            ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
            for cfg in C.FORCED_CFGS:
                for splits in split_list:
                    C.tune(cfg, splits)
                    for req, y in outs.items():
                        if default[req] is None or default[req][0] != 0 or default[req][1] not in (C.FWD2, C.IGEMM):
                            continue
                        gq = C.request_geom(case, req)
                        if cfg == 4 and gq.cout % 96:
                            continue
                        plan = C.plan_of(case, req)                    # (the plan caps the split: deterministic mode, scalar gather)
                        assert plan[0] == 0 and plan[1] in (C.FWD2, C.IGEMM) and plan[2] == cfg and plan[3] <= splits, (name, req, plan)
                        if deterministic and plan[3] == 1:
                            continue
                        key = (req, plan, loop if plan[1] == C.FWD2 else None)
                        if key in done:
                            continue
                        done.add(key)
                        what = "%s %s loop %s forced tile %d split %d plan %s%s" % (name, req, loop, cfg, splits, plan, " deterministic" if deterministic else "")
                        y.reset()
                        rc = _call(case, req, d, y.out)
                        assert rc == 0, what + ": " + lib.cn_last_error_string().decode()
                        _compare(y.out, _ref(name, req), what, y.out.shape[-1])
                        assert y.intact(), what + ": a guard was written"
                        expect[_family_name(plan)] += 1
                        _count(plan)
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == dict(expect), name
    finally:
        ops.prof_enable(False)
        ops.set_deterministic(was)
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    assert done, name
    return len(done)


@pytest.mark.parametrize("name", FORCED_NAMES)
def test_every_forced_tile_split_and_loop_gives_the_integer_result(name):
    """Tiles 0..4 x K splits 1 / 3 / 8 / 16 x every variant of the LDS-DMA loop and the register-staged loop (the LDS-DMA loop off:
    vector gather, and scalar gather where cin is no multiple of 16), each for the forward with bias and LeakyReLU, cn_conv_dgrad and
    cn_conv_dgrad_w.  A split launch must clear the sentinel through its own zero pass."""
    print(name, _forced(name, LOOPS, C.FORCED_SPLITS, False), "launches")


@pytest.mark.parametrize("name", FORCED_NAMES)
def test_the_split_launches_in_deterministic_mode_give_the_integer_result(name):
    """The split launches of the forced test once more -- every tile, splits 3 / 8 / 16, every variant of the LDS-DMA loop and the
    loop off -- under ops.set_deterministic(True): partial slabs in the stream's workspace and cn_sum_parts instead of the zero pass
    and atomics (scalar-gather layers stay unsplit there: nothing to run)."""
    from confignet_amd import ops
    case = C.TABLE[name]
    vectorised = [r for r in ("fwd", "dgrad", "dgrad_w") if C.plan_of(case, r)[0] == 0 and C.plan_of(case, r)[1] in (C.FWD2, C.IGEMM)
                  and C.request_geom(case, r).cin % 16 == 0]
    if not vectorised:
        # no vectorised implicit-GEMM request: plan_conv_fwd keeps every deterministic launch of the entry unsplit (checked, not skipped)
        was = ops.DETERMINISTIC
        try:
            ops.set_deterministic(True)
            for splits in (3, 8, 16):
                C.tune(2, splits)
                assert all(p[0] != 0 or p[3] == 1 for p in (C.plan_of(case, r) for r in ("fwd", "dgrad", "dgrad_w"))), name
        finally:
            ops.set_deterministic(was)
            C.tune(-1, 0)
        return
    print(name, _forced(name, LOOPS, (3, 8, 16), True), "launches")


# ---- 4. fused epilogues at edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b", "m", "l32", "n96", "n192"])
def test_the_residual_epilogues_on_every_tile_and_loop(name):
    """cn_conv_fwd_res and cn_conv_dgrad_w_res (bt = 1 with a residual) with every tile forced, unsplit, on every variant of the
    LDS-DMA loop and the register-staged loop; a forced split must be refused before anything is written."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = C.TABLE[name]
    d = _inputs(name)[1]
    outs = {req: GuardedOut(_out_shape(case, req)) for req in ("res", "dgrad_w_res") if C.request_geom(case, req) is not None}
    ran, expect = 0, collections.Counter()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        for loop in LOOPS:
            ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
            for cfg in C.FORCED_CFGS:
                for req, y in outs.items():
                    if cfg == 4 and C.request_geom(case, req).cout % 96:
                        continue
                    what = "%s %s loop %s forced tile %d" % (name, req, loop, cfg)
                    C.tune(cfg, 3)
                    assert C.plan_of(case, req)[:2] == (P.CN_EUNSUPPORTED, C.UNSUPPORTED), what
                    y.reset()
                    assert _call(case, req, d, y.out) == P.CN_EUNSUPPORTED and y.untouched(), what + ": a refused split wrote"
                    C.tune(cfg, 1)
                    plan = C.plan_of(case, req)
                    assert plan[0] == 0 and plan[2:4] == (cfg, 1), (what, plan)
                    rc = _call(case, req, d, y.out)
                    assert rc == 0, what + ": " + lib.cn_last_error_string().decode()
                    _compare(y.out, _ref(name, req), what, y.out.shape[-1])
                    assert y.intact(), what + ": a guard was written"
                    expect[_family_name(plan)] += 1
                    _count(plan)
                    ran += 1
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == dict(expect), name      # (the refused splits launched nothing)
    finally:
        ops.prof_enable(False)
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    assert ran >= 20


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", C.STATS_NAMES)
def test_the_statistics_epilogue_at_edges(name, mode):
    """cn_conv_fwd_stats in modes 1 (sum a, sum a^2 of the activated output) and 2 (sum v, sum v^2, sum l, sum l^2 of the
    pre-activation output) where 64 rows of one sample are exactly one tile and the columns are ragged (cout 136 / 144): the output
    and the sums are the integer result (sums of multiples of 1/16 below 2^20: exact through any order of the atomics), on every tile
    the plan lets carry them and every loop variant; the statistics buffer is guarded like the output."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = C.TABLE[name]
    g = C.geom(case)
    kind = "stats%d" % mode
    host, d = _inputs(name, kind)
    pre = C._conv(case, host["x"], host["w"], host["bias"])
    stored = C._act(pre, P.ACT_LRELU) if mode == 1 else pre
    ref_y = stored.float().cuda()
    ref_st = C.stats_reference(stored, mode, g.n).float().cuda()
    nk = 2 if mode == 1 else 4
    y, st = GuardedOut(_out_shape(case, "stats")), Guarded(nk * g.n * g.cout, 0.0)
    ran, expect = 0, collections.Counter()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        for loop in LOOPS[:-1]:
            ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
            for cfg in (-1, 0, 1, 2, 4):
                if cfg == 4 and g.cout % 96:
                    continue
                C.tune(cfg, 0 if cfg < 0 else 1)
                out = (ctypes.c_int * 8)()
                rc_plan = lib.cn_conv_fwd_plan(ctypes.byref(g), 0, 1, P.ACT_LRELU if mode == 1 else P.ACT_NONE, 0, mode, 0, 0, ctypes.byref(out))
                what = "%s mode %d loop %s tile %d plan %s" % (name, mode, loop, cfg, [rc_plan] + list(out)[:5])
                y.reset()
                st.view.zero_()
                rc = _call(case, "stats", d, y.out, stats=st.view, stats_mode=mode)
                assert rc == rc_plan, what
                if rc != 0:          # (tiles of 128 rows straddle the samples' 64 rows: nothing is launched)
                    assert rc == P.CN_EUNSUPPORTED and y.untouched() and not bool(st.view.any()) and st.intact(), what
                    continue
                _compare(y.out, ref_y, what, g.cout)
                _compare(st.view.view(nk, g.n, g.cout), ref_st, what + " statistics", g.cout)
                assert y.intact() and st.intact(), what + ": a guard was written"
                expect[ops.PROF_FAMILIES[out[4]]] += 1
                EXACT[("FWD2 statistics", "%dx%d" % C.TILE_OF[out[1]])] += 1
                ran += 1
        # the loop off: no launch can carry the statistics
        ops.check(lib.cn_conv_loop_select(0, 0, 0, -1), "cn_conv_loop_select")
        C.tune(-1, 0)
        y.reset()
        st.view.zero_()
        assert _call(case, "stats", d, y.out, stats=st.view, stats_mode=mode) == P.CN_EUNSUPPORTED and y.untouched() and not bool(st.view.any())
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == dict(expect), name      # (the refused requests launched nothing)
    finally:
        ops.prof_enable(False)
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    assert ran >= 2 * len(LOOPS[:-1]) or ops.DETERMINISTIC      # (deterministic mode: every statistics request is refused)
    assert ran > 2 * len(LOOPS[:-1]) or name != "s128" or ops.DETERMINISTIC


# ---- 5. Winograd -----------------------------------------------------------------------------------------------------------------
def _wino(xs, cout, four, x, w, b, gy, wt):
    """forward (+ bias + ReLU) of the layer xs -> cout, and the data-gradient form on the same extents and channel counts -- the
    gradient of the layer (n, h, w, cout) -> cin with the filter wt [3][3][cout][cin] from its output gradient gy (n, h, w, cin):
    reduction over cin, cout channels out, as the kernel wants them -- through cn_conv_fwd_wino / _wino4 into guarded outputs, the
    transformed filters guarded too; returns (y, gu)"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, h, wd, cin = xs
    positions = 36 if four else 16
    make, run = (lib.cn_conv_wino4_filter, lib.cn_conv_fwd_wino4) if four else (lib.cn_conv_wino_filter, lib.cn_conv_fwd_wino)
    s = ops._stream()
    u, ud = Guarded(positions * cin * cout, UNWRITTEN), Guarded(positions * cin * cout, UNWRITTEN)
    y, gu = GuardedOut((n, h, wd, cout)), GuardedOut((n, h, wd, cout))
    ops.check(make(ops._ptr(w), ops._ptr(u.view), cin, cout, 0, s), "wino filter")
    ops.check(make(ops._ptr(wt), ops._ptr(ud.view), cout, cin, 1, s), "wino filter")
    assert u.intact() and ud.intact() and not bool((u.view == UNWRITTEN).any()) and not bool((ud.view == UNWRITTEN).any())
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        ops.check(run(n, h, wd, cin, cout, ops._ptr(x), ops._ptr(u.view), ops._ptr(b), ops._ptr(y.out), P.ACT_RELU, 0.0, s), "wino forward")
        ops.check(run(n, h, wd, cin, cout, ops._ptr(gy), ops._ptr(ud.view), None, ops._ptr(gu.out), P.ACT_NONE, 0.0, s), "wino data gradient")
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == {"wino_fwd": 2}
    finally:
        ops.prof_enable(False)
    assert y.intact() and gu.intact() and u.intact() and ud.intact(), "a guard was written"
    return y.out, gu.out


@pytest.mark.parametrize("shape", C.WINO_SHAPES, ids=[str(i) for i in range(len(C.WINO_SHAPES))])
def test_winograd_f2x2_gives_the_integer_result(shape):
    """F(2x2, 3x3) with filters that are integer multiples of 4 in [-12, 12]: both 0.5 * filter transforms are exact, the input and
    output transforms only add, so the pass is exact (tests/test_conv_edge_cases_cpu.py) -- partial tiles on both axes, a 1x1
    image, several blocks per image."""
    xs, cout = shape
    case = (xs, (3, 3), cout, 1, 0, None)
    inp = C.integer_inputs(case)
    inp["w"] = inp["w"] * 4
    ref_y = C.reference(case, "res", {**inp, "res": torch.zeros_like(inp["res"])}).float().cuda()      # relu(conv + bias)
    case_t = (xs[:-1] + (cout,), (3, 3), xs[-1], 1, 0, None)
    inp_t = C.integer_inputs(case_t)
    inp_t["w"] = inp_t["w"] * 4
    ref_gu = C.reference(case_t, "dgrad", inp_t).float().cuda()
    d = {k: v.float().cuda() for k, v in inp.items()}
    y, gu = _wino(xs, cout, False, d["x"], d["w"], d["bias"], inp_t["gy"].float().cuda(), inp_t["w"].float().cuda())
    _compare(y, ref_y, "F(2x2) forward %s" % (shape,), cout)
    _compare(gu, ref_gu, "F(2x2) data gradient %s" % (shape,), cout)
    EXACT[("winograd F(2x2)", "8x8 tiles x 64")] += 2


@pytest.mark.parametrize("shape", C.WINO4_SHAPES, ids=[str(i) for i in range(len(C.WINO4_SHAPES))])
def test_winograd_f4x4_into_guarded_outputs(shape):
    """F(4x4, 3x3) has 1/6 and 1/24 coefficients and is not exact: standard-normal data at the bar of its existing test,
    2e-4 of the largest reference value, now into guarded outputs with guarded transformed filters."""
    xs, cout = shape
    cin = xs[-1]
    case = (xs, (3, 3), cout, 1, 0, None)
    inp = C.integer_inputs(case, real=True)
    inp["w"] = inp["w"] / (9 * cin) ** 0.5
    ref_y = C.reference(case, "res", {**inp, "res": torch.zeros_like(inp["res"])})
    case_t = (xs[:-1] + (cout,), (3, 3), cin, 1, 0, None)
    inp_t = C.integer_inputs(case_t, real=True)
    inp_t["w"] = inp_t["w"] / (9 * cin) ** 0.5
    ref_gu = C.reference(case_t, "dgrad", inp_t)
    d = {k: v.float().cuda() for k, v in inp.items()}
    y, gu = _wino(xs, cout, True, d["x"], d["w"], d["bias"], inp_t["gy"].float().cuda(), inp_t["w"].float().cuda())
    for got, ref, what in ((y, ref_y, "forward"), (gu, ref_gu, "data gradient")):
        err, scale = float((got.double().cpu() - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print("F(4x4) %s %s: max abs err %.2e of scale %.2e" % (what, shape, err, scale))
        assert err <= 2e-4 * scale, (what, err, scale)


# ---- 6. the bf16 family ----------------------------------------------------------------------------------------------------------
def _bf16(name):
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = C.TABLE[name] if name in C.TABLE else C.BF16_EXTRA[name]
    g = C.geom(case)
    host, d = _inputs(name)
    taps = g.k_d * g.k_h * g.k_w
    s = ops._stream()
    both = torch.empty((2, taps * g.cin * g.cout), device="cuda", dtype=torch.bfloat16)
    ops.check(lib.cn_conv_weight_prep_bf16(ops._ptr(d["w"]), ops._ptr(both[0]), ops._ptr(both[1]), taps, g.cin, g.cout, s), "cn_conv_weight_prep_bf16")
    x16, gy16 = d["x"].to(torch.bfloat16), d["gy"].to(torch.bfloat16)
    assert torch.equal(x16.float(), d["x"]) and torch.equal(both[1].float().view(d["w"].shape), d["w"])      # (integers up to 3 are exact in bf16)
    y, gu = GuardedOut(_out_shape(case, "fwd"), torch.bfloat16), GuardedOut(_out_shape(case, "dgrad"), torch.bfloat16)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        ops.check(lib.cn_conv_fwd_bf16(ctypes.byref(g), ops._ptr(x16), ops._ptr(both[0]), ops._ptr(d["bias"]), ops._ptr(y.out), P.ACT_LRELU, C.SLOPE, s), "cn_conv_fwd_bf16")
        ops.check(lib.cn_conv_dgrad_bf16(ctypes.byref(g), ops._ptr(gy16), ops._ptr(both[1]), ops._ptr(gu.out), s), "cn_conv_dgrad_bf16")
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == {"igemm_bf16": 2}
    finally:
        ops.prof_enable(False)
    _compare(y.out, _ref(name, "fwd").to(torch.bfloat16), "%s bf16 forward, tile %d" % (name, C.bf16_tile(g)), g.cout)
    _compare(gu.out, _ref(name, "dgrad").to(torch.bfloat16), "%s bf16 data gradient" % name, g.cin)
    assert y.intact() and gu.intact(), name + ": a guard was written"
    loop = "LDS-DMA" if g.cin % 32 == 0 and g.cout >= 48 and C.bf16_tile(g) != 3 else "register-staged"
    EXACT[("bf16 forward, " + loop, "%dx%d" % C.TILE_OF[C.bf16_tile(g)])] += 1
    EXACT[("bf16 data gradient", "-")] += 1


@pytest.mark.parametrize("name", list(C.BF16_TABLE) + list(C.BF16_EXTRA))
def test_the_bf16_forward_and_data_gradient_give_the_rounded_integer_result(name):
    """cn_conv_fwd_bf16 (bias + LeakyReLU) and cn_conv_dgrad_bf16 on every table entry they take and on one geometry per tile arm of
    conv_bf16 the table does not reach (BF16_EXTRA): the accumulator holds the integer result exactly, the stored value is its
    round-to-nearest-even bf16."""
    _bf16(name)


# ---- 7. the upsample-folded path -------------------------------------------------------------------------------------------------
UPFOLD = [("f", C.TABLE["f"]), ("g", C.TABLE["g"])] + [("upfold-%d" % i, (c[0], c[1], c[2], 1, 1, None)) for i, c in enumerate(UPFOLD_CASES)
                                                        if any(e % 2 for e in c[0][1:-1])]


@pytest.mark.parametrize("name,case", UPFOLD, ids=[u[0] for u in UPFOLD])
def test_the_upsample_folded_layer_gives_the_integer_result(name, case):
    """F.conv with a folded x2 upsample runs as per-parity-class filters, which are sums of integers: forward (+ bias + LeakyReLU),
    data gradient at the stored extent and filter gradient are exact."""
    assert len(UPFOLD) >= 4
    upfold_layer_exact(name, case)


def upfold_layer_exact(name, case, folded=True):
    """the body of the test above, for tests/test_filter_prep_gpu.py as well; folded: what ops.upfold_ok must say of the layer"""
    from confignet_amd import functional as F
    from confignet_amd import ops
    spec = ops.ConvSpec(case[1], up=1)
    assert ops.upfold_ok(spec.geom(case[0], case[2])) == folded
    inp = C.integer_inputs(case)
    x, w, b = (inp[k].float().cuda().requires_grad_(True) for k in ("x", "w", "bias"))
    xr, wr, br = (inp[k].clone().requires_grad_(True) for k in ("x", "w", "bias"))
    y = F.conv(x, w, b, spec, P.ACT_LRELU, C.SLOPE)
    _compare(y.detach(), C.reference(case, "fwd", inp).float().cuda(), name + " forward", case[2])
    lin = F.conv(x, w, b, spec)
    gx, gw, gb = torch.autograd.grad((lin * inp["gy"].float().cuda()).sum(), [x, w, b])
    gxr, gwr, gbr = torch.autograd.grad((C._conv(case, xr, wr, br) * inp["gy"]).sum(), [xr, wr, br])
    assert float(gwr.abs().max()) < 2 ** 24
    _compare(gx, gxr.float().cuda(), name + " data gradient", case[0][-1])
    _compare(gw, gwr.float().cuda(), name + " filter gradient", case[2])
    _compare(gb, gbr.float().cuda(), name + " bias gradient", case[2])
    EXACT[("upsample-folded F.conv", "-")] += 3


# ---- 8. rounding pass ------------------------------------------------------------------------------------------------------------
ROUNDING_SHAPES = ("c", "f", "n192", "m")
_RATIOS = {}               # (kernel, tile) -> (largest error / bound, where)


def _note(kernel, tile, ratio, where):
    if (kernel, tile) not in _RATIOS or not ratio <= _RATIOS[(kernel, tile)][0]:
        _RATIOS[(kernel, tile)] = (ratio, where)


_RAN = []                  # one entry per test case of this file that has run in this process


@pytest.fixture(autouse=True)
def _ran():
    yield
    _RAN.append(1)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """Once, when the last test of this file has run: the rounding ratios and the exact-launch counts of THIS process, with the number
    of test cases of the file that ran in it -- a record made from a selection of the tests says so in its first lines."""
    yield
    path = os.environ.get("CONV_EDGE_ERRORS")
    if not path or not (_RATIOS or EXACT):
        return
    with open(path, "w") as f:
        f.write("tests/test_conv_edges_gpu.py on one MI355X, written once at the end of the run (CONV_EDGE_ERRORS names the path): both tables\n"
                "hold what the tests of that one process did -- %d test cases of the file ran in it.\n\n" % len(_RAN))
        f.write("Rounding pass: standard-normal inputs on the shapes c, f, n192 and m of tests/conv_edge_cases.py, forward with bias and data\n"
                "gradient, one launch per tile and K-slice class, with the LDS-DMA loop on (FWD2; the 128x32 tile on more than 32 channels\n"
                "is IGEMM's) and off (IGEMM).  ratio = the largest |got - ref| / (2 (K + S + 2) 2^-24 A) over the elements of every launch\n"
                "of the tile (A = float64 convolution of |x| and |w| plus |bias|, K = reduction length, S = K slices); the test holds every\n"
                "ratio at <= 1.\n\n")
        f.write("%-8s %-10s %10s   %s\n" % ("kernel", "tile", "ratio", "largest at"))
        for (k, t), (r, w) in sorted(_RATIOS.items()):
            f.write("%-8s %-10s %10.3e   %s\n" % (k, t, r, w))
        f.write("\nLaunches of the exact pass compared bit for bit, per route (or kernel) and tile:\n")
        for (k, t), n in sorted(EXACT.items()):
            f.write("%-32s %-16s %6d\n" % (k, t, n))


@pytest.mark.parametrize("name", ROUNDING_SHAPES)
def test_the_accumulate_arithmetic_stays_within_the_fp32_summation_bound(name):
    """One launch per tile and K-slice class of the forward (bias, no activation) and of the data gradient, on real values, with the
    LDS-DMA loop on and with it off (the register-staged loop on every tile)."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    case = C.TABLE[name]
    host, d = _inputs(name, "real")
    jobs = []                  # (request, float64 reference, A)
    for req in ("fwd", "dgrad"):
        if req == "fwd":       # conv + bias: the "res" request with a zero residual, no activation
            inp = {**host, "res": torch.zeros_like(host["res"])}
            jobs.append((req, C._conv(case, host["x"], host["w"], host["bias"]), C.exact_bound(case, "res", inp)))
        else:
            jobs.append((req, C.reference(case, "dgrad", host), C.exact_bound(case, "dgrad", host)))
    over, expect, kernels = [], collections.Counter(), set()
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        for loop in (LOOPS[1], LOOPS[-1]):
            ops.check(lib.cn_conv_loop_select(*loop), "cn_conv_loop_select")
            for req, ref, A in jobs:
                gq = C.request_geom(case, req)
                for cfg in C.FORCED_CFGS:
                    if cfg == 4 and gq.cout % 96:
                        continue
                    seen = set()
                    for splits in C.FORCED_SPLITS:
                        C.tune(cfg, splits)
                        plan = C.plan_of(case, req)
                        assert plan[0] == 0 and plan[2] == cfg and (loop[0] or plan[1] == C.IGEMM)
                        if C.split_class(plan[3]) in seen:
                            continue
                        seen.add(C.split_class(plan[3]))
                        y = GuardedOut(_out_shape(case, req))
                        rc = _call(case, req, d, y.out, act=P.ACT_NONE)
                        assert rc == 0 and y.intact()
                        err = (y.out.double().cpu() - ref).abs()
                        r = float((err / C.rounding_bound(A, C.ktot(gq), plan[3] if plan[3] > 1 else 0)).max())
                        where = "%s %s, %d slices" % (name, req, plan[3])
                        kernel, tile = C.ROUTE_NAMES[plan[1]], "%dx%d" % C.TILE_OF[cfg]
                        print("%s %s %s: error / bound %.3e" % (kernel, tile, where, r))
                        _note(kernel, tile, r, where)
                        expect[_family_name(plan)] += 1
                        kernels.add((kernel, cfg))
                        if not r <= 1.0:
                            over.append((kernel, tile, where, r))
        torch.cuda.synchronize()
        assert _families(ops.prof_collect_by_family()) == dict(expect), name
    finally:
        ops.prof_enable(False)
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    assert sum(expect.values()) >= 16 and not over, over
    assert {c for k, c in kernels if k == "IGEMM"} >= {0, 1, 2, 3} and {c for k, c in kernels if k == "FWD2"} >= {0, 1, 2}, kernels
