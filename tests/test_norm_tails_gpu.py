"""Layer-level tests of the statistics / normalisation family (csrc/elementwise.hip: nc_reduce*, nc_lin2*,
norm_apply_rows_kernel; csrc/norm_coef.hip: norm_coef_*, dual_coef_*, dual_gx_kernel) against float64 statements of the LAYERS
(tests/norm_tail_ref.py; its tangent-tail part is pinned by finite differences in tests/test_norm_tail_reference_cpu.py):

  1. the R1 tangent tail (DualTailFn, DualTailBatchedFn: forward, and the backward with its second-order terms);
  2. AdaIn and the DiscrBlock tail on BOTH dispatch arms (cn_norm_apply / norm_coef + nc_lin2), offset and constant inputs;
  3. ChannelAffineActFn's one-pass backward (cn_bn_act_bwd);
  4. cn_nc_reduce_dact and the members of the family that had no test in bf16 storage.

How the bounds are set.  Every error is measured relative to max |reference| of THAT quantity (no clamp to 1: the tangent
tail's dL/dx has a maximum of 0.16 at (2, 40, 36, 48), a clamped bound would pass a 100 % error in one of its terms).  The
bound of an fp32 quantity is MULT = 32 times its YARDSTICK -- the error of the same reference statement evaluated in float32 by
torch on the CPU against its float64 run, computed here per case and per quantity -- and never more than the project's older
bounds for these layers (2e-4 on outputs, 5e-4 on gradients, tests/test_nets_gpu.py).  32: the kernels take variances in one
pass and add S terms sequentially and through atomics where torch takes two passes and pairwise sums.  Offset inputs multiply
the bound by (1 + mean^2 / var) (what a one-pass fp32 variance loses), constant channels by the factors derived at the test.
bf16 storage: inputs rounded to bf16, reference in float64 on the rounded values; sums (fp32 accumulation) to 1e-5 sqrt(S),
stored maps (rounded once) to 2^-8, each of the quantity's maximum.

Inputs are drawn in float32, so the LeakyReLU / ReLU decisions of product, yardstick and reference are the same decisions.

Measured table (case x quantity x yardstick x bound x observed error): profiles/norm_tail_errors.txt, written by this file
when NORM_TAIL_ERRORS names a path.  Extract (MI355X):
    case                                                 quantity yardstick     bound  observed
    DualTailFn (3, 5, 7, 6) ty+style                     ty        9.84e-08  3.15e-06  1.32e-07
    DualTailFn (3, 5, 7, 6) ty+style                     tstyle    1.24e-07  3.96e-06  1.52e-07
    DualTailFn (3, 5, 7, 6) ty+style                     g_tx      1.19e-07  3.79e-06  1.37e-07
    DualTailFn (3, 5, 7, 6) ty+style                     g_x       3.58e-07  1.15e-05  3.15e-07
    DualTailFn (3, 5, 7, 6) ty+style                     g_gamma   1.37e-07  4.37e-06  2.41e-07
    DualTailBatchedFn (2, 40, 36, 48) fused              ty        1.90e-07  6.08e-06  2.09e-07
    DualTailBatchedFn (2, 40, 36, 48) fused              tstyle    1.27e-07  4.07e-06  1.43e-07
    DualTailBatchedFn (2, 40, 36, 48) fused              g_tx      1.59e-07  5.08e-06  2.37e-07
    DualTailBatchedFn (2, 40, 36, 48) fused              g_x       2.04e-07  6.52e-06  4.24e-07
    DualTailBatchedFn (2, 40, 36, 48) fused              g_gamma   1.11e-07  3.55e-06  1.36e-07
    tail (1, 58, 58, 20) gy+gstyle fused                 y         9.63e-08  3.08e-06  1.26e-07
    tail (1, 58, 58, 20) gy+gstyle fused                 style     1.15e-07  3.67e-06  9.61e-08
    tail (1, 58, 58, 20) gy+gstyle fused                 g_x       1.59e-07  5.09e-06  1.21e-07
    tail (1, 58, 58, 20) gy+gstyle fused                 g_gamma   1.20e-07  3.83e-06  1.73e-07
    tail (1, 58, 58, 20) gy+gstyle fused                 g_beta    1.85e-07  5.91e-06  1.85e-07
    adain (1, 64, 64, 16) offset 8 fused                 y         2.19e-07  4.72e-04  4.43e-06
    adain (1, 64, 64, 16) offset 8 fused                 g_x       1.62e-07  3.49e-04  4.96e-06
    adain (1, 64, 64, 16) offset 8 fused                 g_sb      2.95e-07  6.36e-04  5.50e-06
    adain (1, 64, 64, 16) constant channel product       g_x       1.30e-07  1.32e-04  9.26e-08
    adain (1, 64, 64, 16) constant channel fallback      g_x       1.30e-07  1.32e-04  5.37e-08
    bf16 adain (1, 64, 64, 16) constant channel          y                -  3.91e-03  2.73e-03
    bf16 adain (1, 64, 64, 16) constant channel          g_x              -  3.91e-03  2.58e-03
    channel_affine_act (2, 64, 64, 8) relu=1 res=1 fused y         7.32e-08  2.34e-06  5.83e-08
    channel_affine_act (2, 64, 64, 8) relu=1 res=1 fused g_x       3.29e-08  1.05e-06  3.29e-08
    channel_affine_act (2, 64, 64, 8) relu=1 res=1 fused g_a       1.33e-07  4.26e-06  2.04e-07
    channel_affine_act (2, 64, 64, 8) relu=1 res=1 fused g_b       1.16e-07  3.71e-06  2.31e-07
    channel_affine_act (2, 64, 64, 8) relu=1 res=1 fused g_res     0.00e+00  0.00e+00  0.00e+00
(no fp32 quantity of the 575 rows above 0.2 of its bound)

Not built: cn_norm_apply's `gx * n > 8192` grid cap needs n >= 513 samples at G = 16384 (a 130 MB tensor); no product shape
reaches it."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import norm_tail_ref as NR

SLOPE = NR.SLOPE
MULT = 32.0
CAP_OUT, CAP_GRAD = 2e-4, 5e-4


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda().contiguous()


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def bf16_round(a):
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64)


def dev_bf16(a):
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).cuda().contiguous()


def leaf(a):
    return dev(a).requires_grad_(True)


_ROWS = []


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("NORM_TAIL_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("%-58s %-10s %10s %10s %10s\n" % ("case", "quantity", "yardstick", "bound", "observed"))
            for r in _ROWS:
                f.write("%-58s %-10s %10s %10.2e %10.2e\n" % (r[0], r[1], "-" if r[2] is None else "%.2e" % r[2], r[3], r[4]))


class Report:
    """Collects every comparison of one case (so the table is complete even when one of them fails), asserts at the end."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            assert not self.failed, "%s: %s" % (self.case, "; ".join(self.failed))

    def _note(self, name, yard, bound, err):
        _ROWS.append((self.case, name, yard, bound, err))
        print("%s %s: yardstick %s bound %.3e observed %.3e" % (self.case, name, yard, bound, err))
        if not err <= bound:
            self.failed.append("%s: error %.3e of its maximum, bound %.3e" % (name, err, bound))

    def fp32(self, name, got, ref, yard, factor=1.0):
        """fp32 quantity: min(MULT * yardstick, cap) * factor, relative to max |ref|."""
        bound = fp32_bound(name, yard) * factor
        err = NR.rel_err(got, ref)                           # (an identically zero gradient must come out as zeros: yardstick 0)
        self._note(name, yard, bound, err)
        return bound

    def rel(self, name, got, ref, bound):
        self._note(name, None, bound, NR.rel_err(got, ref))

    def bf16_sum(self, name, got, ref, spatial):
        assert got.dtype == torch.float32
        self.rel(name, got, ref, 1e-5 * math.sqrt(spatial))

    def bf16_map(self, name, got, ref):
        assert got.dtype == torch.bfloat16
        self.rel(name, got, ref, 2.0 ** -8)


def fp32_bound(name, yard):
    cap = CAP_GRAD if name.startswith("g_") else CAP_OUT
    return min(MULT * yard, cap)


def _f32(rng, *shape):
    return rng.normal(size=shape).astype(np.float32)


def _bc(v, n, nd, c):
    return v.reshape(n, *([1] * nd), c)


# =============================================================================================================================
# 1. the R1 tangent tail
# =============================================================================================================================
TANGENT_SHAPES = {
    "generic": (2, 6, 10, 8),        # generic nc_lin2_kernel, one row block per (n, channel block): plain stores
    "rows": (2, 40, 36, 48),         # G = 17280 >= 16384, CG = 12, q = 3: rows kernels with the x2 sample period, TX = 16 with 4 idle
                                     # columns, 23 row blocks, the last ragged (32 rows: tail loop only), atomics
    "scalar": (3, 5, 7, 6),          # c % 4 != 0: scalar kernels, the non-lazy arm (ta stored, dual_tail_gx + two nc_lin2)
    "three": (3, 6, 10, 8),          # N = 3 under 4 heads: sample n of the stack pairs with x[n % N], not x[n % heads]
}
HEADS = 3                            # heads that go on through the instance norm, behind the one that leaves through the style


@functools.lru_cache(maxsize=None)
def _tangent_inputs(key):
    shape = TANGENT_SHAPES[key]
    rng = np.random.default_rng(sum(shape) + 100)
    n, c = shape[0], shape[-1]
    x = _f32(rng, *shape) * 1.5 + 0.2
    tx = _f32(rng, (1 + HEADS) * n, *shape[1:])
    h = _f32(rng, HEADS * n, *shape[1:])
    u = _f32(rng, n, 2 * c)
    gamma, beta = 1.0 + 0.5 * _f32(rng, c), 0.1 * _f32(rng, c)
    return x, tx, gamma, beta, h, u


@functools.lru_cache(maxsize=None)
def _single_ref(key, use_h, use_u):
    """Reference and yardsticks of ONE head: direction tx[:N], cotangents h[:N] / u."""
    x, tx, gamma, beta, h, u = _tangent_inputs(key)
    n = x.shape[0]
    return NR.yardstick(lambda dt: NR.tangent_tail_grads(x, tx[:n], gamma, beta, h[:n] if use_h else None, u if use_u else None, dtype=dt))


@functools.lru_cache(maxsize=None)
def _batched_ref(key):
    x, tx, gamma, beta, h, u = _tangent_inputs(key)
    return NR.yardstick(lambda dt: NR.tangent_tail_batched_grads(x, tx, gamma, beta, h, u, dtype=dt))


def _tail_statistics(xd, gd, bd):
    from confignet_amd import functional as F
    with torch.no_grad():
        return F.DiscrTailFn.apply(xd, gd, bd, True, SLOPE)[2:]


def _guard_second_order(ref, yard):
    """Input guard: in EVERY channel the reference dL/dx (second-order terms only: zero if the statistics are treated as
    constants) reaches at least 100 times the bound applied to it, so no channel's term can hide below the tolerance."""
    g = ref["g_x"]
    bound_abs = fp32_bound("g_x", yard["g_x"]) * float(g.abs().max())
    per_channel = g.abs().reshape(-1, g.shape[-1]).max(dim=0).values
    assert float(per_channel.min()) >= 100 * bound_abs, (float(per_channel.min()), bound_abs)


@pytest.mark.parametrize("variant", ["ty+style", "ty+style,u=None", "ty+style,h=None", "ty", "style"])
@pytest.mark.parametrize("key", ["generic", "rows", "scalar"])
def test_tangent_tail_one_head_against_the_float64_jvp(key, variant):
    """DualTailFn as hologan_discriminator.tangent calls it: (ty, tstyle) against the float64 JVP of the layer, and the
    gradients of <h, ty> + <u, tstyle> w.r.t. tx, x (second order) and gamma against autograd through that JVP."""
    from confignet_amd import functional as F
    want_ty, want_style = variant != "style", variant != "ty"
    use_h = want_ty and "h=None" not in variant
    use_u = want_style and "u=None" not in variant
    x, tx, gamma, beta, h, u = _tangent_inputs(key)
    n = x.shape[0]
    ref, yard = _single_ref(key, use_h, use_u)
    _guard_second_order(ref, yard)
    xd, txd, gd = leaf(x), leaf(tx[:n]), leaf(gamma)
    mean, q, smean, ssd = _tail_statistics(xd.detach(), gd.detach(), dev(beta))
    ty, tstyle = F.DualTailFn.apply(txd, xd, gd, mean, q, smean, ssd, want_ty, want_style, SLOPE)
    assert (ty is not None) == want_ty and (tstyle is not None) == want_style
    outs = ([ty] if use_h else []) + ([tstyle] if use_u else [])
    cots = ([dev(h[:n])] if use_h else []) + ([dev(u)] if use_u else [])
    g_tx, g_x, g_gamma = torch.autograd.grad(outs, [txd, xd, gd], cots, allow_unused=True)
    with Report("DualTailFn %s %s" % (TANGENT_SHAPES[key], variant)) as r:
        if want_ty:
            r.fp32("ty", ty, ref["ty"], yard["ty"])
        if want_style:
            r.fp32("tstyle", tstyle, ref["tstyle"], yard["tstyle"])
        r.fp32("g_tx", g_tx, ref["g_tx"], yard["g_tx"])
        r.fp32("g_x", g_x, ref["g_x"], yard["g_x"])
        if g_gamma is None:
            assert not use_h
        else:
            r.fp32("g_gamma", g_gamma, ref["g_gamma"], yard["g_gamma"])


def _run_batched(key):
    from confignet_amd import functional as F
    x, tx, gamma, beta, h, u = _tangent_inputs(key)
    xd, txd, gd = leaf(x), leaf(tx), leaf(gamma)
    mean, q, smean, ssd = _tail_statistics(xd.detach(), gd.detach(), dev(beta))
    ty, tstyle = F.DualTailBatchedFn.apply(txd, xd, gd, mean, q, smean, ssd, SLOPE)
    g_tx, g_x, g_gamma = torch.autograd.grad([ty, tstyle], [txd, xd, gd], [dev(h), dev(u)])
    return {"ty": ty.detach(), "tstyle": tstyle.detach(), "g_tx": g_tx, "g_x": g_x, "g_gamma": g_gamma}


TANGENT_QUANTITIES = ("ty", "tstyle", "g_tx", "g_x", "g_gamma")


@pytest.mark.parametrize("key", ["generic", "rows", "scalar", "three"])
def test_tangent_tail_of_stacked_heads_against_the_sum_of_single_head_references(key):
    """DualTailBatchedFn with 1 style head + 3 norm heads (tx: 4 N samples) against the sum over heads of the single-head
    float64 reference, on both arms of its backward (two passes: cn_nc_reduce_hxt + cn_dual_tail_gx_tx / five launches), and
    the arms against each other."""
    from confignet_amd import functional as F
    shape = TANGENT_SHAPES[key]
    ref, yard = _batched_ref(key)
    _guard_second_order(ref, yard)
    arms = {"fused": _run_batched(key)}
    if shape[-1] % 4 == 0:
        prev, F.FUSED_R1_TAIL = F.FUSED_R1_TAIL, False
        try:
            arms["unfused"] = _run_batched(key)
        finally:
            F.FUSED_R1_TAIL = prev
    else:
        arms = {"unfused": arms["fused"]}            # c % 4 != 0: the Function itself takes the non-lazy arm
    for arm, got in arms.items():
        with Report("DualTailBatchedFn %s %s" % (shape, arm)) as r:
            for k in TANGENT_QUANTITIES:
                r.fp32(k, got[k], ref[k], yard[k])
    if len(arms) == 2:
        with Report("DualTailBatchedFn %s fused vs unfused" % (shape,)) as r:
            for k in TANGENT_QUANTITIES:
                r.rel(k, arms["fused"][k], arms["unfused"][k].cpu().double(), fp32_bound(k, yard[k]))


# =============================================================================================================================
# 2. AdaIn and the DiscrBlock tail on both dispatch arms
# =============================================================================================================================
NORM_SHAPES = [
    # (shape, cn_norm_apply takes it)
    ((1, 64, 64, 16), True),         # G = S C / 4 = 16384 exactly
    ((1, 64, 63, 16), False),        # G = 16128: the boundary pair
    ((2, 40, 36, 48), True),         # q = CG / gcd(CG, 256) = 3
    ((1, 58, 58, 20), True),         # CG = 5, q = 5, grid columns rounded 17 -> 20
    ((1, 24, 24, 132), False),       # G = 19008 but CG = 33, q = 33 > 32: cn_norm_apply refuses, the generic nc_lin2_kernel runs
    ((2, 16, 16, 16, 32), True),     # three spatial axes (AdaIn only)
    ((2, 16, 16, 48), False),        # small
]
NORM_IDS = ["x".join(map(str, s)) for s, _ in NORM_SHAPES]


def _norm_inputs(shape, offset=0.15, const_channel=None, seed=0):
    rng = np.random.default_rng(sum(shape) + 200 + seed)
    n, c = shape[0], shape[-1]
    x = _f32(rng, *shape) + np.float32(offset)
    gy = _f32(rng, *shape)
    sb = 0.5 * _f32(rng, n, 2 * c)
    if const_channel is not None:
        x[..., const_channel] = np.float32(3.7)
        sb[:, const_channel] = np.clip(sb[:, const_channel], -0.5, 0.5)      # |s + 1| <= 1.5: what the output bound is derived for
    gamma, beta = 1.0 + 0.5 * _f32(rng, c), 0.1 * _f32(rng, c)
    gstyle = _f32(rng, n, 2 * c)
    return x, gy, sb, gamma, beta, gstyle


def _offset_factor(v):
    """max over (sample, channel) of 1 + mean^2 / var from float64 statistics: what a one-pass fp32 variance loses."""
    v = t64(v)
    axes = tuple(range(1, v.dim() - 1))
    mu = v.mean(dim=axes)
    var = ((v - _bc(mu, v.shape[0], len(axes), v.shape[-1])) ** 2).mean(dim=axes)
    return float((1.0 + mu * mu / var).max())


def _spatial(shape):
    return int(np.prod(shape[1:-1]))


def _adain_takes_fused(x, sb, gy=None):
    """Whether cn_norm_apply takes these inputs (an assertion on its return value).  With gy: where it does, both arms are run on
    the SAME statistics (the sums come from atomics, two runs of them need not give the same bits) and their side outputs and
    parameter gradients must be the same bits -- "the same arithmetic and order as the separate kernels" (elementwise.hip,
    norm_apply_rows_kernel)."""
    from confignet_amd import ops
    xd, sbd = dev(x), dev(sb)
    sp = _spatial(x.shape)
    s1, s2 = ops.nc_reduce(xd)
    fused = ops.norm_apply_fwd(ops.NORM_ADAIN, xd, s1, s2, sbd, None, 1e-3)
    if fused is None or gy is None:
        return fused is not None
    _, _, mean, r = ops.norm_coef_fwd(ops.NORM_ADAIN, s1, s2, sbd, None, sp, 1e-3, xd)
    assert torch.equal(fused[1], mean) and torch.equal(fused[2], r)
    gyd = dev(gy)
    t1, t2 = ops.nc_reduce(gyd, xd)
    bwd = ops.norm_apply_bwd(ops.NORM_ADAIN, gyd, xd, t1, t2, mean, r, sbd, 1e-3)
    assert bwd is not None
    g_sb = ops.norm_coef_bwd(ops.NORM_ADAIN, t1, t2, mean, r, sbd, sp, 1e-3)[3]
    assert torch.equal(bwd[1], g_sb)
    return True


def _run_adain(x, sb, gy):
    from confignet_amd import functional as F
    xd, sbd = leaf(x), leaf(sb)
    y = F.adain(xd, sbd)
    g_x, g_sb = torch.autograd.grad([y], [xd, sbd], [dev(gy)])
    return {"y": y.detach(), "g_x": g_x, "g_sb": g_sb}


def _both_arms(run):
    """run() on the dispatch the product takes, then with cn_norm_apply switched off."""
    from confignet_amd import ops
    first = run()
    prev, ops.NORM_APPLY = ops.NORM_APPLY, False
    try:
        second = run()
    finally:
        ops.NORM_APPLY = prev
    return first, second


@pytest.mark.parametrize("shape,fused", NORM_SHAPES, ids=NORM_IDS)
def test_adain_on_both_dispatch_arms(shape, fused):
    x, gy, sb, _, _, _ = _norm_inputs(shape)
    ref, yard = NR.yardstick(lambda dt: NR.adain_grads(x, sb, gy, dtype=dt))
    assert _adain_takes_fused(x, sb, gy) == fused
    got, fallback = _both_arms(lambda: _run_adain(x, sb, gy))
    with Report("adain %s %s" % (shape, "fused" if fused else "fallback")) as r:
        for k in ("y", "g_x", "g_sb"):
            r.fp32(k, got[k], ref[k], yard[k])
    if fused:
        with Report("adain %s fallback (cn_norm_apply off)" % (shape,)) as r:
            for k in ("y", "g_x", "g_sb"):
                r.fp32(k, fallback[k], ref[k], yard[k])


def _run_tail(x, gamma, beta, gy, gstyle):
    from confignet_amd import functional as F
    xd, gd, bd = leaf(x), leaf(gamma), leaf(beta)
    y, style, mean, q, _, _ = F.DiscrTailFn.apply(xd, gd, bd, True, SLOPE)
    outs = ([y] if gy is not None else []) + ([style] if gstyle is not None else [])
    cots = ([dev(gy)] if gy is not None else []) + ([dev(gstyle)] if gstyle is not None else [])
    g_x, g_gamma, g_beta = torch.autograd.grad(outs, [xd, gd, bd], cots, allow_unused=True)
    return {"y": y.detach(), "style": style.detach(), "mean": mean, "q": q, "g_x": g_x, "g_gamma": g_gamma, "g_beta": g_beta}


def _tail_takes_fused(x, gamma, beta, gy=None):
    """As _adain_takes_fused, for the instance norm behind LeakyReLU: mean, q, d gamma, d beta of the two arms from the same sums."""
    from confignet_amd import ops
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    sp = _spatial(x.shape)
    a1, a2 = ops.nc_reduce(xd, flags=1, slope=SLOPE)
    fused = ops.norm_apply_fwd(ops.NORM_INSTANCE, xd, a1, a2, gd, bd, 1e-3, flags=1, slope=SLOPE)
    if fused is None or gy is None:
        return fused is not None
    _, _, mean, q = ops.norm_coef_fwd(ops.NORM_INSTANCE, a1, a2, gd, bd, sp, 1e-3)
    assert torch.equal(fused[1], mean) and torch.equal(fused[2], q)
    gyd = dev(gy)
    t1, t2 = ops.nc_reduce(gyd, xd, flags=2, slope=SLOPE)
    bwd = ops.norm_apply_bwd(ops.NORM_INSTANCE, gyd, xd, t1, t2, mean, q, gd, 1e-3, flags=2 | 4, slope=SLOPE)
    assert bwd is not None
    _, _, _, g_gamma, g_beta = ops.norm_coef_bwd(ops.NORM_INSTANCE, t1, t2, mean, q, gd, sp, 1e-3)
    assert torch.equal(bwd[1], g_gamma) and torch.equal(bwd[2], g_beta)
    return True


TAIL_QUANTITIES = ("y", "style", "g_x", "g_gamma", "g_beta")


@pytest.mark.parametrize("cot", ["gy+gstyle", "gstyle=None", "gy=None"])
@pytest.mark.parametrize("shape,fused", [s for s in NORM_SHAPES if len(s[0]) == 4], ids=[i for i, s in zip(NORM_IDS, NORM_SHAPES) if len(s[0]) == 4])
def test_discriminator_tail_on_both_dispatch_arms(shape, fused, cot):
    """DiscrTailFn: y, style and the gradients with both cotangents, without the style's (no a3 / b3 term) and with the style's
    alone (the style-only arm of its backward)."""
    x, gy, _, gamma, beta, gstyle = _norm_inputs(shape)
    gy = None if cot == "gy=None" else gy
    gstyle = None if cot == "gstyle=None" else gstyle
    ref, yard = NR.yardstick(lambda dt: NR.tail_grads(x, gamma, beta, gy, gstyle, dtype=dt))
    assert _tail_takes_fused(x, gamma, beta, gy) == fused
    got, fallback = _both_arms(lambda: _run_tail(x, gamma, beta, gy, gstyle))
    with Report("tail %s %s %s" % (shape, cot, "fused" if fused else "fallback")) as r:
        for k in TAIL_QUANTITIES:
            r.fp32(k, got[k], ref[k], yard[k])
    if fused:
        with Report("tail %s %s fallback (cn_norm_apply off)" % (shape, cot)) as r:
            for k in TAIL_QUANTITIES:
                r.fp32(k, fallback[k], ref[k], yard[k])


def test_offset_inputs_stay_within_the_one_pass_variance_bound():
    """x ~ N(8, 1) at (1, 64, 64, 16): a one-pass fp32 variance s2 / S - mu^2 loses a factor (1 + mu^2 / var), here ~65 (with
    the REFERENCE's fp32 arithmetic on the CPU: 1.6e-5 relative error of the variance at this offset against 1.3e-7 at offset
    0.15).  The bound of every quantity is multiplied by that factor, taken from the float64 statistics of the input; outside
    even that bound it is a bug."""
    shape = (1, 64, 64, 16)
    x, gy, sb, gamma, beta, gstyle = _norm_inputs(shape, offset=8.0)
    l = np.where(x > 0, x, np.float32(SLOPE) * x)
    factor = max(_offset_factor(x), _offset_factor(l))
    assert 40 < factor < 100
    ref, yard = NR.yardstick(lambda dt: NR.adain_grads(x, sb, gy, dtype=dt))
    assert _adain_takes_fused(x, sb)
    for arm, got in zip(("fused", "fallback"), _both_arms(lambda: _run_adain(x, sb, gy))):
        with Report("adain %s offset 8 %s" % (shape, arm)) as r:
            for k in ("y", "g_x", "g_sb"):
                r.fp32(k, got[k], ref[k], yard[k], factor)
    ref, yard = NR.yardstick(lambda dt: NR.tail_grads(x, gamma, beta, gy, gstyle, dtype=dt))
    for arm, got in zip(("fused", "fallback"), _both_arms(lambda: _run_tail(x, gamma, beta, gy, gstyle))):
        with Report("tail %s offset 8 %s" % (shape, arm)) as r:
            for k in TAIL_QUANTITIES:
                r.fp32(k, got[k], ref[k], yard[k], factor)


CONST_CHANNEL = 5
CONST_SHAPES = [(1, 64, 64, 16), (2, 16, 16, 48)]


@pytest.mark.parametrize("shape", CONST_SHAPES, ids=["fused", "fallback"])
def test_constant_channels_meet_the_variance_guards(shape):
    """One channel of every sample is the constant 3.7: its raw one-pass fp32 variance is a rounding residue of either sign, which
    the fmaxf(..., 0) guards must catch.  Everything stays finite.
    AdaIn has eps INSIDE the root, so it is defined there: the channel's output is b -- a = (s + 1) / sqrt(1e-3) ~ 32 (s + 1)
    multiplies a few ulp of 3.7, ~8e-6 |s + 1|; with |s + 1| <= 1.5 the bound 1e-4 max(1, |b|) leaves a tenfold margin.
    The instance norm's (std + eps) has an infinite derivative at std = 0 in the reference too: forward only, the channel equals
    beta to the same absolute bound times 1 / eps * sqrt(1e-3); no gradient check."""
    from confignet_amd import functional as F
    ch = CONST_CHANNEL
    x, gy, sb, gamma, beta, gstyle = _norm_inputs(shape, const_channel=ch, seed=1)
    n, c = shape[0], shape[-1]
    assert float(np.abs(sb[:, ch] + 1.0).max()) <= 1.5
    for arm, got in zip(("product", "fallback"), _both_arms(lambda: _run_adain(x, sb, gy))):
        for k in ("y", "g_x", "g_sb"):
            assert bool(torch.isfinite(got[k]).all()), (arm, k)
        b = t64(sb[:, c + ch]).reshape(n, 1, 1)
        err = (got["y"][..., ch].cpu().double() - b).abs()
        assert bool((err <= 1e-4 * b.abs().clamp_min(1.0)).all()), (arm, float(err.max()))
    forward = lambda: dict(zip(("y", "style"), (t.detach() for t in F.DiscrTailFn.apply(dev(x), dev(gamma), dev(beta), True, SLOPE)[:2])))
    for arm, got in zip(("product", "fallback"), _both_arms(forward)):
        assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["style"]).all()), arm
        bt = float(beta[ch])
        err = float((got["y"][..., ch].cpu().double() - bt).abs().max())
        assert err <= 1e-4 * max(1.0, abs(bt)) * (1.0 / 1e-3) * math.sqrt(1e-3), (arm, err)
        assert float((got["style"][:, ch].cpu().double() - 3.7).abs().max()) <= 1e-5 * 3.7


@pytest.mark.parametrize("shape", CONST_SHAPES, ids=["fused", "fallback"])
def test_adain_input_gradient_of_a_constant_channel(shape):
    """The same inputs: AdaIn's gx of the constant channel against float64, at the usual bound (yardstick and error relative to that
    channel's maximum) times sqrt((1 + 1e-3) / 1e-3).

    With the one-pass variance alone this missed at (1, 64, 64, 16): 1.08e-2 of the channel's maximum against a bound of 1.32e-4
    on an MI355X, both arms ((2, 16, 16, 48) passed with 5.8e-8).  (sum x, sum x^2) in fp32 leave a residue of ~1e-6 mu^2 = 2e-5
    where the variance is 0 -- 2 % of eps = 1e-3 under the root, 1 % of r = rsqrt(var + eps), which multiplies gx.  The
    coefficient code of both arms now takes mean((x - mu)^2) from the tensor for a channel with mu^2 > 1000 (var + eps)
    (csrc/typed.h: cn_adain_refine, cn_var_two_pass), whatever produced the sums."""
    ch = CONST_CHANNEL
    x, gy, sb, _, _, _ = _norm_inputs(shape, const_channel=ch, seed=1)
    ref, r32 = NR.adain_grads(x, sb, gy), NR.adain_grads(x, sb, gy, dtype=torch.float32)
    yard_ch = NR.rel_err(r32["g_x"][..., ch], ref["g_x"][..., ch])
    # the arm this shape is meant to take, and (fused) mean, r, d[s|b] of the two arms bit for bit ON the two-pass path
    assert _adain_takes_fused(x, sb, gy) == (shape == CONST_SHAPES[0])
    for arm, got in zip(("product", "fallback"), _both_arms(lambda: _run_adain(x, sb, gy))):
        with Report("adain %s constant channel %s" % (shape, arm)) as r:
            r.fp32("g_x", got["g_x"][..., ch], ref["g_x"][..., ch], yard_ch, math.sqrt((1 + 1e-3) / 1e-3))


def test_bf16_adain_on_a_constant_channel():
    """bf16 storage takes norm_coef_fwd + nc_lin2 only (cn_norm_apply refuses it), so this is the bf16 instantiation of the two-pass
    variance: the constant channel (3.703125 once rounded) against float64 on the bf16-rounded inputs, output and input gradient
    as stored maps (2^-8 of the channel's maximum; the 1 % error of r without the two-pass variance would be 2.8 times that)."""
    from confignet_amd import functional as F
    shape, ch = CONST_SHAPES[0], CONST_CHANNEL
    x, gy, sb, _, _, _ = _norm_inputs(shape, const_channel=ch, seed=1)
    ref = NR.adain_grads(bf16_round(x).numpy(), sb, bf16_round(gy).numpy())
    xd, sbd = dev_bf16(x).requires_grad_(True), leaf(sb)
    y = F.adain(xd, sbd)
    g_x, g_sb = torch.autograd.grad([y], [xd, sbd], [dev_bf16(gy)])
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(g_x.float()).all()) and bool(torch.isfinite(g_sb).all())
    with Report("bf16 adain %s constant channel" % (shape,)) as r:
        r.bf16_map("y", y.detach()[..., ch], ref["y"][..., ch])
        r.bf16_map("g_x", g_x[..., ch], ref["g_x"][..., ch])


# =============================================================================================================================
# 3. ChannelAffineActFn / cn_bn_act_bwd
# =============================================================================================================================
AFFINE_SHAPES = [
    (2, 8, 8, 64),        # rep = 1, one row block per channel block
    (2, 64, 64, 8),       # 8192 rows -> rep = 16 partial rows, summed on the host
    (1, 91, 91, 8),       # 8281 rows, odd -> rep = 1, 17 row blocks on one address (atomics), ragged last block
    (4, 2, 2, 2048),      # CG = 512, cblk = 8, TY = 4
    (2, 5, 7, 6),         # c % 4 != 0: the Function takes the unfused arm
]


@functools.lru_cache(maxsize=None)
def _affine_inputs(shape, relu, res):
    rng = np.random.default_rng(sum(shape) + 300)
    c = shape[-1]
    x, gy = _f32(rng, *shape), _f32(rng, *shape)
    a, b = 1.0 + 0.5 * _f32(rng, c), 0.3 * _f32(rng, c)
    r = _f32(rng, *shape) if res else None
    if relu:
        # keep the ReLU's argument away from 0, so that its float64, float32 and product evaluations take the same decisions
        pre = lambda: t64(x) * t64(a) + t64(b) + (t64(r) if res else 0.0)
        near = (pre().abs() < 1e-4).numpy()
        x[near] += np.float32(0.5)
        assert float(pre().abs().min()) >= 1e-4
    return x, a, b, r, gy


def _run_affine(x, a, b, res, relu, gy):
    from confignet_amd import functional as F
    xd, ad, bd = leaf(x), leaf(a), leaf(b)
    rd = leaf(res) if res is not None else None
    y = F.channel_affine_act(xd, ad, bd, rd, relu)
    g = torch.autograd.grad([y], [xd, ad, bd] + ([rd] if rd is not None else []), [dev(gy)])
    out = {"y": y.detach(), "g_x": g[0], "g_a": g[1], "g_b": g[2]}
    if rd is not None:
        out["g_res"] = g[3]
    return out


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=["x".join(map(str, s)) for s in AFFINE_SHAPES])
def test_channel_affine_act_backward_in_one_pass(shape, relu, res):
    """relu?(x a + b (+ res)) and its gradients against float64 autograd, on the one-pass backward (cn_bn_act_bwd) and on the
    separate passes (BN_BWD_FUSED off)."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    x, a, b, r, gy = _affine_inputs(shape, relu, res)
    ref, yard = NR.yardstick(lambda dt: NR.channel_affine_act_grads(x, a, b, r, relu, gy, dtype=dt))
    keys = ("y", "g_x", "g_a", "g_b") + (("g_res",) if res else ())
    arms = {"fused" if shape[-1] % 4 == 0 else "unfused (c % 4)": _run_affine(x, a, b, r, relu, gy)}
    if shape[-1] % 4 == 0:
        prev, F.BN_BWD_FUSED = F.BN_BWD_FUSED, False
        try:
            arms["unfused"] = _run_affine(x, a, b, r, relu, gy)
        finally:
            F.BN_BWD_FUSED = prev
    for arm, got in arms.items():
        with Report("channel_affine_act %s relu=%d res=%d %s" % (shape, relu, res, arm)) as rp:
            for k in keys:
                rp.fp32(k, got[k], ref[k], yard[k])
    if shape[-1] % 4 != 0:
        # the V = 1 kernel, which the Function does not reach: cn_bn_act_bwd directly
        y = arms["unfused (c % 4)"]["y"]
        gx, g, gb, ga = ops.bn_act_bwd(dev(gy), y if relu else dev(x), dev(x), dev(a), ops.ACT_RELU if relu else ops.ACT_NONE, res)
        with Report("bn_act_bwd %s relu=%d res=%d scalar kernel" % (shape, relu, res)) as rp:
            rp.fp32("g_x", gx, ref["g_x"], yard["g_x"])
            rp.fp32("g_a", ga, ref["g_a"], yard["g_a"])
            rp.fp32("g_b", gb, ref["g_b"], yard["g_b"])
            if res:
                rp.fp32("g_res", g, ref["g_res"], yard["g_res"])
            else:
                assert g is None


def test_one_pass_activation_backward_inside_the_zero_pool():
    """cn_bn_act_bwd and cn_act_bwd_bias with their sums carved from the step's zero pool (no clearing launch of their own):
    the same result as outside it."""
    from confignet_amd import ops
    shape = (2, 8, 8, 64)
    x, a, b, r, gy = _affine_inputs(shape, True, True)
    ref, yard = NR.yardstick(lambda dt: NR.channel_affine_act_grads(x, a, b, r, True, gy, dtype=dt))
    y = dev(ref["y"].numpy())
    xd, gyd, ad = dev(x), dev(gy), dev(a)
    outside = ops.bn_act_bwd(gyd, y, xd, ad, ops.ACT_RELU, True)
    outside_p = ops.act_bwd_partials(gyd, y, ops.ACT_RELU)
    ops.zero_pool_begin("test", xd.device)
    try:
        inside = ops.bn_act_bwd(gyd, y, xd, ad, ops.ACT_RELU, True)
        inside_p = ops.act_bwd_partials(gyd, y, ops.ACT_RELU)
        inside = [t.clone() for t in inside]
        inside_p = [t.clone() for t in inside_p]
    finally:
        ops.zero_pool_end()
    g_ref = t64(gy) * (ref["y"] > 0)
    for where, (gx, g, gb, ga), (gx_p, gb_p) in (("outside", outside, outside_p), ("inside", inside, inside_p)):
        with Report("bn_act_bwd / act_bwd_partials %s zero pool %s" % (shape, where)) as rp:
            rp.fp32("g_x", gx, ref["g_x"], yard["g_x"])
            rp.fp32("g_res", g, ref["g_res"], yard["g_res"])
            rp.fp32("g_b", gb, ref["g_b"], yard["g_b"])
            rp.fp32("g_a", ga, ref["g_a"], yard["g_a"])
            rp.fp32("g_res", gx_p, g_ref, yard["g_res"])
            rp.fp32("g_b", gb_p.sum(0), ref["g_b"], yard["g_b"])
    # the same result: the maps, and the sums that come from the pool (two row blocks per channel here: an atomic pair onto zero,
    # which commutes)
    for a_, b_ in zip(tuple(outside) + tuple(outside_p), tuple(inside) + tuple(inside_p)):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("shape", [(2, 64, 64, 8), (2, 8, 8, 64)], ids=["2x64x64x8", "2x8x8x64"])
def test_bf16_channel_affine_backward_in_one_pass(shape):
    from confignet_amd import ops
    rng = np.random.default_rng(sum(shape) + 310)
    c = shape[-1]
    rows = int(np.prod(shape[:-1]))
    x, gy = _f32(rng, *shape), _f32(rng, *shape)
    y = np.maximum(_f32(rng, *shape), 0)                      # a ReLU output (zeros included)
    a = 1.0 + 0.5 * _f32(rng, c)
    gx, g, gb, ga = ops.bn_act_bwd(dev_bf16(gy), dev_bf16(y), dev_bf16(x), dev(a), ops.ACT_RELU, True)
    g_ref = bf16_round(gy) * (bf16_round(y) > 0)
    with Report("bf16 bn_act_bwd %s" % (shape,)) as rp:
        rp.bf16_map("g_res", g, g_ref)
        rp.bf16_map("g_x", gx, g_ref * t64(a))
        rp.bf16_sum("g_b", gb, g_ref.reshape(rows, c).sum(0), rows)
        rp.bf16_sum("g_a", ga, (g_ref * bf16_round(x)).reshape(rows, c).sum(0), rows)


# =============================================================================================================================
# 4. cn_nc_reduce_dact, and the rest of the family in bf16 storage
# =============================================================================================================================
def _act_out(z, act):
    from confignet_amd import ops
    if act == ops.ACT_LRELU:
        return np.where(z > 0, z, np.float32(SLOPE) * z).astype(np.float32)
    if act == ops.ACT_RELU:
        return np.maximum(z, 0).astype(np.float32)
    return np.tanh(z).astype(np.float32)


def _dact_ref(x1, x2, act, flags, period, dtype=torch.float64):
    """a = x1 act'(x2) with x2 the activation's OUTPUT, sum a, sum a f2(x2); x2 holds `period` samples."""
    from confignet_amd import ops
    x1, x2 = NR.tt(x1, dtype), NR.tt(x2, dtype)
    x2 = x2.repeat(x1.shape[0] // x2.shape[0], *([1] * (x2.dim() - 1)))
    one = torch.ones((), dtype=dtype)
    if act == ops.ACT_LRELU:
        d = torch.where(x2 > 0, one, torch.full((), SLOPE, dtype=dtype))
    elif act == ops.ACT_RELU:
        d = torch.where(x2 > 0, one, torch.zeros((), dtype=dtype))
    else:
        d = 1.0 - x2 * x2
    a = x1 * d
    f2 = torch.where(x2 > 0, x2, SLOPE * x2) if flags & 2 else x2
    axes = tuple(range(1, x1.dim() - 1))
    return {"a": a, "sum": a.sum(dim=axes), "dot": (a * f2).sum(dim=axes)}


def _dact_inputs(shape, act, period):
    rng = np.random.default_rng(sum(shape) + 400 + act)
    x1 = _f32(rng, *shape)
    x2 = _act_out(_f32(rng, period, *shape[1:]), act)
    return x1, x2


@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("act", ["lrelu", "relu", "tanh"])
@pytest.mark.parametrize("shape", [(6, 9, 11, 40), (6, 40, 36, 48)], ids=["6x9x11x40", "6x40x36x48"])
def test_activation_backward_with_its_two_sums_in_one_pass(shape, act, flags):
    """cn_nc_reduce_dact with the sample period of the stacked tangent pass (3 N samples of x1 against N of x2): the map and both
    sums; the sums alone (want_a = False: a is None); the first sum alone (want_dot = False)."""
    from confignet_amd import ops
    code = {"lrelu": ops.ACT_LRELU, "relu": ops.ACT_RELU, "tanh": ops.ACT_TANH}[act]
    period = shape[0] // 3
    x1, x2 = _dact_inputs(shape, code, period)
    ref, yard = NR.yardstick(lambda dt: _dact_ref(x1, x2, code, flags, period, dt))
    x1d, x2d = dev(x1), dev(x2)
    with Report("nc_reduce_dact %s %s flags=%d" % (shape, act, flags)) as r:
        a, s1, s2 = ops.nc_reduce_dact(x1d, x2d, code, SLOPE, x2_period=period, flags=flags)
        r.fp32("a", a, ref["a"], yard["a"])
        r.fp32("sum", s1, ref["sum"], yard["sum"])
        r.fp32("dot", s2, ref["dot"], yard["dot"])
        a, s1, s2 = ops.nc_reduce_dact(x1d, x2d, code, SLOPE, x2_period=period, flags=flags, want_a=False)
        assert a is None
        r.fp32("sum", s1, ref["sum"], yard["sum"])
        r.fp32("dot", s2, ref["dot"], yard["dot"])
        a, s1, s2 = ops.nc_reduce_dact(x1d, x2d, code, SLOPE, x2_period=period, flags=flags, want_dot=False)
        assert s2 is None
        r.fp32("a", a, ref["a"], yard["a"])
        r.fp32("sum", s1, ref["sum"], yard["sum"])


def test_activation_backward_sums_without_a_sample_period_and_in_deterministic_mode():
    """x2 with as many samples as x1 (no period); then deterministic mode at a size with 23 row blocks per (n, channel block):
    the per-block partials added in block order (the `parts` arm of nc_reduce_launch) -- two runs give the same bits."""
    from confignet_amd import ops
    shape = (6, 40, 36, 48)
    x1, x2 = _dact_inputs(shape, ops.ACT_LRELU, shape[0])
    ref, yard = NR.yardstick(lambda dt: _dact_ref(x1, x2, ops.ACT_LRELU, 2, shape[0], dt))
    x1d, x2d = dev(x1), dev(x2)
    with Report("nc_reduce_dact %s lrelu flags=2 no period" % (shape,)) as r:
        a, s1, s2 = ops.nc_reduce_dact(x1d, x2d, ops.ACT_LRELU, SLOPE, flags=2)
        for k, v in (("a", a), ("sum", s1), ("dot", s2)):
            r.fp32(k, v, ref[k], yard[k])
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        runs = [ops.nc_reduce_dact(x1d, x2d, ops.ACT_LRELU, SLOPE, flags=2, want_a=False)[1:] for _ in range(2)]
        runs = [[t.clone() for t in run] for run in runs]
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    with Report("nc_reduce_dact %s lrelu flags=2 deterministic" % (shape,)) as r:
        r.fp32("sum", runs[0][0], ref["sum"], yard["sum"])
        r.fp32("dot", runs[0][1], ref["dot"], yard["dot"])


def _lrelu64(x):
    return torch.where(x > 0, x, SLOPE * x)


def _dual_gx_case(shape, rounder, dtype):
    """Inputs and float64 statements of cn_dual_tail_gx / cn_dual_tail_gx_tx with RANDOM coefficients (the map, not the algebra:
    the algebra is section 1), as tests/test_ops_gpu.py::test_r1_tail_backward_reductions_and_gradients_in_two_passes states them."""
    rng = np.random.default_rng(sum(shape) + 500)
    n, c = shape[0], shape[-1]
    heads = 3
    x = _f32(rng, *shape)
    tx = _f32(rng, (heads + 1) * n, *shape[1:])
    h = _f32(rng, heads * n, *shape[1:])
    x64, tx64, h64 = (NR.tt(rounder(t).numpy(), dtype) for t in (x, tx, h))
    xr = x64.repeat(heads, 1, 1, 1)
    mask = torch.where(xr > 0, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))
    co = {k: _f32(rng, heads * n, c) for k in ("kh", "kt", "ka", "kc", "K1", "K2", "K0")}
    co.update({k: _f32(rng, n, c) for k in ("et", "ex", "e0", "D2", "D0")})
    return x, tx, h, x64, tx64, h64, xr, mask, co, heads


def _dual_gx_ref(case, ta64, dtype=torch.float64):
    x, tx, h, x64, tx64, h64, xr, mask, co, heads = case
    n, c = x64.shape[0], x64.shape[-1]
    b = lambda k, rows: NR.tt(co[k], dtype).reshape(rows, 1, 1, c)
    a64 = torch.where(xr > 0, xr, SLOPE * xr)
    per_head = mask * (b("kh", heads * n) * h64 + b("kt", heads * n) * ta64 + b("ka", heads * n) * a64 + b("kc", heads * n))
    g_x = per_head.reshape(heads, *x64.shape).sum(0) + b("et", n) * tx64[:n] + b("ex", n) * x64 + b("e0", n)
    g_tx = torch.cat([b("D2", n) * x64 + b("D0", n), mask * (b("K1", heads * n) * h64 + b("K2", heads * n) * a64 + b("K0", heads * n))])
    return {"g_x": g_x, "g_tx": g_tx}


TWO_SHAPES = [(3, 9, 11, 40), (2, 40, 36, 48)]
TWO_IDS = ["3x9x11x40", "2x40x36x48"]


@pytest.mark.parametrize("shape", TWO_SHAPES, ids=TWO_IDS)
def test_fp32_members_without_a_test_of_their_own(shape):
    """cn_row_scale_diff ((a - b) s[row] k, the backward of the squared-difference sum) and cn_dual_tail_gx (the five-launch arm's
    second-order map, random coefficients) in fp32 against float64."""
    from confignet_amd import ops
    rng = np.random.default_rng(sum(shape) + 600)
    n = shape[0]
    a, b = _f32(rng, *shape), _f32(rng, *shape)
    k = 0.37
    for rows in (1, n):
        s = (0.5 + rng.uniform(size=rows)).astype(np.float32)
        fn = lambda dt: {"out": (NR.tt(a, dt) - NR.tt(b, dt)) * NR.tt(s, dt).reshape(rows, 1, 1, 1) * k}
        ref, yard = NR.yardstick(fn)
        with Report("row_scale_diff %s rows=%d" % (shape, rows)) as r:
            r.fp32("out", ops.row_scale_diff(dev(a), dev(b), dev(s), k), ref["out"], yard["out"])
    ident = lambda t: torch.as_tensor(t)

    def fn(dt):
        case = _dual_gx_case(shape, ident, dt)
        return _dual_gx_ref(case, case[7] * case[4][n:], dt)
    ref, yard = NR.yardstick(fn, keys=("g_x",))
    x, tx, h, x64, tx64, h64, xr, mask, co, heads = _dual_gx_case(shape, ident, torch.float64)
    cod = {k_: dev(v) for k_, v in co.items()}
    ta = dev((mask * tx64[n:]).numpy())
    with Report("dual_tail_gx %s" % (shape,)) as r:
        r.fp32("g_x", ops.dual_tail_gx(dev(h), ta, dev(tx), dev(x), cod, SLOPE), ref["g_x"], yard["g_x"])


@pytest.mark.parametrize("shape", TWO_SHAPES, ids=TWO_IDS)
def test_bf16_statistics_of_the_tails(shape):
    """bf16 storage: cn_nc_reduce4, cn_nc_reduce_hxt (ta given / formed from tx in the pass), cn_nc_reduce_dact."""
    from confignet_amd import ops
    rng = np.random.default_rng(sum(shape) + 700)
    n = shape[0]
    S = int(np.prod(shape[1:-1]))
    x = _f32(rng, *shape) * 2 + 0.5
    xb, xr = dev_bf16(x), bf16_round(x)
    lr = _lrelu64(xr)
    with Report("bf16 nc_reduce4 %s" % (shape,)) as r:
        got = ops.nc_reduce4(xb, SLOPE)
        for name, g, rf in zip(("sum x", "sum x^2", "sum l", "sum l^2"), got, (xr, xr * xr, lr, lr * lr)):
            r.bf16_sum(name, g, rf.sum(dim=(1, 2)), S)
    heads = 3
    h, tx = _f32(rng, heads * n, *shape[1:]), _f32(rng, heads * n, *shape[1:])
    hr, txr = bf16_round(h), bf16_round(tx)
    xrep = xr.repeat(heads, 1, 1, 1)
    mask = torch.where(xrep > 0, 1.0, SLOPE)
    for lazy in (False, True):
        ta_r = mask * txr if lazy else bf16_round((mask * txr).numpy())
        ta_d = dev_bf16(tx) if lazy else dev_bf16((mask * txr).numpy())
        with Report("bf16 nc_reduce_hxt %s ta_is_tx=%d" % (shape, lazy)) as r:
            H1, H2, E = ops.nc_reduce_hxt(dev_bf16(h), xb, ta_d, SLOPE, ta_is_tx=lazy)
            r.bf16_sum("sum h", H1, hr.sum(dim=(1, 2)), S)
            r.bf16_sum("sum h l", H2, (hr * _lrelu64(xrep)).sum(dim=(1, 2)), S)
            r.bf16_sum("sum h ta", E, (hr * ta_r).sum(dim=(1, 2)), S)
    with Report("bf16 nc_reduce_dact %s" % (shape,)) as r:
        for want_a in (True, False):
            a, s1, s2 = ops.nc_reduce_dact(dev_bf16(tx), xb, ops.ACT_LRELU, SLOPE, x2_period=n, flags=2, want_a=want_a)
            if want_a:
                r.bf16_map("a", a, mask * txr)
            else:
                assert a is None
            r.bf16_sum("sum", s1, (mask * txr).sum(dim=(1, 2)), S)
            r.bf16_sum("dot", s2, (mask * txr * _lrelu64(xrep)).sum(dim=(1, 2)), S)


@pytest.mark.parametrize("shape", TWO_SHAPES, ids=TWO_IDS)
def test_bf16_maps_of_the_tails(shape):
    """bf16 storage: cn_dual_tail_gx_tx with random coefficients (ta given / formed in the pass), cn_tap_bwd, cn_row_scale_diff."""
    from confignet_amd import ops
    n = shape[0]
    case = _dual_gx_case(shape, bf16_round, torch.float64)
    x, tx, h, x64, tx64, h64, xr, mask, co, heads = case
    cod = {k: dev(v) for k, v in co.items()}
    for lazy in (False, True):
        ta64 = mask * tx64[n:] if lazy else bf16_round((mask * tx64[n:]).numpy())
        ta_d = dev_bf16(tx)[n:] if lazy else dev_bf16((mask * tx64[n:]).numpy())
        ref = _dual_gx_ref(case, ta64)
        gx, gtx = ops.dual_tail_gx_tx(dev_bf16(h), ta_d, dev_bf16(tx), dev_bf16(x), cod, SLOPE, ta_is_tx=lazy)
        with Report("bf16 dual_tail_gx_tx %s ta_is_tx=%d" % (shape, lazy)) as r:
            r.bf16_map("g_x", gx, ref["g_x"])
            r.bf16_map("g_tx", gtx, ref["g_tx"])
    rng = np.random.default_rng(sum(shape) + 800)
    y = np.maximum(_f32(rng, *shape), 0)
    tgt, g = _f32(rng, *shape), _f32(rng, *shape)
    a, b = _f32(rng, *shape), _f32(rng, *shape)
    k = 0.37
    for rows in (1, n):
        s = (0.5 + rng.uniform(size=rows)).astype(np.float32)
        sb = t64(s).reshape(rows, 1, 1, 1)
        with Report("bf16 tap_bwd / row_scale_diff %s rows=%d" % (shape, rows)) as r:
            for with_g in (True, False):
                out = ops.tap_bwd(dev_bf16(y), dev_bf16(tgt), dev_bf16(g) if with_g else None, dev(s), k, ops.ACT_RELU)
                ref = ((bf16_round(g) if with_g else 0.0) + (bf16_round(y) - bf16_round(tgt)) * sb * k) * (bf16_round(y) > 0)
                r.bf16_map("tap_bwd", out, ref)
            r.bf16_map("row_scale_diff", ops.row_scale_diff(dev_bf16(a), dev_bf16(b), dev(s), k), (bf16_round(a) - bf16_round(b)) * sb * k)
