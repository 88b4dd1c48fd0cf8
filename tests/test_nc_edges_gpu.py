"""Every launch shape of the per-(sample, channel) reductions and of the per-sample rows grid (csrc/elementwise.hip: plan_nc_reduce,
nc_reduce_rows, plan_nc_rows) on the edge shapes of tests/golden/nc_plans.json: dead lanes in the last channel block, a short last
row block, a single row block (plain stores), scalar channels, the tail loop alone, the ordered partials of deterministic mode.

Exact arithmetic: inputs are integers in [-3, 3], the slope is 0.25, integer coefficients are in [-2, 2].  Every term is a multiple
of 1/16 below 10 in size (and a multiple of 1/4 below 8 where it is stored as bf16: exact there too), and a sum over at most 16384
rows stays below 2^24 sixteenths, so fp32 holds every partial sum exactly in ANY order of the adds, fused or not: each result is
compared with the float64 reference by torch.equal, without a tolerance.  The entries are called through `lib` directly; what a
call must write holds NaN before it (a missing store or a missing clear shows), outputs declared clear hold zero, and 256 floats in
front of and behind the sums keep a sentinel."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nc_plans.json")))
SHAPES = [tuple(s) for s in GOLDEN["edge_shapes"]]              # the twelve (n, s, c) of the reductions
ROWS_SHAPES = [tuple(s) for s in GOLDEN["rows_shapes"]]         # the six (n, s, c) of the rows grid
BF16_SHAPES = [(3, 35, 20), (2, 64, 260), (2, 4099, 48)]
SLOPE = 0.25
LRELU, RELU = 1, 2
GUARD, GUARD_VALUE = 256, 12345.0
CN_EINVAL = -1
NAN = float("nan")
_id = lambda s: "x".join(map(str, s))


def _ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """three (n, s, c) tensors and a (c,) coefficient of small integers (float64, host): drawn once per shape, never changed"""
    n, s, c = shape
    return tuple(_ints(shape, 7 * n + 3 * s + c + k) for k in range(3)) + (_ints((c,), c, -2, 2),)


def _lrelu(t):
    return torch.where(t > 0, t, t * SLOPE)


def _deriv(o, act, slope):
    return torch.where(o > 0, torch.ones_like(o), torch.full_like(o, slope if act == LRELU else 0.0))


def _model(x1, x2, flags=0, period=0, dact=None, x3=None, coef=None):
    """(sum a, sum a b, a, coef a) of nc_reduce_kernel in float64; dact = (activation code, slope of its derivative)"""
    a = _lrelu(x1) if flags & 1 else x1
    if x2 is not None and period:
        x2 = x2[:period].repeat(x1.shape[0] // period, 1, 1)
    if dact is not None:
        a = a * _deriv(x2, *dact)
    b = a if x2 is None else (_lrelu(x2) if flags & 2 else x2)
    if x3 is not None:
        b = x3
    return a.sum(1), (a * b).sum(1), a, (None if coef is None else a * coef)


class Sums:
    """Q x (n, c) fp32 sums inside a larger allocation with sentinels on both sides, holding `fill` before the call"""

    def __init__(self, q, n, c, fill):
        self.buf = torch.full((q * n * c + 2 * GUARD,), GUARD_VALUE, device="cuda", dtype=torch.float32)
        self.all = self.buf[GUARD:GUARD + q * n * c].view(q, n, c)
        self.all.fill_(fill)
        self.fill = fill

    def __getitem__(self, q):
        return self.all[q]

    def check(self, want, what):
        """want: one float64 (n, c) tensor per sum, None for a sum that was not asked for (it must still hold what it held)"""
        edge = torch.full((GUARD,), GUARD_VALUE, device="cuda")
        assert torch.equal(self.buf[:GUARD], edge) and torch.equal(self.buf[-GUARD:], edge), what + ": a guard was written"
        for q, w in enumerate(want):
            if w is None:
                kept = torch.isnan(self.all[q]) if self.fill != self.fill else self.all[q] == self.fill
                assert bool(kept.all()), "%s: sum %d was written" % (what, q)
            else:
                _same(self.all[q], w, "%s: sum %d" % (what, q))


def _same(got, want, what):
    got, want = got.double().cpu(), want.reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()           # (NaN != anything)
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements wrong, first at %s: got %r, want %r" % (what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda()


def _dtypes(shape):
    return [torch.float32, torch.bfloat16] if shape in BF16_SHAPES else [torch.float32]


def _fills():
    """(what the sums hold before the call, flag): NaN and the call clears what it must; zero and bit 4 says so"""
    return ((NAN, 0), (0.0, 16))


def _call(fn, *args):
    from confignet_amd import ops
    ops.check(fn(*args, ops._stream()), fn.__name__)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_nc_reduce(shape):
    """both sums, each alone, the leaky-relu flags, x2 absent, x2 with a sample period of 1; outputs NaN or declared clear"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape
    h1, h2 = _inputs(shape)[:2]
    cases = [(flags, True, 0) for flags in (0, 1, 2, 3)] + [(0, False, 0), (1, False, 0)] + ([(2, True, 1)] if n == 2 else [])
    for dtype in _dtypes(shape):
        x1, x2 = _dev(h1, dtype), _dev(h2, dtype)
        x2p = _dev(h2[:1], dtype)
        for flags, has2, period in cases:
            r1, r2, _, _ = _model(h1, h2 if has2 else None, flags, period)
            for want1, want2 in ((True, True), (True, False), (False, True)):
                for fill, clear in _fills() if (want1 and want2) else _fills()[:1]:
                    what = "%s %s flags %d x2 %d period %d sums %d%d fill %s" % (shape, dtype, flags, has2, period, want1, want2, fill)
                    out = Sums(2, n, c, fill)
                    _call(lib.cn_nc_reduce, ops._ptr(x1), ops._ptr((x2p if period else x2) if has2 else None), ops._ptr(out[0]) if want1 else None,
                          ops._ptr(out[1]) if want2 else None, n, s, c, flags | clear | period << 8, SLOPE, ops._dt(x1))
                    out.check([r1 if want1 else None, r2 if want2 else None], what)


STAT_SHAPES = [sh for sh in SHAPES if sh[2] % 4 == 0]          # every shape but (5, 70, 3)


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=_id)
def test_nc_reduce4_and_nc_reduce_hxt(shape):
    """the four tail statistics; the three h-x-ta sums with ta given and with ta = lrelu'(x) tx formed in the pass, x at the
    sample period n and (n = 2) at the period 1"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape
    hh, hx, ht = _inputs(shape)[:3]
    l = _lrelu(hh)
    want4 = [hh.sum(1), (hh * hh).sum(1), l.sum(1), (l * l).sum(1)]
    for dtype in _dtypes(shape):
        h, x, t = _dev(hh, dtype), _dev(hx, dtype), _dev(ht, dtype)
        for fill, clear in _fills():
            out = Sums(4, n, c, fill)
            _call(lib.cn_nc_reduce4, ops._ptr(h), ops._ptr(out.all), n, s, c, SLOPE, clear, ops._dt(h))
            out.check(want4, "reduce4 %s %s fill %s" % (shape, dtype, fill))
        for period in (n, 1) if n == 2 else (n,):
            xs = hx[:period].repeat(n // period, 1, 1)
            xp = _dev(hx[:period], dtype)
            for lazy in (0, 1):
                ta = ht * _deriv(xs, LRELU, SLOPE) if lazy else ht
                want3 = [hh.sum(1), (hh * _lrelu(xs)).sum(1), (hh * ta).sum(1)]
                for fill, clear in _fills():
                    out = Sums(3, n, c, fill)
                    _call(lib.cn_nc_reduce_hxt, ops._ptr(h), ops._ptr(xp), ops._ptr(t), ops._ptr(out.all), n, s, c, SLOPE, period,
                          clear | (32 if lazy else 0), ops._dt(h))
                    out.check(want3, "hxt %s %s period %d ta_is_tx %d fill %s" % (shape, dtype, period, lazy, fill))


def test_the_four_wide_entries_refuse_scalar_channels_and_write_nothing():
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape = (5, 70, 3)
    h, x, t = (_dev(v, torch.float32) for v in _inputs(shape)[:3])
    out = Sums(4, n, c, NAN)
    assert lib.cn_nc_reduce4(ops._ptr(h), ops._ptr(out.all), n, s, c, SLOPE, 0, ops._dt(h), ops._stream()) == CN_EINVAL
    assert lib.cn_nc_reduce_hxt(ops._ptr(h), ops._ptr(x), ops._ptr(t), ops._ptr(out.all), n, s, c, SLOPE, n, 0, ops._dt(h), ops._stream()) == CN_EINVAL
    out.check([None] * 4, "refused")


def _maps(shape, dtype, count):
    """`count` (n, s, c) tensors of NaN for the maps a fused backward writes"""
    return [torch.full(shape, NAN, device="cuda", dtype=dtype) for _ in range(count)]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_fused_activation_backward_entries(shape):
    """cn_act_bwd_bias, cn_bn_act_bwd (with and without g_out; its activations have slope 0) and cn_nc_reduce_dact (sums with and
    without the map and the second sum, leaky-relu on x2 for the second sum) with ReLU and LeakyReLU"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape
    hg, hy, hx, hk = _inputs(shape)
    for dtype in _dtypes(shape):
        gy, y, x, k = _dev(hg, dtype), _dev(hy, dtype), _dev(hx, dtype), _dev(hk, torch.float32)
        for act in (RELU, LRELU):
            for fill, clear in _fills():
                what = "%s %s act %d fill %s" % (shape, dtype, act, fill)
                r1, _, ra, _ = _model(hg, hy, dact=(act, SLOPE))
                out, (gx,) = Sums(1, n, c, fill), _maps(shape, dtype, 1)
                _call(lib.cn_act_bwd_bias, ops._ptr(gy), ops._ptr(y), ops._ptr(gx), ops._ptr(out[0]), n, s, c, act, SLOPE, clear, ops._dt(gy))
                out.check([r1], "act_bwd_bias " + what)
                _same(gx, ra, "act_bwd_bias gx " + what)

                r1, r2, ra, rs = _model(hg, hy, dact=(act, 0.0), x3=hx, coef=hk)
                for with_g in (True, False):
                    out, (g, gx) = Sums(2, n, c, fill), _maps(shape, dtype, 2)
                    _call(lib.cn_bn_act_bwd, ops._ptr(gy), ops._ptr(y), ops._ptr(x), ops._ptr(k), ops._ptr(g) if with_g else None, ops._ptr(gx),
                          ops._ptr(out[0]), ops._ptr(out[1]), n, s, c, act, clear, ops._dt(gy))
                    out.check([r1, r2], "bn_act_bwd g_out %d %s" % (with_g, what))
                    _same(gx, rs, "bn_act_bwd gx " + what)
                    if with_g:
                        _same(g, ra, "bn_act_bwd g " + what)
                    else:
                        assert bool(torch.isnan(g).all())

                for flags, with_a, with_dot in ((2, True, True), (0, True, False), (2, False, True)):
                    r1, r2, ra, _ = _model(hg, hy, flags, dact=(act, SLOPE))
                    out, (a,) = Sums(2, n, c, fill), _maps(shape, dtype, 1)
                    _call(lib.cn_nc_reduce_dact, ops._ptr(gy), ops._ptr(y), ops._ptr(out[0]), ops._ptr(out[1]) if with_dot else None,
                          ops._ptr(a) if with_a else None, n, s, c, flags | clear, SLOPE, act, ops._dt(gy))
                    out.check([r1, r2 if with_dot else None], "reduce_dact flags %d a %d dot %d %s" % (flags, with_a, with_dot, what))
                    if with_a:
                        _same(a, ra, "reduce_dact a " + what)
                    else:
                        assert bool(torch.isnan(a).all())


@pytest.mark.parametrize("shape", [(1, 1030, 8), (2, 4099, 48)], ids=_id)
def test_the_ordered_partials_of_deterministic_mode(shape):
    """every entry once with per-row-block partials and the ordered second pass (3 and 65 row blocks, a short last one)"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape
    h1, h2, h3, hk = _inputs(shape)
    x1, x2, x3, k = _dev(h1, torch.float32), _dev(h2, torch.float32), _dev(h3, torch.float32), _dev(hk, torch.float32)
    dt = ops._dt(x1)
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        r1, r2, _, _ = _model(h1, h2, 2)
        for want1, want2 in ((True, True), (True, False), (False, True)):
            out = Sums(2, n, c, NAN)
            _call(lib.cn_nc_reduce, ops._ptr(x1), ops._ptr(x2), ops._ptr(out[0]) if want1 else None, ops._ptr(out[1]) if want2 else None, n, s, c, 2, SLOPE, dt)
            out.check([r1 if want1 else None, r2 if want2 else None], "det reduce %d%d" % (want1, want2))
        l = _lrelu(h1)
        out = Sums(4, n, c, NAN)
        _call(lib.cn_nc_reduce4, ops._ptr(x1), ops._ptr(out.all), n, s, c, SLOPE, 0, dt)
        out.check([h1.sum(1), (h1 * h1).sum(1), l.sum(1), (l * l).sum(1)], "det reduce4")
        for lazy in (0, 1):
            ta = h3 * _deriv(h2, LRELU, SLOPE) if lazy else h3
            out = Sums(3, n, c, NAN)
            _call(lib.cn_nc_reduce_hxt, ops._ptr(x1), ops._ptr(x2), ops._ptr(x3), ops._ptr(out.all), n, s, c, SLOPE, n, 32 if lazy else 0, dt)
            out.check([h1.sum(1), (h1 * _lrelu(h2)).sum(1), (h1 * ta).sum(1)], "det hxt %d" % lazy)
        r1, _, ra, _ = _model(h1, h2, dact=(LRELU, SLOPE))
        out, (gx,) = Sums(1, n, c, NAN), _maps(shape, torch.float32, 1)
        _call(lib.cn_act_bwd_bias, ops._ptr(x1), ops._ptr(x2), ops._ptr(gx), ops._ptr(out[0]), n, s, c, LRELU, SLOPE, 0, dt)
        out.check([r1], "det act_bwd_bias")
        _same(gx, ra, "det act_bwd_bias gx")
        r1, r2, ra, rs = _model(h1, h2, dact=(RELU, 0.0), x3=h3, coef=hk)
        out, (g, gx) = Sums(2, n, c, NAN), _maps(shape, torch.float32, 2)
        _call(lib.cn_bn_act_bwd, ops._ptr(x1), ops._ptr(x2), ops._ptr(x3), ops._ptr(k), ops._ptr(g), ops._ptr(gx), ops._ptr(out[0]), ops._ptr(out[1]),
              n, s, c, RELU, 0, dt)
        out.check([r1, r2], "det bn_act_bwd")
        _same(gx, rs, "det bn_act_bwd gx")
        _same(g, ra, "det bn_act_bwd g")
        r1, r2, ra, _ = _model(h1, h2, 2, dact=(LRELU, SLOPE))
        out, (a,) = Sums(2, n, c, NAN), _maps(shape, torch.float32, 1)
        _call(lib.cn_nc_reduce_dact, ops._ptr(x1), ops._ptr(x2), ops._ptr(out[0]), ops._ptr(out[1]), ops._ptr(a), n, s, c, 2, SLOPE, LRELU, dt)
        out.check([r1, r2], "det reduce_dact")
        _same(a, ra, "det reduce_dact a")
    finally:
        ops.set_deterministic(was)


def _lin2_model(x1, a1, x2, a2, b, flags, a3=None, b3=None):
    v1 = _lrelu(x1) if flags & 1 else x1
    if flags & 16:
        v1 = v1 * _deriv(x2, LRELU, SLOPE)
    r = b + a1 * v1 + a2 * (_lrelu(x2) if flags & 2 else x2)
    if flags & 4:
        r = r * _deriv(x2, LRELU, SLOPE)
    if a3 is not None:
        r = r + a3 * x2 + b3
    return torch.clamp(r, min=0.0) if flags & 8 else r


@pytest.mark.parametrize("per_channel", [False, True], ids=["per-sample", "per-channel"])
@pytest.mark.parametrize("shape", ROWS_SHAPES, ids=_id)
def test_nc_lin2_on_and_next_to_the_rows_grid(shape, per_channel):
    """the rows grid (gx a multiple of q, one channel group per thread), the generic kernel one group short of it and at q = 33,
    scalar channels; flag sets 0, lrelu(x2) with the mask, relu, the mask with a3 / b3, the tangent through the activation"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    n, s, c = shape
    h1, h2 = _inputs(shape)[:2]
    cs = (1, 1, c) if per_channel else (n, 1, c)
    a1, a2, b, a3, b3 = (_ints(cs, 100 + k + c, -2, 2) for k in range(5))
    x1, x2 = _dev(h1, torch.float32), _dev(h2, torch.float32)
    d = [_dev(t.reshape(-1, c), torch.float32) for t in (a1, a2, b, a3, b3)]
    for flags, with3 in ((0, False), (2 | 4, False), (8, False), (4, True), (16, False)):
        want = _lin2_model(h1, a1, h2, a2, b, flags, a3 if with3 else None, b3 if with3 else None)
        y = torch.full(shape, NAN, device="cuda")
        _call(lib.cn_nc_lin2, ops._ptr(x1), ops._ptr(d[0]), ops._ptr(x2), ops._ptr(d[1]), ops._ptr(d[2]), ops._ptr(d[3]) if with3 else None,
              ops._ptr(d[4]) if with3 else None, ops._ptr(y), n, s, c, 0 if per_channel else c, flags, SLOPE, ops._dt(y))
        _same(y, want, "lin2 %s per_channel %d flags %d a3 %d" % (shape, per_channel, flags, with3))
