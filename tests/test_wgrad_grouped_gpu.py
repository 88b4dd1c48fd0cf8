"""The grouped filter gradient (cn_conv_wgrad_grouped: many jobs of csrc/wgrad2.hip in a few launches), the ResNet-50 trunk that
leaves its filter gradients to the join of its pass, and the row-chunked cn_bn_fold_bwd.

Grouped call.  The body is the single launch's; what is new is the job table in the kernel arguments, the workgroup id relative to
the job's first workgroup, the plan that gives a job its share of a launch, and the cut into launches.  So:
  * with every job planned as a launch of its own (solo) the result must be the bits of cn_conv_wgrad_ws on random fp32 inputs
    -- same body, same numbers;
  * with the grouped plan the slices differ, so the inputs are the integers of tests/wgrad_edge_cases.py (every partial sum
    exact in fp32 in any order): the result must equal the float64 reference, and therefore the per-layer launches, bit for bit.
The lists (tests/wgrad_grouped_cases.py says which way of going wrong each job is there for) are a few hundred microseconds each.

Trunk.  ResNetTrunkFn at 64 x 64, n = 2, with and without a gradient sink: every parameter gradient of the grouped path against
the float64 oracle, held to TWICE the error the per-layer path has against the same oracle on the same inputs (only the order of
the filter gradients' row sums differs, by at most the slice count; the forward pass and the data gradients are the same launches).

cn_bn_fold_bwd.  Row-chunked against the float64 formula in the kernel's comment, on integers and powers of two: bit equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import wgrad_edge_cases as W
from tests import wgrad_grouped_cases as C

GUARD = 256
GUARD_VALUE = 12345.0


class Packed:
    """The outputs of a list of jobs as views into ONE allocation, 256 sentinel floats in front of, between and behind them"""

    def __init__(self, shapes, priors):
        sizes = [int(np.prod(s)) for s in shapes]
        self.buf = torch.full((sum(sizes) + GUARD * (len(sizes) + 1),), GUARD_VALUE, device="cuda", dtype=torch.float32)
        self.views, self.gaps, o = [], [], 0
        for s, n, p in zip(shapes, sizes, priors):
            self.gaps.append((o, o + GUARD))
            o += GUARD
            v = self.buf[o:o + n].view(s)
            v.copy_(p)
            self.views.append(v)
            o += n
        self.gaps.append((o, o + GUARD))

    def intact(self):
        return all(bool((self.buf[a:b] == GUARD_VALUE).all()) for a, b in self.gaps)


def _prior(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-5, 6, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def _exact(name):
    """per job of a list: (x, gy, float64 reference + the prior where the job accumulates, prior) on integer inputs -- computed
    once, shared, never changed"""
    out = []
    for k, (case, acc) in enumerate(C.LISTS[name]):
        x, gy = W.integer_inputs(case, seed=100 + k)
        prior = _prior(W.filter_shape(case), 7 + k)
        ref = W.reference(x, gy, case) + (prior.double() if acc else 0.0)
        out.append((x.float(), gy.float(), ref.float(), prior))
    return out


def _single_launches(cases, xs, gys, priors):
    """cn_conv_wgrad_ws per job on copies of the priors"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    outs = []
    for (case, acc), x, gy, p in zip(cases, xs, gys, priors):
        g = W.geom(case)
        out = p.clone().cuda()
        nbytes = int(lib.cn_conv_wgrad_workspace_bytes(ctypes.byref(g)))
        ws = torch.full((max(nbytes // 4, 1),), float("nan"), device="cuda")
        ops.check(lib.cn_conv_wgrad_ws(ctypes.byref(g), ops._fptr(x), ops._fptr(gy), ops._fptr(out), acc, ops._ptr(ws), nbytes, ops._stream()),
                  "cn_conv_wgrad_ws")
        outs.append(out)
    return outs


def _grouped(cases, xs, gys, priors, solo):
    from confignet_amd import ops
    packed = Packed([W.filter_shape(c) for c, _ in cases], priors)
    jobs = [(x, gy, W.geom(c), v, acc) for (c, acc), x, gy, v in zip(cases, xs, gys, packed.views)]
    ops._sum_slabs_grouped(ops.conv_wgrad_grouped(jobs, solo=solo))
    torch.cuda.synchronize()
    return packed


@pytest.mark.parametrize("name", list(C.LISTS))
def test_jobs_planned_alone_give_the_bits_of_the_single_launch(name):
    from confignet_amd import ops
    cases = C.LISTS[name]
    gen = torch.Generator().manual_seed(5)
    xs = [torch.randn(c[0], generator=gen).cuda() for c, _ in cases]
    gys = [torch.randn(tuple(ops.geom_out_shape(W.geom(c))), generator=gen).cuda() for c, _ in cases]
    priors = [torch.randn(W.filter_shape(c), generator=gen) for c, _ in cases]
    want = _single_launches(cases, xs, gys, priors)
    packed = _grouped(cases, xs, gys, priors, solo=True)
    for k, (got, ref) in enumerate(zip(packed.views, want)):
        assert torch.equal(got, ref), "%s job %d %s: %d of %d elements differ from cn_conv_wgrad_ws" % (
            name, k, cases[k][0], int((got != ref).sum()), ref.numel())
    assert packed.intact(), name + ": a guard between the outputs was written"


@pytest.mark.parametrize("name", list(C.LISTS))
def test_the_grouped_plan_gives_the_integer_result(name):
    cases = C.LISTS[name]
    data = _exact(name)
    xs, gys = [d[0].cuda() for d in data], [d[1].cuda() for d in data]
    priors = [d[3] for d in data]
    packed = _grouped(cases, xs, gys, priors, solo=False)
    plan, _ = C.plan([W.geom(c) for c, _ in cases])
    for k, (got, d) in enumerate(zip(packed.views, data)):
        ref = d[2].cuda()
        assert torch.equal(got, ref), "%s job %d %s (%s): %d of %d elements differ from the float64 reference, largest %g" % (
            name, k, cases[k][0], plan[k], int((got != ref).sum()), ref.numel(), float((got - ref).abs().max()))
    assert packed.intact(), name + ": a guard between the outputs was written"
    single = _single_launches(cases, xs, gys, priors)
    for k, (got, ref) in enumerate(zip(packed.views, single)):
        assert torch.equal(got, ref), "%s job %d: grouped and per-layer launches differ on integer inputs" % (name, k)


# ---- the trunk ---------------------------------------------------------------------------------------------------------------------
def _randomize(net, seed, scale):
    rng = np.random.default_rng(seed)
    ws = net.get_weights()
    for i, w in enumerate(ws):
        if w.ndim == 1:
            ws[i] = (w + rng.normal(size=w.shape) * scale).astype(np.float32)
    net.set_weights(ws)


@functools.lru_cache(maxsize=None)
def _trunk_runs():
    """{(sink, grouped): gradient arena} of one RealEncoder step at 64 x 64, n = 2, the float64 oracle's gradients laid out the same
    way, and the table of the trainable tensors (name, offset, size)"""
    from confignet_amd import nn as cnn
    from confignet_amd import ops
    from confignet_amd.dnn_models.real_encoder import RealEncoder
    from oracle import ref_nets as R
    rng = np.random.default_rng(11)
    enc = RealEncoder(43, (64, 64, 3), ((-30, 30), (-10, 10), (0, 0)), rng=rng)
    _randomize(enc, 7, 0.05)
    img_np = rng.uniform(-1, 1, size=(2, 64, 64, 3)).astype(np.float32)
    base = enc.arena.data_ptr()
    table = [(enc._entries[i][0], (enc.weights[i].data_ptr() - base) // 4, enc.weights[i].numel()) for i in enc._trainable_idx]
    runs = {}
    try:
        for sink in (False, True):
            for grouped in (False, True):
                ops.WGRAD_GROUPED = grouped
                img = torch.tensor(img_np, device="cuda")
                emb, rot = enc(img)
                loss = (emb ** 2).sum() + (rot ** 2).sum() * 10
                if sink:
                    cnn.backward_into_arenas(loss, [enc])
                else:
                    grads = torch.autograd.grad(loss, enc.trainable_weights)
                    enc.grad_arena.zero_()
                    for p_, g_ in zip(enc.trainable_weights, grads):
                        o = (p_.data_ptr() - base) // 4
                        enc.grad_arena[o:o + p_.numel()] += g_.reshape(-1)
                torch.cuda.synchronize()
                runs[(sink, grouped)] = enc.grad_arena.detach().double().cpu()
    finally:
        ops.WGRAD_GROUPED = True
    wr = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in enc.get_weights()]
    e, r = R.real_encoder_forward(wr, torch.tensor(img_np, dtype=torch.float64))
    g64 = torch.autograd.grad((e ** 2).sum() + (r ** 2).sum() * 10, [wr[i] for i in enc._trainable_idx])
    ref = torch.zeros_like(runs[(False, False)])
    for (_, o, n), g_ in zip(table, g64):
        ref[o:o + n] = g_.reshape(-1)
    return runs, ref, table


def _errors(arena, ref, table):
    """(rel-L2 of the whole arena, worst rel-L2 of one tensor, its name)"""
    whole = float((arena - ref).norm() / ref.norm())
    worst = max((float((arena[o:o + n] - ref[o:o + n]).norm() / (ref[o:o + n].norm() + 1e-30)), name) for name, o, n in table)
    return whole, worst[0], worst[1]


@pytest.mark.parametrize("sink", [False, True])
def test_trunk_gradients_grouped_within_twice_the_per_layer_error(sink):
    """Measured on an MI355X (profiles/resnet_join_ab.txt): per-layer against float64 and grouped against float64 agree to the
    printed digits -- the error of both is the fp32 forward / data-gradient chain's, which the two paths share."""
    runs, ref, table = _trunk_runs()
    per_layer = _errors(runs[(sink, False)], ref, table)
    grouped = _errors(runs[(sink, True)], ref, table)
    direct = float((runs[(sink, True)] - runs[(sink, False)]).norm() / runs[(sink, False)].norm())
    print("trunk gradients vs float64, sink=%s: per-layer arena %.3e worst tensor %.3e (%s); grouped arena %.3e worst tensor %.3e (%s); "
          "grouped vs per-layer %.3e" % ((sink,) + per_layer + grouped + (direct,)))
    assert np.isfinite(runs[(sink, True)].numpy()).all()
    assert per_layer[0] > 0.0 and per_layer[1] > 0.0
    assert grouped[0] <= 2.0 * per_layer[0], "gradient arena: grouped rel-L2 %.3e, per-layer %.3e" % (grouped[0], per_layer[0])
    assert grouped[1] <= 2.0 * per_layer[1], "worst tensor: grouped %.3e (%s), per-layer %.3e (%s)" % (grouped[1:] + per_layer[1:])
    # every tensor by itself: not beyond twice the per-layer path's WORST tensor (its own per-layer error can be zero by chance)
    for name, o, n in table:
        e = float((runs[(sink, True)][o:o + n] - ref[o:o + n]).norm() / (ref[o:o + n].norm() + 1e-30))
        assert e <= 2.0 * per_layer[1], "%s: grouped rel-L2 %.3e, twice the per-layer path's worst %.3e" % (name, e, 2.0 * per_layer[1])


# ---- cn_bn_fold_bwd ----------------------------------------------------------------------------------------------------------------
def test_bn_fold_bwd_in_row_chunks_equals_the_float64_formula_bit_for_bit():
    """d w = g' a, d gamma = rs (sum_k g' w + gs bm), d beta = gs, d b = a gs, ADDED to what gout holds.  Segments: K = 1 (fifteen
    empty chunks), K = 16 (a chunk a row), K = 37 (no multiple of the 16 chunks: three rows a chunk, the last chunk one row, three
    empty), K = 9 * 64 (36 rows a chunk, more than the 16 row lanes), cout 64 / 128 / 64 / 192.  g', w, gs, bm and the prior are
    integers in [-3, 3], a and rs powers of two: every product and sum is exact in fp32 (|sum| <= 9 * 576 * 4 < 2^24)."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    assert lib.cn_bn_fold_bwd_chunks() == 16
    rng = np.random.default_rng(3)
    segs = [(1, 64), (16, 128), (37, 64), (576, 192)]
    ncols = sum(c for _, c in segs)
    # arena layout per segment: kernel (K x cout), bias, gamma, beta -- 4 floats of padding between the segments
    seg9, arena_size, packed, aoff, blk = [], 0, 0, 0, 0
    for K, c in segs:
        src = arena_size
        offs = [src + K * c, src + K * c + c, src + K * c + 2 * c]
        seg9.append([src, packed, K * c, c, aoff] + offs + [blk])
        arena_size = offs[2] + c + 4
        packed += K * c
        aoff += c
        blk += c // 64
    ints = lambda n: rng.integers(-3, 4, size=n).astype(np.float64)
    arena, gwf, gs, bm, prior = ints(arena_size), ints(packed), ints(ncols), ints(ncols), ints(arena_size)
    a, rs = 2.0 ** rng.integers(-2, 3, size=ncols), 2.0 ** rng.integers(-2, 3, size=ncols)
    want = prior.copy()
    for (src, dst, count, c, ao, ob, og, obeta, _), (K, _) in zip(seg9, segs):
        g, w = gwf[dst:dst + count].reshape(K, c), arena[src:src + count].reshape(K, c)
        sl = slice(ao, ao + c)
        want[src:src + count] += (g * a[sl]).reshape(-1)
        want[og:og + c] += rs[sl] * ((g * w).sum(0) + gs[sl] * bm[sl])
        want[obeta:obeta + c] += gs[sl]
        want[ob:ob + c] += a[sl] * gs[sl]
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    table = torch.tensor(seg9, dtype=torch.int32, device="cuda")
    for chunked in (True, False):
        gout = dev(prior)
        ops.bn_fold_bwd(table, blk, dev(gwf), dev(gs), dev(arena), dev(a), dev(rs), dev(bm), gout, chunked=chunked)
        torch.cuda.synchronize()
        got = gout.double().cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "chunked=%s: %d of %d elements differ, first at %d: %g != %g" % (
            chunked, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])
