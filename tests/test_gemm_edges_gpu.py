"""Every kernel and every route of the dense GEMM family (csrc/gemm.hip: the 64x64 MFMA tile with its split-K forms, the thin
kernel with its K slices, the rows kernels <8 | 16 | 32, TB>, the depth kernel, the two grouped kernels) at the smallest shapes at
which each can go wrong, through `lib` directly.  The route every cn_gemm / cn_gemm_acc request takes is the one cn_gemm_plan names,
and tests/test_gemm_plan_cpu.py pins that function to the recorded plans.

Exact pass: integer inputs in [-3, 3], integer bias in [-2, 2], an integer prior value in [-5, 5] where C is accumulated into, slope
0.25, mask values in [-3, 3].  Every term is a multiple of 1/4 below 9 K + 7 in size and K <= 12289, so 4 |sum| < 2^24: fp32 holds
every partial sum exactly in ANY order of the adds -- across K steps, MFMA blocks, K quarters, slices, slabs and atomics -- and the
activations (none, LeakyReLU, ReLU, ReLU6) and the mask epilogue (1, the slope, 0, or 1 - y^2 on an integer y, times the sum: below
2^24 quarters as well) are exact too.  Each result is compared with the float64 reference by torch.equal, without a tolerance: one
dropped or doubled K element, one bias added twice, one wrong row or column shows as a whole number.

Operands are views into larger allocations, once with the tight leading dimension and once with ld = extent + 3 (rows misaligned
for any 8- or 16-byte load), the padding holding NaN: one read of it poisons a whole output element.  C is used with ldc = n and
ldc = n + 5 inside 256 sentinel floats on both sides (Guarded of tests/test_wgrad_edges_gpu.py); its padding columns hold the
sentinel and must keep it; what a call must write holds NaN before it, what it adds to holds the integer prior value.

Rounding pass: what integers cannot show, on standard-normal inputs, one case per kernel at its shape with the most slices:
    |got - ref|_ij <= 2 (K + S + 2) 2^-24 A_ij,      A = the float64 product of |A| and |B|, plus |bias| and |prior|,
S the slice count (K quarters of the rows kernels, K slices, slabs): fp32 accumulation of K products in any order plus S combining
adds plus at most two more for the bias and a prior value, the factor 2 for truncating intermediate rounding inside the MFMA -- the
bound of the two convolution edge files, derived, not tuned.  The largest observed error / bound per kernel is in
profiles/gemm_edge_errors.txt, written by this file when GEMM_EDGE_ERRORS names a path."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_edge_cases as G
from tests.test_wgrad_edges_gpu import GUARD_VALUE, Guarded

SLOPE = 0.25
NAN = float("nan")
CN_EINVAL = -1
NONE, LRELU, RELU, TANH, RELU6 = G.NONE, G.LRELU, G.RELU, G.TANH, G.RELU6
ACTS = (NONE, LRELU, RELU, RELU6)


def _ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def _op(t, pad):
    """(view, leading dimension): the float64 host matrix as fp32 on the device, a view with ld = columns + pad into a larger
    allocation that holds NaN everywhere else"""
    rows, cols = t.shape
    ld = cols + pad
    buf = torch.full((rows * ld + 8,), NAN, device="cuda", dtype=torch.float32)
    v = buf[4:4 + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(t.float())
    return v, ld


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Out:
    """m x n floats with leading dimension n + pad between two guards: the data holds NaN, or `before`; the padding columns the sentinel"""

    def __init__(self, m, n, pad, before=None):
        self.g = Guarded(m * (n + pad), GUARD_VALUE)
        self.full = self.g.view.view(m, n + pad)
        self.data = self.full[:, :n]
        self.ldc = n + pad
        if before is None:
            self.data.fill_(NAN)
        else:
            self.data.copy_(before.float())

    def check(self, want, what):
        assert self.g.intact(), what + ": a guard was written"
        assert bool((self.full[:, self.data.shape[1]:] == GUARD_VALUE).all()), what + ": a padding column of C was written"
        _same(self.data, want, what)

    def untouched(self, what):
        assert self.g.intact(), what + ": a guard was written"
        assert bool((self.full[:, self.data.shape[1]:] == GUARD_VALUE).all()), what + ": a padding column of C was written"
        assert bool(torch.isnan(self.data).all()), what + ": C was written"


def _same(got, want, what):
    """torch.equal, or which rows and columns differ and by how much (whole numbers: products, bias or prior values)"""
    got = got.double().cpu()
    if torch.equal(got, want):
        return
    d = got - want
    bad = (got != want).nonzero()                # (NaN != anything)
    head = ", ".join("(%d, %d): %+g" % (int(r), int(c), float(d[r, c])) for r, c in bad[:8])
    rws, cls = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, 1].tolist()))
    raise AssertionError("%s: %d of %d elements wrong; rows %s..%s (%d), columns %s..%s (%d); first: %s" % (
        what, len(bad), d.numel(), rws[0], rws[-1], len(rws), cls[0], cls[-1], len(cls), head))


def _act(v, act):
    if act == LRELU:
        return torch.where(v > 0, v, v * SLOPE)
    if act == RELU:
        return v.clamp(min=0.0)
    if act == RELU6:
        return v.clamp(min=0.0, max=6.0)
    assert act == NONE
    return v


def _mask_deriv(y, act):
    """act'(.) taken from the stored activation output y, as the mask epilogue of the grouped rows kernel takes it"""
    if act == LRELU:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    if act == RELU:
        return (y > 0).double()
    if act == TANH:
        return 1.0 - y * y
    return torch.ones_like(y)


def _plan(*req):
    from confignet_amd._lib import lib
    out = (ctypes.c_int * 9)()
    assert lib.cn_gemm_plan(*req, ctypes.byref(out)) == 0, req
    return list(out)


def _pads(i):
    """(A, B, C padded?) of the i-th launch: the eight combinations in turn"""
    return i & 1, i >> 1 & 1, i >> 2 & 1


class Problem:
    """op(A) op(B) on small integers: the float64 product, a bias and a prior value, computed once; A and B on the device with the
    tight and the padded leading dimension"""

    def __init__(self, ta, tb, m, n, k, real=False):
        self.shape = (ta, tb, m, n, k)
        seed = 1000003 * ta + 500009 * tb + 7919 * m + 131 * n + k
        if real:
            gen = torch.Generator().manual_seed(seed)
            a = torch.randn((k, m) if ta else (m, k), generator=gen).double()
            b = torch.randn((n, k) if tb else (k, n), generator=gen).double()
            self.bias, self.prior = torch.randn(n, generator=gen).double(), torch.randn(m, n, generator=gen).double()
        else:
            a, b = _ints((k, m) if ta else (m, k), seed), _ints((n, k) if tb else (k, n), seed + 1)
            self.bias, self.prior = _ints((n,), seed + 2, -2, 2), _ints((m, n), seed + 3, -5, 5)
        oa, ob = a.T if ta else a, b.T if tb else b
        self.prod = oa @ ob
        self.mag = oa.abs() @ ob.abs()
        self.a, self.b = a, b
        self.A = [_op(a, 0), _op(a, 3)]
        self.B = [_op(b, 0), _op(b, 3)]
        self.dbias = self.bias.float().cuda()

    def want(self, bias=0, act=NONE, acc=0):
        v = _act(self.prod + self.bias if bias else self.prod, act)
        return v + self.prior if acc else v

    def launch(self, out, bias=0, act=NONE, acc=0, pads=(0, 0)):
        from confignet_amd import ops
        from confignet_amd._lib import lib
        ta, tb, m, n, k = self.shape
        (A, lda), (B, ldb) = self.A[pads[0]], self.B[pads[1]]
        if acc:
            assert not bias and act == NONE
            return lib.cn_gemm_acc(ta, tb, m, n, k, _p(A), lda, _p(B), ldb, _p(out.data), out.ldc, ops._stream())
        return lib.cn_gemm(ta, tb, m, n, k, _p(A), lda, _p(B), ldb, _p(out.data), out.ldc, _p(self.dbias) if bias else None, act, SLOPE, ops._stream())

    def run(self, route, bias=0, act=NONE, acc=0, pads=(0, 0, 0), slices=None):
        """one call into NaN (or onto the prior value) on the route the test names; returns the plan"""
        from confignet_amd import ops
        ta, tb, m, n, k = self.shape
        req = (ta, tb, m, n, k, n + 5 * pads[2], bias, act, acc, int(ops.DETERMINISTIC))
        what = "ta %d tb %d m %d n %d k %d ldc %d bias %d act %d accumulate %d det %d, A / B padded %d %d" % (req + tuple(pads[:2]))
        plan = _plan(*req)
        assert plan == G.transcribed_plan(*req) and plan[0] == route, (what, plan)
        if slices is not None:
            assert G.slices_of(plan, k)[0] == slices, (what, plan)
        out = Out(m, n, 5 * pads[2], self.prior if acc else None)
        ops.check(self.launch(out, bias, act, acc, pads), "cn_gemm")
        out.check(self.want(bias, act, acc), what)
        return plan


# ---- cn_gemm: rows route ---------------------------------------------------------------------------------------------------
ROWS_M = {8: (1, 8), 16: (9, 16), 32: (17, 32)}


@pytest.mark.parametrize("tb", [0, 1], ids=["nn", "nt"])
@pytest.mark.parametrize("mt", [8, 16, 32])
def test_the_rows_kernels_and_the_tile_kernel_one_past_their_limit(mt, tb):
    """gemm_rows_kernel<MT, TB>: the smallest and the largest m of the instantiation, one and three 64-column blocks with dead
    lanes, K with empty quarters (1, 3), uneven quarters (5, 145) and the LDS limit 8192 / MT; with and without bias, four
    activations.  K = limit + 1 takes the tile kernel (split over K where there is no activation) and gives the same integers."""
    limit = 8192 // mt
    i = 0
    for m in ROWS_M[mt]:
        for n in (5, 63, 64, 65, 130):
            for k in (1, 3, 5, 145, limit, limit + 1):
                P = Problem(0, tb, m, n, k)
                i += 3
                for bias in (0, 1):
                    for act in ACTS:
                        plan = P.run(G.ROWS if k <= limit else G.TILE, bias, act, pads=_pads(i % 8))
                        assert plan[1] == (mt if k <= limit else 0)
                        i += 1


# ---- cn_gemm / cn_gemm_acc: depth route -----------------------------------------------------------------------------------
def test_the_depth_kernel_and_the_tile_kernel_next_to_it():
    """gemm_depth_kernel (A^T B, k <= 32): one and several 16-row x 64-column tiles with dead rows and columns, written and added
    to a prior value; k = 33, and k = 32 with a bias, take the tile kernel with ta."""
    i = 0
    for m in (1, 15, 16, 17, 33):
        for n in (1, 63, 64, 65):
            for k in (1, 31, 32, 33):
                P = Problem(1, 0, m, n, k)
                for acc in (0, 1):
                    for _ in range(2):
                        P.run(G.DEPTH if k <= 32 else G.TILE, acc=acc, pads=_pads(i % 8))
                        i += 1
                if k == 32:
                    P.run(G.TILE, bias=1, pads=_pads(i % 8))


# ---- cn_gemm: thin route --------------------------------------------------------------------------------------------------
THIN_SLICES = {128: 1, 129: 1, 255: 1, 257: 1, 8191: 1, 8192: 2, 8193: 2, 12287: 2, 12289: 3}


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_the_thin_kernel_and_its_k_slices(n):
    """thin_gemm_kernel: one workgroup per (row, K slice), 256 lanes stride K: K of one stride, one element more, one less than two
    strides, and the slice rule at and next to k = 8192 and 12288 (1, 2, 2, 2, 3 slices, the last one shorter); a bias is added
    once however many slices add into C; an activation keeps one slice."""
    i = n
    for m in (1, 3, 256):
        for k in THIN_SLICES:
            if k > 8000 and m > 3:
                continue
            P = Problem(0, 0, m, n, k)
            for bias in (0, 1):
                for _ in range(2):
                    P.run(G.THIN, bias, pads=_pads(i % 8), slices=THIN_SLICES[k])
                    i += 1
            if k in (129, 8192):
                P.run(G.THIN, 1, LRELU, pads=_pads(i % 8), slices=1)
                P.run(G.THIN, 0, RELU6, pads=_pads((i + 5) % 8), slices=1)


def test_the_neighbours_of_the_thin_route_take_the_tile_kernel():
    for i, (m, n, k) in enumerate(((3, 4, 127), (257, 1, 129), (257, 4, 128), (1, 1, 127))):
        P = Problem(0, 0, m, n, k)
        for bias in (0, 1):
            P.run(G.TILE, bias, pads=_pads((3 * i + 5 * bias) % 8))
        P.run(G.TILE, 1, LRELU, pads=_pads((3 * i + 2) % 8))


# ---- cn_gemm / cn_gemm_acc: tile route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["nn", "nt", "tn", "tt"])
def test_the_tile_kernel_with_every_transpose(ta, tb):
    """gemm_kernel: one element, a tile with one row / column short of and past 64, several tiles; K of one element, one short of,
    exactly and one past one 16-deep stage, two stages and a bit, an even number of them with a remainder.  With a bias, with a bias
    and an activation, plain (tn with k <= 32: the depth kernel takes that one) and added to a prior value."""
    i = 2 * ta + tb
    for m, n in ((1, 1), (63, 65), (64, 64), (65, 63), (130, 70)):
        for k in (1, 15, 16, 17, 33, 100):
            P = Problem(ta, tb, m, n, k)
            plain = G.DEPTH if (ta and not tb and k <= 32) else G.TILE
            for bias, act, acc, route in ((1, NONE, 0, G.TILE), (1, LRELU, 0, G.TILE), (1, RELU6, 0, G.TILE), (0, NONE, 0, plain), (0, RELU, 0, G.TILE),
                                          (0, NONE, 1, plain)):
                P.run(route, bias, act, acc, pads=_pads(i % 8), slices=1)
                i += 1


@pytest.mark.parametrize("shape", list(G.SPLITK), ids=lambda s: "x".join(map(str, s)))
def test_split_k_on_the_tile_kernel(shape):
    """K slices added with atomics: behind the zero pass (C holds NaN before the call), with a short last slice, a slice count that
    shrank after rounding to the stage depth, the bias added by the first slice only; onto a prior value without a zero pass."""
    P = Problem(*shape)
    slices = G.SPLITK[shape]
    for bias in (0, 1):
        for i in range(8):
            plan = P.run(G.TILE, bias, pads=_pads(i), slices=slices)
            assert plan[6] == int(slices > 1)
    for i in (0, 3, 5, 6):
        plan = P.run(G.TILE, acc=1, pads=_pads(i), slices=slices)
        assert plan[6] == 0
    P.run(G.TILE, 1, LRELU, pads=_pads(7), slices=1)


def test_accumulating_split_k_keeps_the_prior_value():
    P = Problem(0, 0, 8, 70, 1100)
    for i in (0, 7):
        plan = P.run(G.TILE, acc=1, pads=_pads(i), slices=4)
        assert plan[4:8] == [4, 288, 0, 0]


# ---- deterministic mode ---------------------------------------------------------------------------------------------------
def test_the_ordered_slabs_of_deterministic_mode():
    """The split-K requests again under set_deterministic(True): with ldc = n per-slice slabs in the stream's workspace and the
    ordered sum (which must write all of C: it holds NaN before); with ldc = n + 5 and onto a prior value one slice, the padding
    columns and the prior value respected; the thin kernel at k = 8192 in one slice."""
    from confignet_amd import ops
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        for shape, slices in G.SPLITK.items():
            P = Problem(*shape)
            m, n = shape[2], shape[3]
            for bias in (0, 1):
                for ab in range(4):
                    plan = P.run(G.TILE, bias, pads=_pads(ab), slices=slices)
                    assert plan[6] == 0 and plan[7] == (slices * m * n if slices > 1 else 0)
                plan = P.run(G.TILE, bias, pads=_pads(4 + bias), slices=1)
                assert plan[6] == 0 and plan[7] == 0
            for i in (0, 7):
                plan = P.run(G.TILE, acc=1, pads=_pads(i), slices=1)
                assert plan[6] == 0 and plan[7] == 0
        P = Problem(0, 0, 2, 3, 8192)
        for i in (0, 7):
            P.run(G.THIN, i & 1, pads=_pads(i), slices=1)
    finally:
        ops.set_deterministic(was)
    assert ops.DETERMINISTIC == was


# ---- cn_gemm_rows_grouped -------------------------------------------------------------------------------------------------
ROWS_EPI = (("act", NONE, 0), ("act", LRELU, 1), ("act", RELU, 1), ("act", RELU6, 1), ("mask", LRELU, 1), ("mask", RELU, 0), ("mask", TANH, 1),
            ("mask", NONE, 0))


class RowsJob:
    """one job of cn_gemm_rows_grouped on small integers, its operands padded or tight, and its float64 result"""

    def __init__(self, i, m, n, k, tb, kind, act, bias, padded, out=None, real=False):
        from confignet_amd._lib import CnRowsJob
        seed = 31 * i + 7 * m + 3 * n + k
        if real:
            gen = torch.Generator().manual_seed(seed)
            a, b = torch.randn(m, k, generator=gen).double(), torch.randn((n, k) if tb else (k, n), generator=gen).double()
            self.bias = torch.randn(n, generator=gen).double() if bias else None
        else:
            a, b = _ints((m, k), seed), _ints((n, k) if tb else (k, n), seed + 1)
            self.bias = _ints((n,), seed + 2, -2, 2) if bias else None
        ob = b.T if tb else b
        self.v = a @ ob + (self.bias if bias else 0.0)
        self.mag = a.abs() @ ob.abs() + (self.bias.abs() if bias else 0.0)
        self.kind, self.what = kind, "job %d (m %d n %d k %d tb %d %s act %d bias %d padded %d)" % (i, m, n, k, tb, kind, act, bias, padded)
        (self.A, lda), (self.B, ldb) = _op(a, 3 * padded), _op(b, 3 * padded)
        self.dbias = self.bias.float().cuda() if bias else None
        self.mask = None
        if kind == "mask":
            y = _ints((m, n), seed + 3)
            self.want = self.v * _mask_deriv(y, act)
            self.out = Out(m, n, 5)                       # (the mask shares C's leading dimension)
            self.mask = _op(y, 5)[0]
        elif kind == "acc":
            self.want = None                              # (the owner of the shared C checks the sum)
            self.out = out or Out(m, n, 5 * padded, _ints((m, n), seed + 4, -5, 5))
        else:
            self.want = _act(self.v, act)
            self.out = Out(m, n, 5 * padded)
        self.c = CnRowsJob(a=self.A.data_ptr(), b=self.B.data_ptr(), c=self.out.data.data_ptr(), bias=None if self.dbias is None else self.dbias.data_ptr(),
                           mask=None if self.mask is None else self.mask.data_ptr(), m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=self.out.ldc, tb=tb,
                           act=act, accumulate=int(kind == "acc"), slope=SLOPE)


def _rows_grouped(jobs):
    from confignet_amd import ops
    from confignet_amd._lib import CnRowsJob, lib
    arr = (CnRowsJob * len(jobs))(*[j.c for j in jobs])
    return lib.cn_gemm_rows_grouped(arr, len(jobs), ops._stream())


def _rows_group(cap, count=17):
    """`count` jobs with m <= cap, mixed m, k, n, tb and epilogue; jobs 3 and 9 (one launch) add into one C"""
    M = [m for m in (1, 5, 8, 9, 16, 17, 32) if m <= cap]
    K, N = (1, 3, 64, 145, 256), (1, 4, 63, 64, 65, 300)
    jobs = []
    for i in range(count):
        m, n, k, tb = M[i % len(M)], N[i % 6], K[i % 5], i % 2
        kind, act, bias = ROWS_EPI[i % 8]
        if i == 3:
            jobs.append(RowsJob(i, m, n, k, tb, "acc", NONE, 0, 1))
        elif i == 9:
            jobs.append(RowsJob(i, jobs[3].out.data.shape[0], jobs[3].out.data.shape[1], k, tb, "acc", NONE, 0, 0, out=jobs[3].out))
        else:
            jobs.append(RowsJob(i, m, n, k, tb, kind, act, bias, (i >> 1) & 1))
    return jobs


@pytest.mark.parametrize("cap", [8, 16, 32])
def test_the_grouped_rows_kernels_on_mixed_groups(cap):
    """17 jobs in one call: a launch of 16 whose MT comes from its largest m (the cap: 8, 16, 32 -- with k = 256 next to it the
    MT = 32 group sits exactly at the LDS limit) and whose LDS block is sized by its largest k while every job places its partial
    sums behind MT x its OWN k, and a launch of one job with another MT.  m, k, n (one to five column blocks) and tb mixed within
    the group; the epilogues: activation, the mask product with the LeakyReLU / ReLU / tanh / no derivative (mask and C at
    ldc = n + 5), and two jobs of one launch adding into one C onto a prior value."""
    from confignet_amd import ops
    jobs = _rows_group(cap)
    assert max(j.c.m for j in jobs[:16]) == cap and max(j.c.k for j in jobs[:16]) == 256 and len({j.c.k for j in jobs[:16]}) == 5
    assert cap == 8 or jobs[16].c.m <= 8                     # (the second launch is instantiated for fewer rows)
    prior = jobs[3].out.data.double().cpu()
    ops.check(_rows_grouped(jobs), "cn_gemm_rows_grouped")
    for j in jobs:
        if j.kind != "acc":
            j.out.check(j.want, j.what)
    jobs[3].out.check(prior + jobs[3].v + jobs[9].v, jobs[3].what + " + " + jobs[9].what)


def test_a_grouped_rows_launch_exactly_at_the_lds_limit():
    """m <= 8 with k = 1024: MT x k = 8192 floats, accepted; next to jobs with a short k in the same launch"""
    from confignet_amd import ops
    jobs = [RowsJob(0, 8, 65, 1024, 0, "act", LRELU, 1, 1), RowsJob(1, 1, 130, 1024, 1, "act", NONE, 0, 0), RowsJob(2, 5, 63, 3, 0, "mask", TANH, 1, 1),
            RowsJob(3, 7, 4, 1023, 1, "act", RELU6, 1, 0)]
    ops.check(_rows_grouped(jobs), "cn_gemm_rows_grouped")
    for j in jobs:
        j.out.check(j.want, j.what)


# ---- cn_gemm_depth_grouped ------------------------------------------------------------------------------------------------
class DepthJob:
    def __init__(self, i, m, n, k, padded, out=None, real=False):
        from confignet_amd._lib import CnDepthJob
        seed = 17 * i + 5 * m + 3 * n + k
        if real:
            gen = torch.Generator().manual_seed(seed)
            a, b, prior = torch.randn(k, m, generator=gen).double(), torch.randn(k, n, generator=gen).double(), torch.randn(m, n, generator=gen).double()
        else:
            a, b, prior = _ints((k, m), seed), _ints((k, n), seed + 1), _ints((m, n), seed + 2, -5, 5)
        self.v = a.T @ b
        self.mag = a.T.abs() @ b.abs()
        self.what = "job %d (m %d n %d k %d padded %d)" % (i, m, n, k, padded)
        (self.A, lda), (self.B, ldb) = _op(a, 3 * padded), _op(b, 3 * padded)
        self.prior = None if out else prior
        self.out = out or Out(m, n, 5 * padded, prior)
        self.c = CnDepthJob(a=self.A.data_ptr(), b=self.B.data_ptr(), c=self.out.data.data_ptr(), m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=self.out.ldc)


def _depth_grouped(jobs):
    from confignet_amd import ops
    from confignet_amd._lib import CnDepthJob, lib
    arr = (CnDepthJob * len(jobs))(*[j.c for j in jobs])
    return lib.cn_gemm_depth_grouped(arr, len(jobs), ops._stream())


def test_the_grouped_depth_kernel_against_float64():
    """65 jobs: a launch of 64 and a launch of one.  One to three 16-row tiles and one to three 64-column tiles per job with dead
    rows and columns, k of 1, 7 and 32, padded and tight leading dimensions; every C holds an integer prior value and jobs 7 and 20
    (one launch) add into one C.  Each job is compared with the float64 A^T B + prior, not with cn_gemm_acc."""
    from confignet_amd import ops
    M, N, K = (1, 15, 16, 17, 40), (1, 63, 64, 65, 130), (1, 7, 32)
    jobs = []
    for i in range(65):
        m, n, k = M[i % 5], N[(i + i // 5) % 5], K[i % 3]
        if i == 20:
            jobs.append(DepthJob(i, jobs[7].c.m, jobs[7].c.n, k, 0, out=jobs[7].out))
        else:
            jobs.append(DepthJob(i, m, n, k, (i >> 1) & 1))
    assert {(j.c.m, j.c.n) for j in jobs} >= {(m, n) for m in M for n in N}
    ops.check(_depth_grouped(jobs), "cn_gemm_depth_grouped")
    for i, j in enumerate(jobs):
        if i not in (7, 20):
            j.out.check(j.prior + j.v, j.what)
    jobs[7].out.check(jobs[7].prior + jobs[7].v + jobs[20].v, jobs[7].what + " + " + jobs[20].what)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refused_requests_write_nothing():
    """a leading dimension below the extent (each of lda, ldb, ldc, with and without a transpose), a rows job with m = 33, a rows
    group whose MT x largest k passes 8192 floats (m <= 8 with k = 1025: the first k past the limit; and m = 9 with k = 3 next to
    m = 1 with k = 513: each job alone would fit), a depth job with k = 33, accumulate together with a bias or a mask: CN_EINVAL, C
    keeps its NaN, the guards their sentinel."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    for ta, tb in ((0, 0), (1, 1)):
        m, n, k = 5, 7, 9
        P = Problem(ta, tb, m, n, k)
        (A, lda), (B, ldb) = P.A[1], P.B[1]
        for dla, dlb, dlc in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            out = Out(m, n, 5)
            bad = ((m if ta else k) - 1 if dla else lda, (k if tb else n) - 1 if dlb else ldb, n - 1 if dlc else out.ldc)
            assert lib.cn_gemm(ta, tb, m, n, k, _p(A), bad[0], _p(B), bad[1], _p(out.data), bad[2], None, NONE, SLOPE, ops._stream()) == CN_EINVAL, bad
            assert lib.cn_gemm_acc(ta, tb, m, n, k, _p(A), bad[0], _p(B), bad[1], _p(out.data), bad[2], ops._stream()) == CN_EINVAL, bad
            out.untouched("cn_gemm ta %d tb %d ld %s" % (ta, tb, bad))
    groups = {"m = 33": [RowsJob(0, 33, 65, 5, 0, "act", NONE, 0, 0)],
              "8 x 1025": [RowsJob(0, 8, 65, 1025, 0, "act", NONE, 0, 0)],
              "16 x 513": [RowsJob(0, 9, 65, 3, 0, "act", NONE, 0, 0), RowsJob(1, 1, 65, 513, 0, "act", NONE, 0, 0)],
              "lda": [RowsJob(0, 8, 65, 5, 0, "act", NONE, 0, 0)], "ldb": [RowsJob(0, 8, 65, 5, 1, "act", NONE, 0, 0)], "ldc": [RowsJob(0, 8, 65, 5, 0, "act", NONE, 0, 0)],
              "accumulate + bias": [RowsJob(0, 8, 65, 5, 0, "act", NONE, 1, 0)], "accumulate + mask": [RowsJob(0, 8, 65, 5, 0, "mask", LRELU, 0, 0)]}
    groups["lda"][0].c.lda, groups["ldb"][0].c.ldb, groups["ldc"][0].c.ldc = 4, 4, 64
    groups["accumulate + bias"][0].c.accumulate = groups["accumulate + mask"][0].c.accumulate = 1
    for name, jobs in groups.items():
        assert _rows_grouped(jobs) == CN_EINVAL, name
        for j in jobs:
            j.out.untouched("rows group " + name)
    for name, k, field in (("k = 33", 33, None), ("lda", 5, "lda"), ("ldb", 5, "ldb"), ("ldc", 5, "ldc")):
        j = DepthJob(0, 17, 65, k, 0)
        j.out.data.fill_(NAN)
        if field:
            setattr(j.c, field, getattr(j.c, field) - 1)
        assert _depth_grouped([j]) == CN_EINVAL, name
        j.out.untouched("depth group " + name)


# ---- rounding pass --------------------------------------------------------------------------------------------------------
_RATIOS = {}               # kernel -> (largest error / bound, where)


def _ratio(got, ref, mag, k, s):
    """largest |got - ref| / bound over the elements, bound = 2 (K + S + 2) 2^-24 A"""
    err = (got.double().cpu() - ref).abs()
    return float((err / (2.0 * (k + s + 2) * 2.0 ** -24 * mag)).max())


def _note(kernel, ratio, where):
    if kernel not in _RATIOS or not ratio <= _RATIOS[kernel][0]:
        _RATIOS[kernel] = (ratio, where)
    path = os.environ.get("GEMM_EDGE_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("Rounding pass of tests/test_gemm_edges_gpu.py, one MI355X (written when GEMM_EDGE_ERRORS names a path): standard-normal\n"
                    "operands, bias and prior value, one case per kernel at its edge shape with the most slices.  ratio = the largest\n"
                    "|got - ref|_ij / (2 (K + S + 2) 2^-24 A_ij) over the elements of every launch of the kernel (A = the float64 product of |A| and\n"
                    "|B| plus |bias| plus |prior|, S = K quarters, K slices or slabs); the test holds every ratio at <= 1.\n\n")
            f.write("%-28s %10s   %s\n" % ("kernel", "ratio", "largest at"))
            for k, (r, w) in sorted(_RATIOS.items()):
                f.write("%-28s %10.3e   %s\n" % (k, r, w))


def _real_case(kernel, shape, s, bias=0, acc=0, det=False):
    from confignet_amd import ops
    ta, tb, m, n, k = shape
    P = Problem(*shape, real=True)
    was = ops.DETERMINISTIC
    ops.set_deterministic(det)
    try:
        req = (ta, tb, m, n, k, n, bias, NONE, acc, int(det))
        plan = _plan(*req)
        assert G.slices_of(plan, k)[0] == (1 if plan[0] in (G.ROWS, G.DEPTH) else s), plan
        out = Out(m, n, 0, P.prior if acc else None)
        ops.check(P.launch(out, bias, NONE, acc), "cn_gemm")
    finally:
        ops.set_deterministic(was)
    mag = P.mag + (P.bias.abs() if bias else 0.0) + (P.prior.abs() if acc else 0.0)
    r = _ratio(out.data, P.want(bias, NONE, acc), mag, k, s)
    where = "%s m %d n %d k %d, %d slices, bias %d prior %d%s" % ("nt"[ta] + "nt"[tb], m, n, k, s, bias, acc, " deterministic" if det else "")
    print("%s %s: error / bound %.3e" % (kernel, where, r))
    _note(kernel, r, where)
    return r, where


ROUNDING = {
    "gemm_kernel": [((0, 0, 33, 5, 4609), 17, 1, 0, False), ((0, 0, 33, 5, 4609), 17, 0, 1, False), ((0, 0, 33, 5, 4609), 17, 1, 0, True),
                    ((1, 0, 70, 130, 2049), 8, 1, 0, False)],
    "thin_gemm_kernel": [((0, 0, 2, 2, 12289), 3, 1, 0, False)],
    "gemm_rows_kernel": [((0, 0, 8, 130, 1024), 4, 1, 0, False), ((0, 1, 32, 130, 256), 4, 1, 0, False)],
    "gemm_depth_kernel": [((1, 0, 33, 65, 32), 1, 0, 1, False)],
}


@pytest.mark.parametrize("kernel", list(ROUNDING))
def test_the_arithmetic_stays_within_the_fp32_summation_bound(kernel):
    over = []
    for shape, s, bias, acc, det in ROUNDING[kernel]:
        r, where = _real_case(kernel, shape, s, bias, acc, det)
        if not r <= 1.0:
            over.append((where, r))
    assert not over, over


def test_the_grouped_kernels_stay_within_the_fp32_summation_bound():
    """the rows kernels' arithmetic in the grouped launch (K quarters: S = 4), the depth kernel's onto a prior value (S = 1)"""
    from confignet_amd import ops
    rows = [RowsJob(0, 8, 130, 1024, 0, "act", NONE, 1, 0, real=True), RowsJob(1, 5, 65, 1024, 1, "act", NONE, 1, 1, real=True)]
    ops.check(_rows_grouped(rows), "cn_gemm_rows_grouped")
    depth = [DepthJob(0, 40, 130, 32, 0, real=True), DepthJob(1, 17, 65, 32, 1, real=True)]
    ops.check(_depth_grouped(depth), "cn_gemm_depth_grouped")
    over = []
    for kernel, jobs, s in (("gemm_rows_grouped_kernel", rows, 4), ("gemm_depth_grouped_kernel", depth, 1)):
        for j in jobs:
            prior = 0.0 if s == 4 else j.prior
            r = _ratio(j.out.data, j.v + prior, j.mag + (0.0 if s == 4 else j.prior.abs()), j.c.k, s)
            print("%s %s: error / bound %.3e" % (kernel, j.what, r))
            _note(kernel, r, j.what)
            if not r <= 1.0:
                over.append((j.what, r))
    assert not over, over
