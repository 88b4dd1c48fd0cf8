"""cn_gemm_rows_grouped_k (csrc/gemm.hip): the grouped rows product for any k.  A launch whose MT x largest k passes 8192 floats runs
gemm_rows_grouped_ksteps_kernel<8 | 16 | 32>, which stages A in chunks of KC = 8192 / MT columns; wave q sums quarter q of every
chunk into registers that persist across the chunks, and the K quarters are combined once after the last chunk.  Everything here goes
through `lib` directly, in the style of tests/test_gemm_edges_gpu.py, whose helpers it uses.

Exact pass: integer inputs in [-3, 3], integer bias in [-2, 2], an integer prior value in [-5, 5] where C is accumulated into, slope
0.25, mask values in [-3, 3].  Every term is a multiple of 1/4 below 9 K + 7 in size and K <= 3071 (3 KC - 1 at MT = 8), so
4 |sum| < 2^24: fp32 holds every partial sum exactly in any order, and each result is compared with the float64 reference by
torch.equal.  One dropped or doubled column at a chunk edge, one chunk read at the wrong offset of A or B, one quarter summed from a
stale chunk shows as a whole number.  Operands are views with NaN padding (tight and ld = extent + 3), C sits between guards with
sentinel padding columns and holds NaN before a call that must write it.

Rounding pass: standard-normal operands and bias, |got - ref|_ij <= 2 (K + S + 2) 2^-24 A_ij with S = 4: the kernel combines the K
quarters ONCE, after the last chunk (not per chunk), so S is the four combining adds of the one-chunk kernels whatever the chunk
count.  The largest error / bound goes to profiles/gemm_rows_ksteps_errors.txt when GEMM_ROWS_KSTEPS_ERRORS names a path."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_rows_ksteps_notes as NOTES
from tests.test_gemm_edges_gpu import CN_EINVAL, LRELU, NONE, RELU, RELU6, ROWS_EPI, TANH, RowsJob, _ratio, _rows_group, _rows_grouped

SHORT_M = {8: 5, 16: 9, 32: 17}
PLAN_FIELDS = 8


def _rows_grouped_k(jobs):
    from confignet_amd import ops
    from confignet_amd._lib import CnRowsJob, lib
    arr = (CnRowsJob * len(jobs))(*[j.c for j in jobs])
    return lib.cn_gemm_rows_grouped_k(arr, len(jobs), ops._stream())


def _plan(jobs):
    from confignet_amd._lib import CnRowsJob, lib
    arr = (CnRowsJob * len(jobs))(*[j.c for j in jobs])
    launches = (len(jobs) + 15) // 16
    out, n = (ctypes.c_int * (PLAN_FIELDS * launches))(), ctypes.c_int()
    assert lib.cn_gemm_rows_grouped_plan(arr, len(jobs), out, len(out), ctypes.byref(n)) == 0 and n.value == launches
    return [list(out)[PLAN_FIELDS * i:PLAN_FIELDS * (i + 1)] for i in range(launches)]


def _run(jobs):
    from confignet_amd import ops
    ops.check(_rows_grouped_k(jobs), "cn_gemm_rows_grouped_k")


# ---- chunk edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [0, 1], ids=["nn", "nt"])
@pytest.mark.parametrize("mt", [8, 16, 32])
def test_the_chunk_edges_of_every_instantiation(mt, tb):
    """one job per launch: k = KC + 1 (a second chunk of one column: waves 1..3 have nothing in it), 2 KC, 2 KC + 5 (a ragged last
    chunk whose length is no multiple of 4), 3 KC - 1; m = MT and a short m with dead rows; one to three column blocks with dead
    lanes; tight and padded leading dimensions; bias and activation in turn"""
    kc = 8192 // mt
    i = 0
    for k, chunks in ((kc + 1, 2), (2 * kc, 2), (2 * kc + 5, 3), (3 * kc - 1, 3)):
        for m in (mt, SHORT_M[mt]):
            for n in (1, 63, 64, 65, 130):
                for padded in (0, 1):
                    kind, act, bias = ROWS_EPI[i % 4]
                    j = RowsJob(i, m, n, k, tb, kind, act, bias, padded)
                    assert _plan([j]) == [[0, 1, mt, kc, chunks, (n + 63) // 64, 4 * (8192 + 3 * mt * 64), 1]], j.what
                    _run([j])
                    j.out.check(j.want, j.what)
                    i += 1


# ---- epilogues --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", [8, 16, 32])
def test_the_three_epilogues_behind_several_chunks(mt):
    """activation + bias (none, LeakyReLU, ReLU, ReLU6), the mask product (LeakyReLU, ReLU, tanh, no derivative; mask and C at
    ldc = n + 5), and two jobs of one launch adding into one C onto an integer prior value -- every job with 3 chunks"""
    kc = 8192 // mt
    k, m = 2 * kc + 5, SHORT_M[mt] + 2
    jobs = [RowsJob(i, m, 65 + i, k, i & 1, "act", act, 1, (i >> 1) & 1) for i, act in enumerate((NONE, LRELU, RELU, RELU6))]
    jobs += [RowsJob(4 + i, m, 65 + i, k, i & 1, "mask", act, i & 1, 1) for i, act in enumerate((LRELU, RELU, TANH, NONE))]
    first = RowsJob(8, m, 130, k, 0, "acc", NONE, 0, 1)
    jobs += [first, RowsJob(9, m, 130, k - 7, 1, "acc", NONE, 0, 0, out=first.out)]
    assert all(j.out.ldc == j.c.n + 5 for j in jobs[4:8])
    (p,) = _plan(jobs)
    assert p[2:5] == [mt, kc, 3] and p[7] == 1
    prior = first.out.data.double().cpu()
    _run(jobs)
    for j in jobs[:8]:
        j.out.check(j.want, j.what)
    first.out.check(prior + first.v + jobs[9].v, first.what + " + " + jobs[9].what)


# ---- a mixed launch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 16, 32])
def test_a_mixed_call_of_sixteen_and_one_jobs(cap):
    """17 jobs: a launch of 16 whose MT comes from its largest m and in which k = 3 and 64 sit next to KC + 1 and 2 KC + 5, so the
    workgroups of one grid run one, two and three chunks; m, n (one to five column blocks), tb and the epilogues mixed, jobs 3 and 9
    adding into one C; then a launch of one job with MT = 8 and its own chunk length"""
    kc = 8192 // cap
    M = [m for m in (1, 5, 8, 9, 16, 17, 32) if m <= cap]
    K, N = (3, 2 * kc + 5, 64, kc + 1, 145), (1, 4, 63, 64, 65, 300)
    jobs = []
    for i in range(16):
        m, n, k, tb = M[i % len(M)], N[i % 6], K[i % 5], i % 2
        kind, act, bias = ROWS_EPI[i % 8]
        if i == 3:
            jobs.append(RowsJob(i, m, n, k, tb, "acc", NONE, 0, 1))
        elif i == 9:
            jobs.append(RowsJob(i, jobs[3].out.data.shape[0], jobs[3].out.data.shape[1], k, tb, "acc", NONE, 0, 0, out=jobs[3].out))
        else:
            jobs.append(RowsJob(i, m, n, k, tb, kind, act, bias, (i >> 1) & 1))
    jobs.append(RowsJob(16, 5, 130, 1029, 1, "act", LRELU, 1, 1))
    assert max(j.c.m for j in jobs[:16]) == cap and {j.c.k for j in jobs[:16]} == set(K)
    a, b = _plan(jobs)
    assert a[:5] == [0, 16, cap, kc, 3] and a[7] == 1 and a[5] == sum((j.c.n + 63) // 64 for j in jobs[:16])
    assert b == [16, 1, 8, 1024, 2, 3, 4 * (8192 + 3 * 8 * 64), 1]
    prior = jobs[3].out.data.double().cpu()
    _run(jobs)
    for j in jobs:
        if j.kind != "acc":
            j.out.check(j.want, j.what)
    jobs[3].out.check(prior + jobs[3].v + jobs[9].v, jobs[3].what + " + " + jobs[9].what)


# ---- what the first entry refuses ---------------------------------------------------------------------------------------------
def test_the_two_groups_the_whole_block_entry_refuses():
    """m <= 8 with k = 1025, and m = 9 with k = 3 next to m = 1 with k = 513: cn_gemm_rows_grouped still answers CN_EINVAL and writes
    nothing; cn_gemm_rows_grouped_k gives the float64 result"""
    groups = {"8 x 1025": [RowsJob(0, 8, 65, 1025, 0, "act", NONE, 0, 0)],
              "16 x 513": [RowsJob(0, 9, 65, 3, 0, "act", NONE, 0, 0), RowsJob(1, 1, 65, 513, 0, "act", NONE, 0, 0)]}
    for name, jobs in groups.items():
        assert _rows_grouped(jobs) == CN_EINVAL, name
        for j in jobs:
            j.out.untouched("rows group " + name)
        (p,) = _plan(jobs)
        assert p[4] == 2 and p[7] == 1, (name, p)
        _run(jobs)
        for j in jobs:
            j.out.check(j.want, j.what)


# ---- same bits where the whole block fits ---------------------------------------------------------------------------------------
def _real_rows_group(cap):
    """the shapes and epilogues of _rows_group(cap) on standard-normal inputs; job 9 adds into a C of its own (two atomic adds
    into one element commute only in exact arithmetic, and the order of two workgroups is not the launch's to fix)"""
    M = [m for m in (1, 5, 8, 9, 16, 17, 32) if m <= cap]
    K, N = (1, 3, 64, 145, 256), (1, 4, 63, 64, 65, 300)
    jobs = []
    for i in range(17):
        m, n, k, tb = M[i % len(M)], N[i % 6], K[i % 5], i % 2
        kind, act, bias = ROWS_EPI[i % 8]
        if i in (3, 9):
            kind, act, bias = "acc", NONE, 0
        jobs.append(RowsJob(i, m, n, k, tb, kind, act, bias, (i >> 1) & 1, real=True))
    return jobs


@pytest.mark.parametrize("cap", [8, 16, 32])
def test_groups_that_fit_the_whole_block_give_the_bits_of_the_first_entry(cap):
    """ksteps = 0 for both launches of the call: the same kernel with the same launch arguments.  Standard-normal inputs, every
    output compared bit for bit (guards and padding columns included), and the integer group of tests/test_gemm_edges_gpu.py as well"""
    from confignet_amd import ops
    for build in (_real_rows_group, _rows_group):
        old, new = build(cap), build(cap)
        assert [p[7] for p in _plan(new)] == [0, 0]
        for a, b in zip(old, new):                         # (the same seeds: the same operands and prior values)
            assert torch.equal(a.A, b.A) and torch.equal(a.B, b.B)
        ops.check(_rows_grouped(old), "cn_gemm_rows_grouped")
        _run(new)
        for a, b in zip(old, new):
            assert a.out.g.intact() and b.out.g.intact(), a.what
            assert not bool(torch.isnan(b.out.data).any()), a.what
            assert torch.equal(a.out.full.view(torch.int32), b.out.full.view(torch.int32)), a.what


def test_the_short_jobs_of_a_chunked_launch_stay_within_the_bound_of_the_whole_block_kernel():
    """a launch that takes the chunked kernel because of ONE long job: its short jobs (k <= KC: one chunk) run the multiply-adds of
    gemm_rows_grouped_kernel in its order and are held to the same fp32 bound (S = 4) against float64.  They are NOT asserted bit-equal
    to the first entry: measured on one MI355X, 190 of 4160 and 81 of 2048 elements of the two 32-row jobs differ, all in rows 30 and
    31 (a probe of the same shapes), by at most 5.7e-6 -- one rounding, where hipcc fuses the multiply-add of one kernel and not
    of the other --, and no element of the other four jobs.  The count is printed."""
    from confignet_amd import ops
    def short():
        return [RowsJob(i, m, n, k, i & 1, "act", NONE, 1, i & 1, real=True) for i, (m, n, k) in
                enumerate(((32, 130, 256), (17, 65, 145), (24, 300, 255), (1, 4, 3), (20, 63, 1), (32, 64, 128)))]
    old, new = short(), short() + [RowsJob(6, 32, 65, 257, 0, "act", NONE, 1, 0, real=True)]
    assert [p[7] for p in _plan(old)] == [0] and [p[7] for p in _plan(new)] == [1]
    ops.check(_rows_grouped(old), "cn_gemm_rows_grouped")
    _run(new)
    over = []
    for a, b in zip(old, new):
        differ = int((a.out.data.view(torch.int32) != b.out.data.view(torch.int32)).sum())
        ra, rb = _ratio(a.out.data, a.v, a.mag, a.c.k, 4), _ratio(b.out.data, b.v, b.mag, b.c.k, 4)
        print("%s: error / bound whole block %.3e, chunked launch %.3e; %d of %d elements differ" % (a.what, ra, rb, differ, a.out.data.numel()))
        if not (ra <= 1.0 and rb <= 1.0):
            over.append((a.what, ra, rb))
    assert not over, over


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    """m = 33, each leading dimension one short, accumulate with a bias or a mask: CN_EINVAL, every C keeps its NaN.  Alone, and as
    the last of 17 jobs: every job is checked before the first launch, so the 16 valid jobs in front (a whole launch of their own)
    are not run either"""
    def bad():
        g = {"m = 33": RowsJob(0, 33, 65, 5, 0, "act", NONE, 0, 0), "lda": RowsJob(0, 8, 65, 5, 0, "act", NONE, 0, 0),
             "ldb": RowsJob(0, 8, 65, 5, 0, "act", NONE, 0, 0), "ldb, transposed": RowsJob(0, 8, 65, 5, 1, "act", NONE, 0, 0),
             "ldc": RowsJob(0, 8, 65, 5, 0, "act", NONE, 0, 0), "accumulate + bias": RowsJob(0, 8, 65, 5, 0, "act", NONE, 1, 0),
             "accumulate + mask": RowsJob(0, 8, 65, 5, 0, "mask", LRELU, 0, 0)}
        g["lda"].c.lda, g["ldb"].c.ldb, g["ldb, transposed"].c.ldb, g["ldc"].c.ldc = 4, 64, 4, 64
        g["accumulate + bias"].c.accumulate = g["accumulate + mask"].c.accumulate = 1
        return g
    for name, j in bad().items():
        assert _rows_grouped_k([j]) == CN_EINVAL, name
        j.out.untouched("alone: " + name)
    valid = [RowsJob(i, 8 + i, 65, 700 + i, i & 1, "act", NONE, 1, i & 1) for i in range(16)]
    for name, j in bad().items():
        assert _rows_grouped_k(valid + [j]) == CN_EINVAL, name
        for v in valid + [j]:
            v.out.untouched("last of 17: " + name)
    _run(valid)                                            # (the same jobs without the bad one do run)
    for v in valid:
        v.out.check(v.want, v.what)


# ---- rounding pass ----------------------------------------------------------------------------------------------------------
ROUNDING = ((24, 300, 512, 0), (32, 130, 1024, 1), (17, 65, 2053, 0))


def test_the_chunked_sums_stay_within_the_fp32_summation_bound():
    """S = 4: per output element K products summed in fp32 in four register chains (one per wave, running across the chunks), three
    adds that combine them and one for the bias -- the bound of the one-chunk kernels, unchanged by the chunk count (2, 4 and 9 here)"""
    jobs = [RowsJob(i, m, n, k, tb, "act", NONE, 1, i & 1, real=True) for i, (m, n, k, tb) in enumerate(ROUNDING)]
    over = []
    for j in jobs:                                         # (one launch each: MT = 32 and KC = 256 for all three)
        (p,) = _plan([j])
        assert p[7] == 1 and p[4] == (j.c.k + 255) // 256
        _run([j])
        r = _ratio(j.out.data, j.v, j.mag, j.c.k, 4)
        print("gemm_rows_grouped_ksteps_kernel %s, %d chunks: error / bound %.3e" % (j.what, p[4], r))
        NOTES.note("rounding", j.what, "%-36s %10.3e   %s, %d chunks" % ("gemm_rows_grouped_ksteps_kernel<32>", r, j.what, p[4]))
        if not r <= 1.0:
            over.append((j.what, r))
    assert not over, over
