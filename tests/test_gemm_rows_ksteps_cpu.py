"""The launches of cn_gemm_rows_grouped_k (csrc/gemm.hip: plan_rows_group is the function the call decides with), checked without a
GPU through cn_gemm_rows_grouped_plan: eight ints per launch of up to 16 jobs -- first job, jobs, MT, KC, chunks of the largest k,
workgroups, dynamic LDS bytes, ksteps.  ksteps = 0 is the launch of cn_gemm_rows_grouped (the whole A block [MT][kmax] in LDS, then
the partial sums [3][MT][64]); ksteps = 1 is gemm_rows_grouped_ksteps_kernel: a fixed block of MT x KC = 8192 floats through which A
goes in chunks, and the same partial sums behind it.

The expected plans of the first test are written by hand from that description, not taken from the library."""
import ctypes

import pytest

from confignet_amd._lib import CnRowsJob, lib

CN_EINVAL = -1
FIRST, COUNT, MT, KC, CHUNKS, GRID, LDS, KSTEPS = range(8)


def cdiv(a, b):
    return (a + b - 1) // b


def job(m, n, k, tb=0, **kw):
    """a job as the plan query reads it: the pointers stay NULL"""
    f = dict(m=m, n=n, k=k, lda=k, ldb=k if tb else n, ldc=n, tb=tb, act=0, accumulate=0, slope=0.0)
    f.update(kw)
    return CnRowsJob(**f)


def query(jobs, cap=None):
    arr = (CnRowsJob * len(jobs))(*jobs)
    cap = 8 * cdiv(len(jobs), 16) if cap is None else cap
    out = (ctypes.c_int * max(cap, 1))(*([-7] * max(cap, 1)))
    n = ctypes.c_int(-7)
    rc = lib.cn_gemm_rows_grouped_plan(arr, len(jobs), out, cap, ctypes.byref(n))
    return rc, n.value, list(out)


def plans(jobs):
    rc, n, out = query(jobs)
    assert rc == 0 and n == cdiv(len(jobs), 16), (rc, n)
    return [out[8 * i:8 * i + 8] for i in range(n)]


def rows_lds(mt, k):
    """gemm_rows_lds of csrc/gemm.hip"""
    return 4 * (mt * k + 3 * mt * 64)


def test_the_plans_written_by_hand():
    # 24 rows, k = 512 (the AdaIN bank's backward at the default batch): 32 x 256 floats of A per chunk + 3 x 32 x 64 partial sums
    assert plans([job(24, 300, 512)]) == [[0, 1, 32, 256, 2, 5, 57344, 1]]
    # exactly at the limit of the whole-block launch, and one column past it
    assert plans([job(8, 65, 1024)]) == [[0, 1, 8, 1024, 1, 2, rows_lds(8, 1024), 0]]
    assert rows_lds(8, 1024) == 38912
    assert plans([job(8, 65, 1025)]) == [[0, 1, 8, 1024, 2, 2, 38912, 1]]
    # each job alone would fit (16 x 3, 8 x 513); together MT = 16 meets k = 513
    assert plans([job(9, 65, 3), job(1, 65, 513)]) == [[0, 2, 16, 512, 2, 4, 4 * (8192 + 3 * 16 * 64), 1]]
    # 17 jobs: 16 + 1, the second launch with its own MT, k and grid
    jobs = [job(17 if i == 4 else 3, 64 + i, 300 if i == 7 else 5) for i in range(16)] + [job(8, 130, 2000, tb=1)]
    a, b = plans(jobs)
    assert a == [0, 16, 32, 256, 2, 1 + 15 * 2, 57344, 1]
    assert b == [16, 1, 8, 1024, 2, 3, 38912, 1]
    # a short group keeps today's launch, LDS sized by its largest k
    assert plans([job(16, 64, 145), job(5, 1, 512, tb=1)]) == [[0, 2, 16, 512, 1, 2, rows_lds(16, 512), 0]]
    assert plans([]) == []


def test_the_invariants_of_every_plan():
    ks = (1, 255, 256, 257, 1024, 1025, 4097)
    ns = (1, 63, 64, 65, 300)
    seen = set()
    for m in range(1, 33):
        for i, k in enumerate(ks):
            # a single job, and a mixed group in which this job has the largest m but not always the largest k
            others = [job(1 + (m * 7 + q) % m, ns[(q + i) % 5], ks[(i + q) % 7], tb=q & 1) for q in range(3)]
            for jobs in ([job(m, ns[(m + i) % 5], k)], [job(m, ns[(m + i) % 5], k, tb=1)] + others):
                (p,) = plans(jobs)
                mmax, kmax = max(j.m for j in jobs), max(j.k for j in jobs)
                assert mmax == m
                mt = 8 if m <= 8 else 16 if m <= 16 else 32
                assert p[FIRST] == 0 and p[COUNT] == len(jobs) and p[MT] == mt
                assert p[MT] * p[KC] == 8192
                assert p[CHUNKS] == cdiv(kmax, p[KC]) >= 1
                assert p[GRID] == sum(cdiv(j.n, 64) for j in jobs)
                assert p[KSTEPS] == (0 if mt * kmax <= 8192 else 1)       # 0 exactly where cn_gemm_rows_grouped accepts
                assert p[LDS] == (rows_lds(mt, p[KC]) if p[KSTEPS] else rows_lds(mt, kmax)) <= 65536
                assert p[KSTEPS] == 1 or p[CHUNKS] == 1
                seen.add((mt, p[KSTEPS], p[CHUNKS]))
    assert {(mt, s) for mt, s, _ in seen} == {(mt, s) for mt in (8, 16, 32) for s in (0, 1)}
    assert max(c for _, _, c in seen) == cdiv(4097, 256)


def test_long_calls_are_cut_into_runs_of_sixteen():
    jobs = [job(1 + i % 32, 1 + 7 * i, 1 + 97 * i) for i in range(35)]
    ps = plans(jobs)
    assert [(p[FIRST], p[COUNT]) for p in ps] == [(0, 16), (16, 16), (32, 3)]
    for p in ps:
        run = jobs[p[FIRST]:p[FIRST] + p[COUNT]]
        m, k = max(j.m for j in run), max(j.k for j in run)
        assert p[MT] == (8 if m <= 8 else 16 if m <= 16 else 32) and p[CHUNKS] == cdiv(k, p[KC]) and p[GRID] == sum(cdiv(j.n, 64) for j in run)


BAD = {"m = 33": job(33, 65, 5), "m = 0": job(0, 65, 5), "n = 0": job(8, 0, 5), "k = 0": job(8, 65, 0), "lda": job(8, 65, 5, lda=4),
       "ldb": job(8, 65, 5, ldb=64), "ldb, transposed": job(8, 65, 5, tb=1, ldb=4), "ldc": job(8, 65, 5, ldc=64),
       "accumulate + bias": job(8, 65, 5, accumulate=1, bias=64), "accumulate + mask": job(8, 65, 5, accumulate=1, mask=64),
       "accumulate + activation": job(8, 65, 5, accumulate=1, act=1)}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_jobs_are_argument_errors_of_the_plan_and_of_the_call(name):
    """CN_EINVAL from the plan query, which leaves out and nlaunches alone; and from the call itself, which checks every job before
    it touches a device (here there is none): alone, and last behind 16 valid jobs, i.e. in a second launch"""
    good = [job(8, 65, 700, a=64, b=64, c=64) for _ in range(16)]
    bad = BAD[name]
    for jobs in ([bad], good + [bad]):
        rc, n, out = query(jobs)
        assert rc == CN_EINVAL and n == -7 and set(out) == {-7}, name
        assert b"cn_gemm_rows_grouped_plan: job %d" % (len(jobs) - 1) in lib.cn_last_error_string(), name
        bad.a = bad.b = bad.c = 64                      # (never followed: the call refuses before its first launch)
        arr = (CnRowsJob * len(jobs))(*jobs)
        assert lib.cn_gemm_rows_grouped_k(arr, len(jobs), None) == CN_EINVAL, name
        bad.a = bad.b = bad.c = None


def test_missing_pointers_and_too_little_room():
    assert lib.cn_gemm_rows_grouped_k(None, 1, None) == CN_EINVAL and lib.cn_gemm_rows_grouped_k(None, -1, None) == CN_EINVAL
    arr = (CnRowsJob * 1)(job(8, 65, 5))                                   # NULL operands: fine for the plan, refused by the call
    assert lib.cn_gemm_rows_grouped_k(arr, 1, None) == CN_EINVAL
    assert lib.cn_gemm_rows_grouped_k(None, 0, None) == 0                  # (nothing to do)
    jobs = [job(8, 65, 5)] * 17
    for cap in (0, 8, 15):
        rc, n, out = query(jobs, cap)
        assert rc == CN_EINVAL and n == -7 and set(out) == {-7}, cap
    assert query(jobs, 16)[:2] == (0, 2)
    arr = (CnRowsJob * 17)(*jobs)
    n, out = ctypes.c_int(), (ctypes.c_int * 16)()
    assert lib.cn_gemm_rows_grouped_plan(arr, 17, None, 16, ctypes.byref(n)) == CN_EINVAL
    assert lib.cn_gemm_rows_grouped_plan(arr, 17, out, 16, None) == CN_EINVAL
    assert lib.cn_gemm_rows_grouped_plan(None, 1, out, 16, ctypes.byref(n)) == CN_EINVAL
