"""What tests/test_stream_edges_gpu.py stands on, checked without a GPU (tests/stream_cases.py):
  * cn_stream_plan (csrc/elementwise.hip: plan_stream is the function the fourteen entries decide with) is the hand-written
    transcription of the entries' former inline decisions on every row of the tables, and names the path each row claims; every path
    of every entry is claimed in every dtype the entry accepts; every capped row exceeds its cap and the row below it does not; the
    32-bit index guards of the 4-channel pools, which no small tensor reaches, are exercised through the query;
  * every exact case meets (sum of |terms|) 2^k < 2^24 and its result is representable in the storage type;
  * the integer bf16 rounding is torch's on the whole cast table; the pool model is oracle.ref_ops.maxpool and its tie rule torch's;
  * the GAN yardstick passes the GAN bound by its own structure."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as O
from tests import stream_cases as SC

REQUESTS = SC.plan_requests()


def report(op, dt, rows, row, c, h, w, k, s, pad, aligned, det):
    from confignet_amd._lib import lib
    out = (ctypes.c_longlong * 4)()
    rc = lib.cn_stream_plan(SC.OPS.index(op), dt, rows, row, c, h, w, k, s, pad, aligned, det, ctypes.byref(out))
    return rc, (list(out) if rc == 0 else None)


def test_the_plan_of_every_row_is_the_transcription_and_the_path_it_claims():
    assert len(REQUESTS) > 400
    for what, op, dt, rows, row, c, h, w, k, s, pad, mis, claim in REQUESTS:
        for det in (0, 1):
            q = (op, dt, rows, row, c, h, w, k, s, pad, SC.mask_of(op, mis), det)
            got = report(*q)
            assert got == SC.stream_plan(*q), (what, q, got)
            if claim < 0:
                assert got == (claim, None), (what, q, got)
            else:
                assert got[0] == 0 and got[1][0] == claim, (what, q, got)
                assert (got[1][3] > 0) == (det == 1 and op in ("sqdiff_sum", "row_sumsq")), (what, q, got)


def report_ptrs(op, dt, dst_dt, rows, row, c, h, w, k, s, pad, ptrs, det):
    from confignet_amd._lib import lib
    out, arr = (ctypes.c_longlong * 4)(), (ctypes.c_void_p * 4)(*ptrs)
    rc = lib.cn_stream_plan_ptrs(SC.OPS.index(op), dt, dst_dt, rows, row, c, h, w, k, s, pad, ctypes.byref(arr), det, ctypes.byref(out))
    return rc, (list(out) if rc == 0 else None)


@pytest.mark.parametrize("op", SC.OPS)
def test_the_mask_code_of_the_entries_is_each_entrys_former_alignment_term(op):
    """cn_stream_plan_ptrs takes the mask from pointers with stream_mask, the function every entry takes it with.  On every
    combination of operand addresses 0, 2, 4 and 8 bytes past a 16-byte boundary (and NULL for an optional operand) the plan is the
    transcribed plan under the alignment term the entry wrote inline (tests/stream_cases.py: entry_aligned): 8 bytes past is aligned
    for bf16 and not for fp32, the destination of a cast is judged in ITS type, NULL is aligned."""
    import itertools
    names = SC.OPERANDS[op]
    size = (1, 1024, 0, 0, 0, 0, 0, 0) if SC.OPS.index(op) < 6 else (3, 1024, 0, 0, 0, 0, 0, 0) if SC.OPS.index(op) < 10 else (3, 0, 8, 8, 8, 2, 2, 0)
    base, asked = 0x7F0000100000, 0
    for dt in SC.DTYPES[op]:
        dst_dt = 1 - dt if op == "cast" else dt
        choices = [[base + 0x1000 * i + o for o in (0, 2, 4, 8)] + ([None] if (op, nm) in SC.OPTIONAL else []) for i, nm in enumerate(names)]
        for ptrs in itertools.product(*choices):
            for det in (0, 1):
                al = SC.entry_aligned(op, dt, dst_dt, ptrs)
                want = SC.stream_plan(op, dt, *size, SC.all_aligned(op) if al else 0, det)
                got = report_ptrs(op, dt, dst_dt, *size, ptrs, det)
                assert got == want, (op, dt, [p and hex(p) for p in ptrs], det, got, want)
                asked += 1
    assert asked >= 2 * 4 ** len(names) * len(SC.DTYPES[op])
    if op == "cast":                                                       # an aligned source with a destination one element off: one per lane
        for dt in (SC.F32, SC.BF16):
            one = 4 if dt == SC.BF16 else 2                                # one element of the DESTINATION type
            assert report_ptrs(op, dt, 1 - dt, 1, 1024, 0, 0, 0, 0, 0, 0, (base, base + 0x1000 + one), 0)[1][0] == SC.SCALAR
            assert report_ptrs(op, dt, 1 - dt, 1, 1024, 0, 0, 0, 0, 0, 0, (base, base + 0x1000), 0)[1][0] == SC.VEC
    # an operand that is off makes the path of every entry the one-per-lane one (a refusal for the fused pool)
    for i in range(len(names)):
        ptrs = [base + 0x1000 * j + (2 if j == i else 0) for j in range(len(names))]
        rc, plan = report_ptrs(op, SC.F32, SC.BF16 if op == "cast" else SC.F32, *size, ptrs, 0)
        assert (rc == SC.CN_EUNSUPPORTED) if op == "maxpool2_bwd_act" else plan[0] == SC.SCALAR, (op, names[i])


def test_every_path_of_every_entry_is_claimed_in_every_dtype():
    claimed = {(op, dt, claim) for _, op, dt, *_, claim in REQUESTS if claim >= 0}
    for op in SC.OPS:
        for dt in SC.DTYPES[op]:
            for path in SC.PATHS[op]:
                assert (op, dt, path) in claimed, "no row reaches path %d of %s in dtype %d" % (path, op, dt)
    refused = {mis for *_, mis, rc in SC.POOL2_ACT if rc == SC.CN_EUNSUPPORTED and mis}
    assert refused == set(SC.OPERANDS["maxpool2_bwd_act"])                # each operand misaligned is a refusal
    # every operand of every entry is the misaligned one of some row
    seen = {(op, mis) for _, op, *_, mis, _ in REQUESTS if mis}
    for op in SC.OPS:
        for name in SC.OPERANDS[op]:
            assert (op, name) in seen, "no row misaligns %s of %s" % (name, op)


def test_every_capped_row_exceeds_its_cap_and_the_row_below_does_not():
    capped = 0
    for table in ([(e, dt, mis, path, ns) for e, _, dt, mis, path, ns in SC.FLAT], [("sqdiff_sum", dt, mis, path, ns) for dt, mis, path, ns in SC.SQDIFF]):
        for entry, dt, mis, path, numels in table:
            for i, n in enumerate(numels):
                blocks, cap = SC.uncapped_blocks(entry, n, path == SC.VEC)
                rc, plan = report(entry, dt, 1, n, 0, 0, 0, 0, 0, 0, SC.mask_of(entry, mis), 0)
                assert plan[1] == min(blocks, cap)
                if n in (SC.CAP_V, SC.CAP_S, SC.SQ_CAP_V, SC.SQ_CAP_S):
                    # more blocks' worth than the cap, and not a multiple of the grid: a second trip followed by a ragged tail
                    assert blocks > cap and plan[1] == cap and i == len(numels) - 1 and SC.uncapped_blocks(entry, numels[i - 1], path == SC.VEC)[0] <= cap
                    assert (n // (4 if path == SC.VEC else 1)) % (cap * 256) != 0 and (path != SC.VEC or n % 4)
                    capped += 1
                else:
                    assert blocks <= cap
    for entry, _, dt, mis, rows, lens in SC.ROW:
        for i, r in enumerate(lens):
            blocks, cap = SC.uncapped_blocks(entry, r, False)
            assert (blocks > cap) == (r == SC.ROW_CAP)
            capped += r == SC.ROW_CAP
            assert r != SC.ROW_CAP or (i > 0 and SC.uncapped_blocks(entry, lens[i - 1], False)[0] <= cap)
    for mis, rows, lens in SC.ROW_SUMSQ:
        for i, r in enumerate(lens):
            blocks, cap = SC.uncapped_blocks("row_sumsq", r, False)
            assert (blocks > cap) == (r == SC.SUMSQ_CAP)
            capped += r == SC.SUMSQ_CAP
            assert r != SC.SUMSQ_CAP or (i > 0 and SC.uncapped_blocks("row_sumsq", lens[i - 1], False)[0] <= cap)
    # one capped case per flat kernel and path, in both dtypes where the kernel has two instances
    flat = {(e, dt, path) for e, _, dt, _, path, ns in SC.FLAT if ns[-1] in (SC.CAP_V, SC.CAP_S)}
    for e in ("act_fwd", "act_bwd", "axpby", "mul"):
        assert {(e, dt, p) for dt in (SC.F32, SC.BF16) for p in (SC.VEC, SC.SCALAR)} <= flat, e
    assert {("cast", dt, p) for dt in (SC.F32, SC.BF16) for p in (SC.VEC, SC.SCALAR)} <= flat
    assert capped >= 30


def test_the_32_bit_index_guards_of_the_4_channel_pools():
    """maxpool_fwd4 / maxpool_bwd4 index with 32-bit integers: the forward takes them while both tensors hold fewer than 2^30 groups,
    the backward while the input holds fewer than 2^31 - 1.  No test tensor is that large; the decision is reached through the query."""
    full = 3
    n, c = 1, 4
    for hw, want in ((32767, SC.VEC), (32768, SC.SCALAR)):               # 1 x hw x 32768 x 4: (2^30 - 2^15 | 2^30) input groups
        q = ("maxpool_fwd", SC.F32, n, 0, c, hw, 32768, 1, 1, 0, full, 0)
        assert report(*q) == SC.stream_plan(*q) and report(*q)[1][0] == want
    # the output term alone: k = 1, s = 1, pad = 1 makes the output (h + 2) x (w + 2), larger than the input, which stays under 2^30
    for hw, want in ((32765, SC.VEC), (32766, SC.SCALAR)):               # output 32767 | 32768 rows of 32768 groups; input < 2^30 - 2^16
        q = ("maxpool_fwd", SC.F32, 1, 0, 4, hw, 32766, 1, 1, 1, full, 0)
        assert hw * 32766 < 2 ** 30 - 2 ** 16 and ((hw + 2) * 32768 < 2 ** 30) == (want == SC.VEC)
        assert report(*q) == SC.stream_plan(*q) and report(*q)[1][0] == want, q
    q = ("maxpool_fwd", SC.BF16, 2, 0, 8, 16384, 16383, 3, 2, 1, full, 0)   # 2^29 - 2^15 groups each way... under
    assert report(*q) == SC.stream_plan(*q) and report(*q)[1][0] == SC.VEC
    q = ("maxpool_fwd", SC.BF16, 4, 0, 8, 16384, 16384, 3, 2, 1, full, 0)   # 2^31 input groups
    assert report(*q) == SC.stream_plan(*q) and report(*q)[1][0] == SC.SCALAR
    for total4, want in ((2 ** 31 - 2, SC.VEC), (2 ** 31 - 1, SC.SCALAR), (2 ** 31, SC.SCALAR)):
        h, w = {2 ** 31 - 2: (2, 2 ** 30 - 1), 2 ** 31 - 1: (1, 2 ** 31 - 1), 2 ** 31: (2, 2 ** 30)}[total4]
        q = ("maxpool_bwd", SC.F32, 1, 0, 4, h, w, 3, 2, 1, 7, 0)
        assert h * w == total4 and report(*q) == SC.stream_plan(*q) and report(*q)[1][0] == want, total4
    q = ("maxpool_bwd", SC.F32, 1, 0, 4, 2, 2 ** 30, 2, 2, 0, 7, 0)       # the 2 x 2 kernel indexes with 64 bits: no guard
    assert report(*q) == SC.stream_plan(*q) and report(*q)[1][:2] == [SC.POOL2, 8192]


def test_the_plan_around_every_boundary_and_bad_requests():
    for op in SC.OPS[:10]:
        for dt in SC.DTYPES[op]:
            for row in (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 8192 * 256 - 1, 8192 * 256, 8192 * 256 + 1,
                        8192 * 1024, 8192 * 1024 + 1, 512 * 256 * 4 - 1, 512 * 256 * 4, 512 * 4096, 512 * 4096 + 1, 64 * 8192, 64 * 8192 + 1):
                for al in range(SC.all_aligned(op) + 1):
                    for rows in (1, 3):
                        q = (op, dt, rows, row, 0, 0, 0, 0, 0, 0, al, al & 1)
                        assert report(*q) == SC.stream_plan(*q), q
    for op in SC.OPS[10:]:
        for c, h, w, k, s, pad in ((4, 8, 8, 2, 2, 0), (4, 7, 8, 2, 2, 0), (6, 8, 8, 2, 2, 0), (8, 9, 5, 3, 2, 1), (3, 9, 5, 3, 1, 1), (4, 2, 2, 3, 2, 0)):
            for al in range(SC.all_aligned(op) + 1):
                q = (op, SC.BF16, 3, 0, c, h, w, k, s, pad, al, 0)
                assert report(*q) == SC.stream_plan(*q), q
    from confignet_amd._lib import lib
    out = (ctypes.c_longlong * 4)()
    for bad in ((-1, 0, 1, 4), (14, 0, 1, 4), (0, 2, 1, 4), (0, 0, 0, 4), (0, 0, 1, 0), (6, 1, 1, 4)):
        assert lib.cn_stream_plan(bad[0], bad[1], bad[2], bad[3], 0, 0, 0, 0, 0, 0, 3, 0, ctypes.byref(out)) == SC.CN_EINVAL, bad
    assert lib.cn_stream_plan(10, 0, 1, 0, 4, 0, 8, 2, 2, 0, 3, 0, ctypes.byref(out)) == SC.CN_EINVAL
    assert lib.cn_stream_plan(0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 3, 0, None) == SC.CN_EINVAL


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
def _holds(terms, want, dt, what):
    margin = SC.exact_margin(terms)
    assert 0 <= margin < 2 ** 24, "%s: (sum |terms|) 2^k = %g" % (what, margin)
    assert np.array_equal(SC.storage_round(want, dt), want), what + ": the result is not representable in the storage type"


@pytest.mark.parametrize("row", SC.FLAT, ids=lambda r: "%s-%s-%d-%s" % r[:4])
def test_every_flat_case_is_exact(row):
    entry, variant, dt, mis, path, numels = row
    for n in numels:
        ops, _, want, terms = SC.flat_case(entry, variant, dt, n)
        _holds(terms, want, SC.BF16 if entry == "cast" else dt, "%s numel %d" % (entry, n))
        for a in ops:
            assert a is None or np.array_equal(SC.storage_round(a, dt), a)
    if variant == SC.TANH and entry == "act_fwd":                      # 0 and +-1 only, each present; fp32 tanh of the arguments is exact
        assert set(np.unique(want)) <= {-1.0, 0.0, 1.0} and float(np.tanh(16.0)) > 1 - 2.0 ** -30


@pytest.mark.parametrize("row", SC.ROW, ids=lambda r: "%s-%s-%d-%s-%d" % r[:5])
def test_every_row_map_case_is_exact(row):
    entry, variant, dt, mis, rows, lens = row
    for r in lens:
        ops, scal, want, terms = SC.row_case(entry, variant, dt, rows, r)
        _holds(terms, want, dt, "%s row %d" % (entry, r))
        assert len(set(scal[0].tolist())) == rows                      # the scales differ per row
        for a in ops:
            assert a is None or np.array_equal(SC.storage_round(a, dt), a)
        f32 = np.float32(scal[0]) * np.float32(scal[1])                # s[row] k, which the kernels form in fp32, is exact
        assert np.array_equal(f32.astype(np.float64), scal[0] * scal[1])


def test_every_reduction_case_is_exact():
    for dt, mis, path, numels in SC.SQDIFF:
        for n in numels:
            (a, b), want, terms = SC.sqdiff_case(dt, n)
            _holds(terms, np.asarray(want), SC.F32, "sqdiff_sum numel %d" % n)
            assert np.array_equal(SC.storage_round(a, dt), a) and np.array_equal(SC.storage_round(b, dt), b) and want > SC.SQ_PRESET
    for mis, rows, lens in SC.ROW_SUMSQ:
        for r in lens:
            x, want, terms = SC.sumsq_case(rows, r)
            _holds(terms, want, SC.F32, "row_sumsq row %d" % r)
            assert (want > 0).all() and (rows == 1 or len(set(want.tolist())) > 1 or r < 8)


def test_every_pool_case_is_exact_and_reaches_its_edge():
    seen = set()
    for row in SC.MAXPOOL:
        n, h, w, c, k, s, pad, dt, mis, kind = row[:10]
        x, gy, y, gx = SC.maxpool_case(row)
        what = "maxpool %s" % (row,)
        _holds([y], y, dt, what)
        _holds([9 * np.abs(gy).max()], gx, dt, what)                   # at most nine windows per element
        assert np.array_equal(SC.storage_round(x, dt), x) and np.array_equal(SC.storage_round(gy, dt), gy)
        assert float(gx.sum()) <= float(gy.sum()) + 1e-9 or kind != SC.TIES or pad           # (nothing is counted twice)
        if pad and kind in (SC.MIXED, SC.NEG):                         # padding wins somewhere: a zero output that is no input value, no gradient
            assert (y[:, 0] == 0).any() and abs(float(gx.sum()) - float(gy.sum())) > 0
        if kind == SC.NEG and pad == 0:
            assert (y < 0).all()
        if (h + 2 * pad - k) % s or (w + 2 * pad - k) % s:             # a row or column of the padded input is in no window
            seen.add("leftover")
            if pad == 0:
                edge = gx[:, -1] if (h - k) % s else gx[:, :, -1]
                assert not edge.any()
        if k > s and float(np.abs(gx).max()) > float(np.abs(gy).max()):
            seen.add("collects")                                       # one element collects from several windows
        if SC.pool_out(h, k, s, pad) == 1:
            seen.add("oh1")
        seen.add((kind, row[11]))
    assert {"leftover", "collects", "oh1"} <= seen
    for path in (SC.SCALAR, SC.VEC, SC.POOL2):                           # ties on all three backward kernels
        assert (SC.TIES, path) in seen
    for row in SC.POOL2_ACT:
        x, gy, t, s, want = SC.pool2_act_case(row)
        if want is not None:
            _holds([want], want, row[4], "maxpool2_bwd_act %s" % (row,))
            assert (x == 0).any() and (x > 0).any()
    counts = set()
    for row in SC.AVGPOOL:
        mean, tot, cnt = SC.avgpool3_same(SC.avgpool_case(row))
        counts |= set(cnt.reshape(-1).astype(int).tolist())
        assert SC.exact_margin([9 * np.abs(SC.avgpool_case(row)).max()]) < 2 ** 24
    assert counts == SC.AVG_COUNTS
    # one correct rounding to bf16 is half a bf16 ulp of the binade: up to 2^-8 of the value.  torch's own rounding of 7/3 is further
    # than 2^-9 of it away and inside avgpool_bound, which is tight there
    v = np.asarray([7.0 / 3.0, 1.0, 255.0 / 9.0, 0.0, -1.0 / 3.0])
    err = np.abs(torch.from_numpy(v).to(torch.bfloat16).double().numpy() - v)
    assert err[0] > 2.0 ** -9 * v[0] and (err <= SC.avgpool_bound(v, SC.BF16)).all() and SC.avgpool_bound(v, SC.BF16)[0] < 2.0 ** -8 * v[0]
    assert (SC.avgpool_bound(v, SC.F32) == 3 * 2.0 ** -24 * np.abs(v)).all()


def test_the_small_maps_are_exact():
    for c, has_b, pixels in SC.MASKED_DIFF:
        a, b, m, want = SC.masked_diff_case(c, has_b, pixels)
        _holds([want], want, SC.F32, "masked_diff")
    x = SC.ints((257, 3), -8, 8, 5)
    for perm in SC.PERMS:
        y = SC.chan_affine3_fwd(x, perm, SC.AFFINE_SCALE, SC.AFFINE_OFF)
        _holds([SC.AFFINE_SCALE * x, y], y, SC.F32, "chan_affine3")
        # the backward is the transpose: <A x, g> == <x, A^T g>, and for a permutation that is no involution it differs from A's own direction
        g = SC.ints((257, 3), -8, 8, 6)
        assert float(((y - np.asarray(SC.AFFINE_OFF)) * g).sum()) == float((x * SC.chan_affine3_bwd(g, perm, SC.AFFINE_SCALE)).sum())
    wrong = [p for p in SC.PERMS if not np.array_equal(SC.chan_affine3_bwd(x, p, 1.0), x[:, list(p)])]
    assert sorted(wrong) == [(1, 2, 0), (2, 0, 1)]


# ---- the bf16 rounding ---------------------------------------------------------------------------------------------------------------
def test_the_integer_rounding_is_torch_on_the_whole_cast_table():
    u = SC.cast_table()
    assert u.shape == (327680,) and len(np.unique(u)) == 327680
    mine = SC.bf16_bits(u)
    theirs = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = SC.is_nan32(u)
    assert np.array_equal(mine[~nan], theirs[~nan])
    assert SC.is_nan16(mine[nan]).all() and SC.is_nan16(theirs[nan]).all() and np.array_equal(mine[nan] >> 15, (u[nan] >> 31).astype(np.uint16))
    # what the table holds: ties on even and odd mantissas, the carry into the exponent, overflow to infinity, subnormals, zeros
    at = lambda b, low: int(mine[5 * b + SC.LOW_HALVES.index(low)])
    assert at(0x3F80, 0x8000) == 0x3F80 and at(0x3F81, 0x8000) == 0x3F82               # tie to even: down, up
    assert at(0x3F80, 0x7FFF) == 0x3F80 and at(0x3F80, 0x8001) == 0x3F81
    assert at(0x3FFF, 0x8000) == 0x4000 and at(0x7F7F, 0x8000) == 0x7F80 and at(0xFF7F, 0xFFFF) == 0xFF80   # carry; overflow to +-inf
    assert at(0x0000, 0x8000) == 0x0000 and at(0x0001, 0x8000) == 0x0002 and at(0x8000, 0x0000) == 0x8000   # subnormals; -0
    assert at(0x7F80, 0x0000) == 0x7F80 and SC.is_nan16(np.asarray([at(0x7F80, 0x8001)], np.uint16))[0]     # inf stays; a NaN whose payload is low
    assert np.array_equal(SC.bf16_round(np.asarray([1.0, 1.00390625, -3.5])), np.asarray([1.0, 1.0, -3.5]))


# ---- the pool model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.MAXPOOL, ids=lambda r: "x".join(map(str, r[:7])) + "-" + r[9])
def test_the_pool_model_is_the_oracle_and_its_tie_rule_is_torch(row):
    n, h, w, c, k, s, pad = row[:7]
    x, gy, y, gx = SC.maxpool_case(row)
    xt = torch.from_numpy(x).requires_grad_(True)
    yo = O.maxpool(xt, k, s, pad)
    assert torch.equal(yo.detach(), torch.from_numpy(y))
    # torch's own rule on the zero-padded tensor (first maximum in row-major window order) routes every gradient where the model does
    xp = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), [pad] * 4).requires_grad_(True)
    out, idx = F.max_pool2d(xp, k, s, return_indices=True)
    out.backward(torch.from_numpy(gy).permute(0, 3, 1, 2))
    want = xp.grad[:, :, pad:pad + h, pad:pad + w].permute(0, 2, 3, 1)
    assert torch.equal(want, torch.from_numpy(gx)), row
    if row[9] == SC.TIES:
        assert len(torch.unique(out)) <= 3 and float(x.max()) == 2        # ties are everywhere


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def test_the_yardstick_passes_the_gan_bound():
    for n in SC.GAN_N:
        for label in SC.GAN_LABELS:
            s = SC.gan_scores(n, n)
            assert n < 6 or all(v in s.tolist() for v in SC.GAN_SPECIAL)
            ref, bound, yard = SC.gan_fwd_bound(s, label)
            assert yard <= bound and bound <= max(SC.GAN_FACTOR * yard, n * 2.0 ** -23 * ref) and ref > 0
            gref, gbound, gyard = SC.gan_bwd_bound(s, -1.5, label)
            assert (gyard <= gbound).all() and (gbound <= 1e-6 * np.abs(gref) + 1e-44).all() and (np.sign(gref) == (1 if label else -1)).all()
    # softplus and sigmoid in float64 where fp32 saturates
    assert SC.softplus(np.asarray([-100.0]))[0] == np.exp(-100.0) and SC.softplus(np.asarray([100.0]))[0] == 100.0
    assert SC.sigmoid(np.asarray([-100.0]))[0] > 0 and SC.sigmoid(np.asarray([0.0]))[0] == 0.5


def test_the_adam_bounds_hold_a_plain_fp32_step():
    """the whole step in NumPy float32, one rounding per operation in the order of the kernel's expressions, is inside every bound"""
    f = np.float32
    for n in (257, 4001):
        for b1, b2 in SC.ADAM_BETAS:
            th, g, m, v, ema = SC.adam_state(n, 3)
            assert v[0] == 0 and g[0] == 0 and v[1] == 0 and 0 < abs(g[1]) < SC.ADAM_EPS * 1e-3 and (m > 0).any() and (m < 0).any()
            lr, eps, al = f(SC.ADAM_LR), f(SC.ADAM_EPS), f(SC.EMA_ALPHA)
            m32 = f(b1) * m + (f(1) - f(b1)) * g
            v32 = f(b2) * v + (f(1) - f(b2)) * g * g
            th32 = th - lr * m32 / (np.sqrt(v32) + eps)
            e32 = al * ema + (f(1) - al) * th32
            assert all(a.dtype == np.float32 for a in (m32, v32, th32, e32))
            bounds = SC.adam_bounds(th, g, m, v, ema, SC.ADAM_LR, b1, b2, SC.ADAM_EPS, SC.EMA_ALPHA)
            for key, got in (("m", m32), ("v", v32), ("theta", th32), ("ema", e32)):
                ref, bound = bounds[key]
                err = np.abs(got.astype(np.float64) - ref)
                assert np.isfinite(ref).all() and (bound >= 0).all() and (err <= bound).all(), (key, b1, b2, float((err - bound).max()))
            ref, bound = SC.ema_bound(ema, th, SC.EMA_ALPHA)
            assert (np.abs((al * ema + (f(1) - al) * th).astype(np.float64) - ref) <= bound).all()
            assert set(SC.adam_bounds(th, g, m, v, None, SC.ADAM_LR, b1, b2, SC.ADAM_EPS, SC.EMA_ALPHA)) == {"theta", "m", "v"}
