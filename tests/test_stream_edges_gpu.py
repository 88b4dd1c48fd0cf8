"""The streaming maps, row maps, loss reductions, pools, GAN losses and the Adam / EMA step of csrc/elementwise.hip on every launch
path, called through `lib` at the smallest shapes that reach each edge (tests/stream_cases.py: the tables and what each row reaches).

Every operand lives in a guarded allocation (tests/chan_slices_cases.py: GuardedBuf): outputs hold NaN (accumulators their preset) before the call; after it the
sentinels around every operand are intact, the inputs unchanged and the result is the float64 model element for element -- no
tolerance: tests/test_stream_cases_cpu.py holds (sum of |terms|) 2^k < 2^24 on every exact case.  A misaligned operand is a view one
element into its allocation: the supported scalar fallback of the entry.  Before each launch cn_stream_plan, asked with the alignment
of the pointers the call gets (cn_stream_plan_ptrs: the entries' own mask code), must name the path the row claims, and after the
launch cn_stream_last_plan, which the entry writes, must hold that very plan.

Three families cannot be exact and are held at derived bounds (tests/stream_cases.py: avgpool_bound, adam_bounds, gan_fwd_bound /
gan_bwd_bound): measured error and bound per case go to profiles/stream_edges_errors.txt when STREAM_EDGE_ERRORS names a path."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import stream_cases as SC
from tests.chan_slices_cases import GuardedBuf as Buf

pytestmark = pytest.mark.gpu

TORCH_DT = {SC.F32: torch.float32, SC.BF16: torch.bfloat16}
DT_NAME = {SC.F32: "f32", SC.BF16: "bf16"}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(a):
    return a.ptr if isinstance(a, Buf) else a


def _call(name, *args):
    from confignet_amd._lib import lib
    return getattr(lib, "cn_" + name)(*[_ptr(a) for a in args], _stream())


def _plan(op, dt, rows, row, operands, det=0, geom=(0, 0, 0, 0, 0, 0), dst_dt=None):
    """what cn_stream_plan_ptrs -- the mask code of the entries on the pointers this call gets -- plans"""
    from confignet_amd._lib import lib
    out, ptrs = (ctypes.c_longlong * 4)(), (ctypes.c_void_p * 4)(*[_ptr(a) for a in operands])
    rc = lib.cn_stream_plan_ptrs(SC.OPS.index(op), dt, dt if dst_dt is None else dst_dt, rows, row, *geom, ctypes.byref(ptrs), det, ctypes.byref(out))
    return rc, list(out)


def _decided(op, plan, what):
    """the call just made decided what the query planned: cn_stream_last_plan is written by the entry itself"""
    from confignet_amd._lib import lib
    out = (ctypes.c_longlong * 5)()
    assert lib.cn_stream_last_plan(ctypes.byref(out)) == 0
    assert list(out) == [SC.OPS.index(op)] + plan, "%s: the entry decided %s, the query %s" % (what, list(out), plan)


def _in(a, dt, mis):
    return None if a is None else Buf(a.size, TORCH_DT[dt], 1 if mis else 0, data=a)


class _Mode:
    """deterministic mode for the block, the former mode after it"""

    def __init__(self, det):
        self.det = bool(det)

    def __enter__(self):
        from confignet_amd import ops
        self.was = ops.DETERMINISTIC
        ops.set_deterministic(self.det)

    def __exit__(self, *exc):
        from confignet_amd import ops
        ops.set_deterministic(self.was)


def _all_unchanged(bufs, what):
    for i, b in enumerate(bufs):
        assert b is None or b.unchanged(), "%s: input %d was written" % (what, i)


# ---- flat maps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.FLAT, ids=lambda r: "%s-%s-%s-%s" % (r[0], r[1], DT_NAME[r[2]], r[3]))
def test_flat_maps(row):
    entry, variant, dt, mis, path, numels = row
    names = SC.OPERANDS[entry]
    for n in numels:
        what = "%s %s %s numel %d, %s off a vector boundary" % (entry, variant, DT_NAME[dt], n, mis)
        ops, scal, want, _ = SC.flat_case(entry, variant, dt, n)
        out_dt = dt if entry != "cast" else 1 - dt
        ins = [_in(a, dt, names[i] == mis) for i, a in enumerate(ops)]
        if variant == "inplace":
            out = ins[0]
        else:
            out = Buf(n, TORCH_DT[out_dt], 1 if names[-1] == mis else 0)
        operands = ins + [out]
        rc, plan = _plan(entry, dt, 1, n, operands, dst_dt=out_dt)
        assert rc == 0 and plan[0] == path, what + ": plan %s" % plan
        if entry == "cast":
            rc = _call("cast", ins[0], dt, out, out_dt, n)
        elif entry == "mul":
            rc = _call("mul", *operands, n, dt)
        else:
            rc = _call(entry, *operands, n, *scal, dt)
        assert rc == 0, what
        _decided(entry, plan, what)
        out.check(want, what)
        if variant != "inplace":
            _all_unchanged(ins, what)


# ---- the cast table: every bf16 pattern x five low halves, both store forms, both directions ------------------------------------------
@pytest.mark.parametrize("mis", [None, "src", "dst"])
def test_cast_table_to_bf16(mis):
    u = SC.cast_table()
    want = SC.bf16_bits(u)
    src = Buf(len(u), torch.float32, 1 if mis == "src" else 0, data=np.zeros(1))
    src.t.view(torch.int32).copy_(torch.from_numpy(u.view(np.int32)))
    src.before = src.buf.clone()
    dst = Buf(len(u), torch.bfloat16, 1 if mis == "dst" else 0)
    rc, plan = _plan("cast", SC.F32, 1, len(u), [src, dst], dst_dt=SC.BF16)
    assert rc == 0 and plan[0] == (SC.VEC if mis is None else SC.SCALAR)      # st4 / pack_bf16x2 | stf
    assert _call("cast", src, SC.F32, dst, SC.BF16, len(u)) == 0
    _decided("cast", plan, "cast table to bf16, %s misaligned" % mis)
    assert dst.intact() and src.unchanged()
    got = dst.t.view(torch.int16).cpu().numpy().view(np.uint16)
    nan = SC.is_nan32(u)
    bad = np.flatnonzero(got[~nan] != want[~nan])
    assert not len(bad), "fp32 %#010x -> bf16 %#06x, want %#06x (%d wrong)" % (u[~nan][bad[0]], got[~nan][bad[0]], want[~nan][bad[0]], len(bad))
    assert SC.is_nan16(got[nan]).all() and np.array_equal(got[nan] >> 15, (u[nan] >> 31).astype(np.uint16)), "a NaN did not stay a NaN of its sign"
    assert np.array_equal(got[nan], want[nan])                               # (and the kernel's quiet bit is the model's)


@pytest.mark.parametrize("mis", [None, "src", "dst"])
def test_cast_table_to_f32(mis):
    b = np.arange(65536, dtype=np.uint16)
    src = Buf(len(b), torch.bfloat16, 1 if mis == "src" else 0, data=np.zeros(1))
    src.t.view(torch.int16).copy_(torch.from_numpy(b.view(np.int16)))
    src.before = src.buf.clone()
    dst = Buf(len(b), torch.float32, 1 if mis == "dst" else 0)
    rc, plan = _plan("cast", SC.BF16, 1, len(b), [src, dst], dst_dt=SC.F32)
    assert rc == 0 and plan[0] == (SC.VEC if mis is None else SC.SCALAR)
    assert _call("cast", src, SC.BF16, dst, SC.F32, len(b)) == 0
    _decided("cast", plan, "cast table to f32, %s misaligned" % mis)
    assert dst.intact() and src.unchanged()
    got = dst.t.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, b.astype(np.uint32) << np.uint32(16))         # every pattern, NaN payloads included, bit for bit


# ---- row maps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.ROW, ids=lambda r: "%s-%s-%s-%s-%d" % (r[0], r[1], DT_NAME[r[2]], r[3], r[4]))
def test_row_maps(row):
    entry, variant, dt, mis, rows, lens = row
    names = SC.OPERANDS[entry]
    for r in lens:
        what = "%s %s %s %d x %d, %s off a vector boundary" % (entry, variant, DT_NAME[dt], rows, r, mis)
        ops, scal, want, _ = SC.row_case(entry, variant, dt, rows, r)
        if entry == "row_scale":
            ops = ops[:1]
        ins = [_in(a, dt, names[i] == mis) for i, a in enumerate(ops)]
        s = Buf(rows, data=scal[0])
        out = Buf(rows * r, TORCH_DT[dt], 1 if mis == "out" else 0)
        rc, plan = _plan(entry, dt, rows, r, ins + [out])
        assert rc == 0 and plan[0] == (SC.VEC if mis is None and r % 4 == 0 else SC.SCALAR) and plan[2] == rows, what + ": plan %s" % plan
        assert (plan[1] == 512) == (r == SC.ROW_CAP)
        if entry == "tap_bwd":
            rc = _call("tap_bwd", *ins, s, out, rows, r, scal[1], scal[2], scal[3], dt)
        else:
            rc = _call(entry, *ins, s, out, rows, r, scal[1], dt)
        assert rc == 0, what
        _decided(entry, plan, what)
        out.check(want, what)
        _all_unchanged(ins + [s], what)


# ---- reductions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("row", SC.SQDIFF, ids=lambda r: "%s-%s" % (DT_NAME[r[0]], r[1]))
def test_sqdiff_sum_accumulates(row, det):
    dt, mis, path, numels = row
    with _Mode(det):
        for n in numels:
            what = "sqdiff_sum %s numel %d det %d, %s off a vector boundary" % (DT_NAME[dt], n, det, mis)
            (a, b), want, _ = SC.sqdiff_case(dt, n)
            ins = [_in(a, dt, mis == "a"), _in(b, dt, mis == "b")]
            out = Buf(1, data=np.asarray([SC.SQ_PRESET]))
            rc, plan = _plan("sqdiff_sum", dt, 1, n, ins, det)
            assert rc == 0 and plan[0] == path and plan[3] == (plan[1] if det else 0), what + ": plan %s" % plan
            assert (plan[1] == 512) == (n in (SC.SQ_CAP_V, SC.SQ_CAP_S))
            assert _call("sqdiff_sum", *ins, out, n, SC.SQ_SCALE, dt) == 0, what
            _decided("sqdiff_sum", plan, what)
            out.check([want], what)
            _all_unchanged(ins, what)
            assert _call("sqdiff_sum", *ins, out, n, SC.SQ_SCALE, dt) == 0     # and once more into the same accumulator
            out.check([2 * want - SC.SQ_PRESET], what + ", second call")


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("row", SC.ROW_SUMSQ, ids=lambda r: "%s-%d" % r[:2])
def test_row_sumsq_overwrites(row, det):
    mis, rows, lens = row
    with _Mode(det):
        for r in lens:
            what = "row_sumsq %d x %d det %d, %s off a vector boundary" % (rows, r, det, mis)
            x, want, _ = SC.sumsq_case(rows, r)
            xin = _in(x, SC.F32, mis == "x")
            out = Buf(rows)                                                    # NaN before: the sum replaces it
            rc, plan = _plan("row_sumsq", SC.F32, rows, r, [xin], det)
            assert rc == 0 and plan[0] == (SC.VEC if mis is None and r % 4 == 0 else SC.SCALAR) and plan[3] == (plan[1] * rows if det else 0), what
            assert (plan[1] == 64) == (r == SC.SUMSQ_CAP)
            assert _call("row_sumsq", xin, out, rows, r) == 0, what
            _decided("row_sumsq", plan, what)
            out.check(want, what)
            _all_unchanged([xin], what)


@pytest.mark.parametrize("case", SC.MASKED_DIFF, ids=lambda c: "c%d-b%d-p%d" % c)
def test_masked_diff(case):
    c, has_b, pixels = case
    a, b, m, want = SC.masked_diff_case(c, has_b, pixels)
    ins = [_in(a, SC.F32, False), _in(b, SC.F32, False), Buf(pixels, torch.uint8, data=m)]
    out = Buf(pixels * c)
    assert _call("masked_diff", *ins, out, pixels, c) == 0
    out.check(want, "masked_diff %s" % (case,))
    _all_unchanged(ins, "masked_diff")


# ---- pools -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.MAXPOOL, ids=lambda r: "x".join(map(str, r[:7])) + "-%s-%s-%s" % (DT_NAME[r[7]], r[8], r[9]))
def test_maxpool_forward_and_backward(row):
    n, h, w, c, k, s, pad, dt, mis, kind, fpath, bpath = row
    x, gy, y, gx = SC.maxpool_case(row)
    geom = (c, h, w, k, s, pad)
    what = "maxpool %s" % (row,)
    fmis = SC.FWD_MIS.get(mis)
    xin, yout = _in(x, dt, fmis == "x"), Buf(y.size, TORCH_DT[dt], 1 if fmis == "y" else 0)
    rc, plan = _plan("maxpool_fwd", dt, n, 0, [xin, yout], geom=geom)
    assert rc == 0 and plan[0] == fpath, what + ": forward plan %s" % plan
    assert _call("maxpool_fwd", xin, yout, n, h, w, c, k, s, pad, dt) == 0
    _decided("maxpool_fwd", plan, what)
    yout.check(y, what + " forward")
    _all_unchanged([xin], what)
    ins = [_in(x, dt, mis == "x"), _in(gy, dt, mis == "gy")]
    gout = Buf(x.size, TORCH_DT[dt], 1 if mis == "gx" else 0)
    rc, plan = _plan("maxpool_bwd", dt, n, 0, ins + [gout], geom=geom)
    assert rc == 0 and plan[0] == bpath, what + ": backward plan %s" % plan
    assert _call("maxpool_bwd", *ins, gout, n, h, w, c, k, s, pad, dt) == 0
    _decided("maxpool_bwd", plan, what)
    gout.check(gx, what + " backward")
    _all_unchanged(ins, what)


@pytest.mark.parametrize("row", SC.POOL2_ACT, ids=lambda r: "x".join(map(str, r[:4])) + "-%s-t%d-s%d-%s" % (DT_NAME[r[4]], r[5], r[6], r[7]))
def test_maxpool2_bwd_act(row):
    n, h, w, c, dt, has_t, s_rows, mis, want_rc = row
    x, gy, t, s, want = SC.pool2_act_case(row)
    what = "maxpool2_bwd_act %s" % (row,)
    ins = [_in(x, dt, mis == "x"), _in(gy, dt, mis == "gy"), _in(t, dt, mis == "target")]
    sb = None if s is None else Buf(len(s), data=s)
    out = Buf(x.size, TORCH_DT[dt], 1 if mis == "gx" else 0)
    rc, plan = _plan("maxpool2_bwd_act", dt, n, 0, ins + [out], geom=(c, h, w, 2, 2, 0))
    assert rc == want_rc and (rc or plan[0] == SC.POOL2), what
    assert _call("maxpool2_bwd_act", ins[0], ins[1], ins[2], sb, SC.ROW_K if has_t else 0.0, out, n, h, w, c, s_rows, dt) == want_rc, what
    if want_rc == SC.CN_OK:
        _decided("maxpool2_bwd_act", plan, what)
        out.check(want, what)
    else:
        from confignet_amd._lib import lib
        last = (ctypes.c_longlong * 5)()
        assert lib.cn_stream_last_plan(ctypes.byref(last)) == 0 and last[0] == -1, what + ": the entry did not record its refusal"
        assert out.unchanged(), what + ": a refusal wrote the output"
    _all_unchanged(ins + [sb], what)
    if has_t:                                                              # a target without its scales is an argument error
        assert _call("maxpool2_bwd_act", ins[0], ins[1], ins[2], None, SC.ROW_K, out, n, h, w, c, s_rows, dt) == SC.CN_EINVAL
        assert _call("maxpool2_bwd_act", ins[0], ins[1], ins[2], sb, SC.ROW_K, out, n, h, w, c, n + 1, dt) == SC.CN_EINVAL
        assert want_rc != SC.CN_OK or (out.intact() and np.array_equal(out.values(), want.reshape(-1)))


@pytest.mark.parametrize("row", SC.AVGPOOL, ids=lambda r: "x".join(map(str, r[:4])) + "-%s-%s" % (DT_NAME[r[4]], r[5]))
def test_avgpool3_same(row):
    n, h, w, c, dt, mis, path = row
    x = SC.avgpool_case(row)
    mean, tot, cnt = SC.avgpool3_same(x)
    xin, out = _in(x, dt, mis == "x"), Buf(x.size, TORCH_DT[dt], 1 if mis == "y" else 0)
    rc, plan = _plan("avgpool3_same", dt, n, 0, [xin, out], geom=(c, h, w, 3, 1, 1))
    assert rc == 0 and plan[0] == path, "%s: plan %s" % (row, plan)
    assert _call("avgpool3_same", xin, out, n, h, w, c, dt) == 0
    _decided("avgpool3_same", plan, "avgpool3_same %s" % (row,))
    assert out.intact() and xin.unchanged()
    err, bound = np.abs(out.values() - mean.reshape(-1)), SC.avgpool_bound(mean, dt).reshape(-1)
    _note("avgpool3_same", "x".join(map(str, row[:4])) + " " + DT_NAME[dt] + (" scalar" if path == SC.SCALAR else ""), "mean", err, bound)
    bad = np.flatnonzero(~(err <= bound))
    assert not len(bad), "avgpool3_same %s: element %d off by %.3e, bound %.3e" % (row, bad[0], err[bad[0]], bound[bad[0]])


@pytest.mark.parametrize("pixels", SC.AFFINE_PIXELS)
@pytest.mark.parametrize("perm", SC.PERMS, ids=lambda p: "".join(map(str, p)))
def test_chan_affine3_and_its_transpose(perm, pixels):
    x, g = SC.ints((pixels, 3), -8, 8, pixels), SC.ints((pixels, 3), -8, 8, pixels + 1)
    p, off = (ctypes.c_int * 3)(*perm), (ctypes.c_float * 3)(*SC.AFFINE_OFF)
    xin, gin, y, gx = _in(x, SC.F32, False), _in(g, SC.F32, False), Buf(pixels * 3), Buf(pixels * 3)
    assert _call("chan_affine3_fwd", xin, y, pixels, p, SC.AFFINE_SCALE, off) == 0
    y.check(SC.chan_affine3_fwd(x, perm, SC.AFFINE_SCALE, SC.AFFINE_OFF), "chan_affine3_fwd %s" % (perm,))
    assert _call("chan_affine3_bwd", gin, gx, pixels, p, SC.AFFINE_SCALE) == 0
    gx.check(SC.chan_affine3_bwd(g, perm, SC.AFFINE_SCALE), "chan_affine3_bwd %s" % (perm,))
    _all_unchanged([xin, gin], "chan_affine3")


# ---- the families that cannot be exact -------------------------------------------------------------------------------------------------
_ERRORS = {}               # (entry, case, quantity) -> (largest error / bound, largest error, its bound, the yardstick's error there or None)


def _note(entry, case, quantity, err, bound, yard=None):
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    rec = (float(ratio[i]), float(err[i]), float(bound[i]), None if yard is None else float(np.atleast_1d(yard)[i]))
    if rec[0] >= _ERRORS.get((entry, case, quantity), (-1.0,))[0]:
        _ERRORS[(entry, case, quantity)] = rec
    print("%s %s %s: error %.3e, bound %.3e" % (entry, case, quantity, rec[1], rec[2]))
    path = os.environ.get("STREAM_EDGE_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("The three families of tests/test_stream_edges_gpu.py that cannot be exact, one MI355X (written when STREAM_EDGE_ERRORS names a\n"
                    "path).  error = |got - float64 model| at the element where error / bound is largest; bound as tests/stream_cases.py derives\n"
                    "it (avgpool_bound: 3 x 2^-24 relative, + half a bf16 ulp in bf16; adam_bounds / ema_bound: counted roundings per quantity; gan_*_bound:\n"
                    "max(4 x the torch-float32 yardstick's own error, the floor)); yardstick = the yardstick's error at that element (GAN only).\n\n")
            f.write("%-18s %-34s %-10s %10s %10s %8s %10s\n" % ("entry", "case", "quantity", "error", "bound", "ratio", "yardstick"))
            for (e, c, q), (ratio_, err_, bound_, yard_) in sorted(_ERRORS.items()):
                f.write("%-18s %-34s %-10s %10.3e %10.3e %8.3f %10s\n" % (e, c, q, err_, bound_, ratio_, "-" if yard_ is None else "%.3e" % yard_))


@pytest.mark.parametrize("label", SC.GAN_LABELS)
@pytest.mark.parametrize("n", SC.GAN_N)
def test_gan_loss(n, label):
    s = SC.gan_scores(n, n)
    sin = Buf(n, data=s)
    out, gs, gout = Buf(1), Buf(n), Buf(1, data=np.asarray([-1.5]))
    assert _call("gan_loss_fwd", sin, out, n, label) == 0
    assert _call("gan_loss_bwd", sin, gout, gs, n, label) == 0
    assert out.intact() and gs.intact() and sin.unchanged() and gout.unchanged()
    ref, bound, yard = SC.gan_fwd_bound(s, label)
    err = abs(float(out.values()[0]) - ref)
    _note("gan_loss_fwd", "n %d label %d" % (n, label), "loss", err, bound, yard)
    gref, gbound, gyard = SC.gan_bwd_bound(s, -1.5, label)
    gerr = np.abs(gs.values() - gref)
    _note("gan_loss_bwd", "n %d label %d" % (n, label), "gradient", gerr, gbound, gyard)
    assert err <= bound, "gan_loss_fwd n %d label %d: error %.3e, bound %.3e (yardstick %.3e)" % (n, label, err, bound, yard)
    bad = np.flatnonzero(~(gerr <= gbound))
    assert not len(bad), "gan_loss_bwd n %d label %d: score %r off by %.3e, bound %.3e (yardstick %.3e)" % (n, label, s[bad[0]], gerr[bad[0]], gbound[bad[0]], gyard[bad[0]])


@pytest.mark.parametrize("njobs", SC.GAN_GROUPS)
def test_gan_loss_grouped_is_the_single_head_entries(njobs):
    from confignet_amd._lib import CnGanJob
    ns = [SC.GAN_N[(j + 3) % len(SC.GAN_N)] for j in range(njobs)]
    labels = [SC.GAN_LABELS[j % 2] for j in range(njobs)]
    scores = [Buf(n, data=SC.gan_scores(n, n + j)) for j, n in enumerate(ns)]
    gouts = [None if j == njobs - 1 else Buf(1, data=np.asarray([0.5 * j - 1.5])) for j in range(njobs)]     # the last job: no cotangent
    res, grads = Buf(njobs), [Buf(n) for n in ns]
    for backward in (0, 1):
        jobs = (CnGanJob * njobs)()
        for j, q in enumerate(jobs):
            q.s, q.n, q.label = scores[j].ptr, ns[j], labels[j]
            q.out = grads[j].ptr if backward else res.ptr + 4 * j
            q.gout = gouts[j].ptr if backward and gouts[j] is not None else None
        assert _call("gan_loss_grouped", jobs, njobs, backward) == 0
    assert res.intact() and all(g.intact() for g in grads) and all(b.unchanged() for b in scores + [g for g in gouts if g is not None])
    for j in range(njobs):
        one, g1 = Buf(1), Buf(ns[j])
        assert _call("gan_loss_fwd", scores[j], one, ns[j], labels[j]) == 0
        assert torch.equal(one.t, res.t[j:j + 1]), "job %d of %d (n %d): the grouped loss is not the single-head one" % (j, njobs, ns[j])
        if gouts[j] is None:
            assert not bool(grads[j].t.any()), "job %d: no cotangent must give a zero gradient" % j
        else:
            assert _call("gan_loss_bwd", scores[j], gouts[j], g1, ns[j], labels[j]) == 0
            assert torch.equal(g1.t, grads[j].t), "job %d of %d (n %d): the grouped gradient is not the single-head one" % (j, njobs, ns[j])


@pytest.mark.parametrize("with_ema", [True, False], ids=["ema", "null"])
@pytest.mark.parametrize("betas", SC.ADAM_BETAS, ids=lambda b: "b1_%g-b2_%g" % b)
@pytest.mark.parametrize("n", SC.ADAM_N)
def test_adam_step(n, betas, with_ema):
    b1, b2 = betas
    th, g, m, v, ema = SC.adam_state(n, n % 9973)
    bufs = {"theta": Buf(n, data=th), "g": Buf(n, data=g), "m": Buf(n, data=m), "v": Buf(n, data=v)}
    if with_ema:
        bufs["ema"] = Buf(n, data=ema)
    lr = Buf(1, data=np.asarray([SC.ADAM_LR], np.float32))
    assert _call("adam_step", bufs["theta"], bufs["g"], bufs["m"], bufs["v"], bufs.get("ema"), n, lr, b1, b2, SC.ADAM_EPS, SC.EMA_ALPHA) == 0
    assert bufs["g"].unchanged() and lr.unchanged()
    case = "n %d b1 %g b2 %g%s" % (n, b1, b2, "" if with_ema else " no ema")
    fails = []
    for key, (ref, bound) in SC.adam_bounds(th, g, m, v, ema if with_ema else None, SC.ADAM_LR, b1, b2, SC.ADAM_EPS, SC.EMA_ALPHA).items():
        assert bufs[key].intact(), key
        err = np.abs(bufs[key].values() - ref)
        _note("adam_step", case, key, err, bound)
        bad = np.flatnonzero(~(err <= bound))
        if len(bad):
            fails.append("%s[%d] off by %.3e, bound %.3e" % (key, bad[0], err[bad[0]], bound[bad[0]]))
    assert not fails, "adam_step %s: %s" % (case, "; ".join(fails))


@pytest.mark.parametrize("n", SC.ADAM_N)
def test_ema_step(n):
    th, _, _, _, ema = SC.adam_state(n, n % 9973 + 1)
    e, t = Buf(n, data=ema), Buf(n, data=th)
    assert _call("ema_step", e, t, n, SC.EMA_ALPHA) == 0
    assert e.intact() and t.unchanged()
    ref, bound = SC.ema_bound(ema, th, SC.EMA_ALPHA)
    err = np.abs(e.values() - ref)
    _note("ema_step", "n %d" % n, "ema", err, bound)
    assert (err <= bound).all(), "ema_step n %d: off by %.3e, bound %.3e" % (n, err.max(), bound[np.argmax(err)])


# ---- nothing to do, and arguments that are refused -----------------------------------------------------------------------------------
def test_empty_and_null_requests_write_nothing():
    n = 8
    f = lambda: Buf(n, data=np.arange(n, dtype=np.float64))
    a, b, c, d = f(), f(), f(), f()
    o, s, lr = Buf(n), Buf(3, data=np.asarray(SC.ROW_S)), Buf(1, data=np.asarray([SC.ADAM_LR]))
    m8 = Buf(n, torch.uint8, data=np.ones(n, np.uint8))
    perm, off = (ctypes.c_int * 3)(0, 1, 2), (ctypes.c_float * 3)(0, 0, 0)
    F = SC.F32
    empty = [("act_fwd", a, o, 0, SC.RELU, 0.0, F), ("act_bwd", a, b, o, 0, SC.RELU, 0.0, F), ("axpby", a, b, o, 0, 1.0, 1.0, F), ("mul", a, b, o, 0, F),
             ("cast", a, F, o, SC.BF16, 0), ("sqdiff_sum", a, b, o, 0, 1.0, F), ("masked_diff", a, b, m8, o, 0, 1),
             ("adam_step", o, a, b, c, d, 0, lr, 0.9, 0.999, 1e-7, 0.999), ("ema_step", o, a, 0, 0.999)]
    for name, *args in empty:
        assert _call(name, *args) == SC.CN_OK, name
    null = [("act_fwd", None, o, n, SC.RELU, 0.0, F), ("act_fwd", a, None, n, SC.RELU, 0.0, F),
            ("act_bwd", None, b, o, n, SC.RELU, 0.0, F), ("act_bwd", a, None, o, n, SC.RELU, 0.0, F), ("act_bwd", a, b, None, n, SC.RELU, 0.0, F),
            ("axpby", None, b, o, n, 1.0, 1.0, F), ("axpby", a, b, None, n, 1.0, 1.0, F),
            ("mul", None, b, o, n, F), ("mul", a, None, o, n, F), ("mul", a, b, None, n, F),
            ("cast", None, F, o, SC.BF16, n), ("cast", a, F, None, SC.BF16, n), ("cast", a, F, o, F, n),
            ("sqdiff_sum", None, b, o, n, 1.0, F), ("sqdiff_sum", a, None, o, n, 1.0, F), ("sqdiff_sum", a, b, None, n, 1.0, F),
            ("row_sumsq", None, o, 1, n), ("row_sumsq", a, None, 1, n), ("row_sumsq", a, o, 0, n), ("row_sumsq", a, o, 1, 0),
            ("row_scale", None, s, o, 1, n, 1.0, F), ("row_scale", a, None, o, 1, n, 1.0, F), ("row_scale", a, s, None, 1, n, 1.0, F),
            ("row_scale", a, s, o, 0, n, 1.0, F), ("row_scale", a, s, o, 1, 0, 1.0, F),
            ("row_scale_diff", None, b, s, o, 1, n, 1.0, F), ("row_scale_diff", a, None, s, o, 1, n, 1.0, F), ("row_scale_diff", a, b, None, o, 1, n, 1.0, F),
            ("row_scale_diff", a, b, s, None, 1, n, 1.0, F),
            ("tap_bwd", None, b, c, s, o, 1, n, 1.0, SC.RELU, 0.0, F), ("tap_bwd", a, None, c, s, o, 1, n, 1.0, SC.RELU, 0.0, F),
            ("tap_bwd", a, b, c, None, o, 1, n, 1.0, SC.RELU, 0.0, F), ("tap_bwd", a, b, c, s, None, 1, n, 1.0, SC.RELU, 0.0, F),
            ("masked_diff", None, b, m8, o, n, 1), ("masked_diff", a, b, None, o, n, 1), ("masked_diff", a, b, m8, None, n, 1), ("masked_diff", a, b, m8, o, n, 0),
            ("maxpool_fwd", None, o, 1, 2, 2, 2, 2, 2, 0, F), ("maxpool_fwd", a, None, 1, 2, 2, 2, 2, 2, 0, F), ("maxpool_fwd", a, o, 1, 2, 2, 2, 0, 2, 0, F),
            ("maxpool_bwd", None, b, o, 1, 2, 2, 2, 2, 2, 0, F), ("maxpool_bwd", a, None, o, 1, 2, 2, 2, 2, 2, 0, F), ("maxpool_bwd", a, b, None, 1, 2, 2, 2, 2, 2, 0, F),
            ("maxpool_bwd", a, b, o, 1, 2, 2, 2, 2, 0, 0, F),
            ("maxpool2_bwd_act", None, b, None, None, 0.0, o, 1, 2, 2, 2, 1, F), ("maxpool2_bwd_act", a, None, None, None, 0.0, o, 1, 2, 2, 2, 1, F),
            ("maxpool2_bwd_act", a, b, None, None, 0.0, None, 1, 2, 2, 2, 1, F),
            ("avgpool3_same", None, o, 1, 2, 2, 2, F), ("avgpool3_same", a, None, 1, 2, 2, 2, F), ("avgpool3_same", a, o, 0, 2, 2, 2, F),
            ("chan_affine3_fwd", None, o, 2, perm, 1.0, off), ("chan_affine3_fwd", a, None, 2, perm, 1.0, off), ("chan_affine3_fwd", a, o, 2, None, 1.0, off),
            ("chan_affine3_fwd", a, o, 2, (ctypes.c_int * 3)(0, 1, 3), 1.0, off),
            ("chan_affine3_bwd", None, o, 2, perm, 1.0), ("chan_affine3_bwd", a, None, 2, perm, 1.0), ("chan_affine3_bwd", a, o, 2, (ctypes.c_int * 3)(-1, 1, 2), 1.0),
            ("gan_loss_fwd", None, o, n, 1.0), ("gan_loss_fwd", a, None, n, 1.0), ("gan_loss_fwd", a, o, 0, 1.0),
            ("gan_loss_bwd", None, b, o, n, 1.0), ("gan_loss_bwd", a, None, o, n, 1.0), ("gan_loss_bwd", a, b, None, n, 1.0), ("gan_loss_bwd", a, b, o, 0, 1.0),
            ("adam_step", None, a, b, c, d, n, lr, 0.9, 0.999, 1e-7, 0.999), ("adam_step", o, None, b, c, d, n, lr, 0.9, 0.999, 1e-7, 0.999),
            ("adam_step", o, a, None, c, d, n, lr, 0.9, 0.999, 1e-7, 0.999), ("adam_step", o, a, b, None, d, n, lr, 0.9, 0.999, 1e-7, 0.999),
            ("adam_step", o, a, b, c, d, n, None, 0.9, 0.999, 1e-7, 0.999),
            ("ema_step", None, a, n, 0.999), ("ema_step", o, None, n, 0.999)]
    for name, *args in null:
        assert _call(name, *args) == SC.CN_EINVAL, (name, [type(x).__name__ for x in args])
    from confignet_amd._lib import CnGanJob
    jobs = (CnGanJob * 1)()
    jobs[0].s, jobs[0].out, jobs[0].n, jobs[0].label = a.ptr, None, n, 1.0
    assert _call("gan_loss_grouped", jobs, 1, 0) == SC.CN_EINVAL and _call("gan_loss_grouped", jobs, 0, 0) == SC.CN_OK and _call("gan_loss_grouped", None, 1, 0) == SC.CN_EINVAL
    torch.cuda.synchronize()
    for t in (a, b, c, d, o, s, lr, m8):
        assert t.unchanged()
