"""The 3-D resample (csrc/rotate3d.hip) on every launch path, called through `lib` at the smallest shapes that reach each edge
(tests/rotate3d_cases.py: FWD_SHAPES, BWD_CASES and what each reaches): the forward kernel, the LDS-slab, global-atomics and
deterministic backward kernels, with the matrix gradient requested and with grot == NULL.

Exact arithmetic: the matrices are multiples of 1/4, grid and gout small integers, and every case meets
(sum of |contributions|) 2^k < 2^24 for every output element (tests/test_rotate3d_cases_cpu.py), so fp32 holds every partial sum
in any order and the kernels must give the float64 reference element for element -- one wrong tap, weight, voxel, channel or
sample shows as a whole number of units.  Each sample of a call takes the next matrix of the list and a case is launched until every
matrix has been used.  Outputs hold NaN before the call, 256 guard floats on both sides stay (tests/chan_slices_cases.py: Guarded).
Before each launch the plan query must name the path and channels per workgroup the case is meant for.

Rounding pass: what exact cases cannot show.  One shape per backward path with rotations from three non-zero Euler angles, the
matrix rounded to fp32 before kernel and reference see it, against float64 at the tolerances of tests/test_ops_gpu.py::test_rotate3d
(2e-4 forward, 5e-4 grid gradient, 2e-3 matrix gradient, of the largest reference magnitude); the Euler kernels at n = 65 and
n = 130 (two and three blocks of 64, the last with one and two live threads) at 1e-6 / 1e-5.  The measured errors are in
profiles/rotate3d_edges_errors.txt, written by this file when ROTATE3D_EDGE_ERRORS names a path."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import ref_ops as O
from tests import rotate3d_cases as RC
from tests.chan_slices_cases import GUARD, GUARD_VALUE, Guarded, to_device as _dev

pytestmark = pytest.mark.gpu

_id = lambda s: "x".join(map(str, s))
BIG = 1 << 22                                           # elements from which the float64 reference runs on the device


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(n, g, c, det):
    from confignet_amd._lib import lib
    out = (ctypes.c_int * 4)()
    assert lib.cn_rotate3d_bwd_plan(n, g, c, det, ctypes.byref(out)) == 0
    return list(out)


def _forward(grid, rot):
    from confignet_amd._lib import check, lib
    n, g, c = grid.shape[0], grid.shape[1], grid.shape[-1]
    out = Guarded(tuple(grid.shape))
    check(lib.cn_rotate3d_fwd(grid.data_ptr(), rot.data_ptr(), out.t.data_ptr(), n, g, c, _stream()), "cn_rotate3d_fwd")
    return out


def _backward(grid, rot, gout, need_rot):
    from confignet_amd._lib import check, lib
    n, g, c = grid.shape[0], grid.shape[1], grid.shape[-1]
    ggrid, grot = Guarded(tuple(grid.shape)), Guarded((n, 3, 3)) if need_rot else None
    check(lib.cn_rotate3d_bwd(grid.data_ptr(), rot.data_ptr(), gout.data_ptr(), ggrid.t.data_ptr(), grot.t.data_ptr() if need_rot else None,
                              n, g, c, _stream()), "cn_rotate3d_bwd")
    return ggrid, grot


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


def _exact(g, c, n, value, keep, start):
    return RC.exact_case(g, c, n, value, keep, start, "cuda" if n * g ** 3 * c >= BIG else "cpu")


@pytest.mark.parametrize("shape", RC.FWD_SHAPES, ids=_id)
def test_forward_exact(shape):
    g, c, n = shape
    for start in RC.starts(n):
        grid, rot, _, ref = _exact(g, c, n, RC.FWD_VALUE, 1, start)
        _forward(_dev(grid), _dev(rot)).check(ref["out"], "forward %s from matrix %d" % (shape, start))


@pytest.mark.parametrize("need_rot", [True, False], ids=["grot", "null"])
@pytest.mark.parametrize("case", RC.BWD_CASES, ids=lambda s: _id(s[:4]))
def test_backward_exact(case, need_rot):
    g, c, n, det, path, cc, value, keep = case
    with _Mode(det):
        for start in RC.starts(n):
            grid, rot, gout, ref = _exact(g, c, n, value, keep, start)
            what = "backward (G %d, C %d, N %d) det %d from matrix %d" % (g, c, n, det, start)
            d = [_dev(t) for t in (grid, rot, gout)]
            assert _plan(n, g, c, det)[:2] == [path, cc], what
            ggrid, grot = _backward(*d, need_rot)
            ggrid.check(ref["ggrid"], what + ": ggrid")
            if need_rot:
                grot.check(ref["grot"], what + ": grot")
            if path == RC.DET:                                        # the same bits twice
                again, grot2 = _backward(*d, need_rot)
                assert torch.equal(again.t, ggrid.t) and (not need_rot or torch.equal(grot2.t, grot.t)), what + ": second run differs"


def test_autograd_without_a_matrix_gradient():
    """Rotate3dFn with a matrix that needs no gradient: the exact grid gradient (grot == NULL in the call) and None"""
    from confignet_amd.functional import Rotate3dFn
    g, c, n = 5, 12, 3
    grid, rot, gout, ref = _exact(g, c, n, 4, 1, 6)                    # shear, mix, zero
    x, r = _dev(grid).requires_grad_(True), _dev(rot)
    out = Rotate3dFn.apply(x, r)
    assert torch.equal(out.detach().double().cpu(), ref["out"])
    got = out.grad_fn.apply(_dev(gout))
    assert len(got) == 2 and got[1] is None and torch.equal(got[0].double().cpu(), ref["ggrid"])
    out.backward(_dev(gout))
    assert torch.equal(x.grad.double().cpu(), ref["ggrid"]) and r.grad is None


# ---- rounding pass ---------------------------------------------------------------------------------------------------------------------
TOL = {"out": 2e-4, "ggrid": 5e-4, "grot": 2e-3, "euler matrix": 1e-6, "euler gradient": 1e-5}
PATH_NAMES = {RC.DET: "rotate3d_bwd_det_kernel", RC.LDS: "rotate3d_bwd_lds_kernel", RC.GLOBAL: "rotate3d_bwd_kernel"}
_ERRORS = {}               # (kernel, case, quantity) -> (error, tolerance)


def _note(kernel, case, quantity, err, tol):
    if not err <= _ERRORS.get((kernel, case, quantity), (-1.0, tol))[0]:         # (the larger of a quantity measured twice)
        _ERRORS[(kernel, case, quantity)] = (err, tol)
    path = os.environ.get("ROTATE3D_EDGE_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("Rounding pass of tests/test_rotate3d_edges_gpu.py, one MI355X (written when ROTATE3D_EDGE_ERRORS names a path): standard-normal\n"
                    "grid and gout, three non-zero Euler angles in +-1.2 per sample, the matrix rounded to fp32 before kernel and reference see it.\n"
                    "error = max |got - float64 reference| / max |reference| (Euler kernels: / max(1, max |reference|)); the test holds it at the\n"
                    "tolerance, which is that of tests/test_ops_gpu.py::test_rotate3d.\n\n")
            f.write("%-26s %-22s %-16s %10s %10s\n" % ("kernel", "case (G, C, N) or n", "quantity", "error", "tolerance"))
            for (k, c, q), (e, t) in sorted(_ERRORS.items()):
                f.write("%-26s %-22s %-16s %10.3e %10.0e\n" % (k, c, q, e, t))


def _hold(kernel, case, quantity, got, ref, floor=0.0):
    ref = ref.double().cpu()
    err = float((got.double().cpu() - ref).abs().max() / max(floor, float(ref.abs().max())))
    print("%s %s %s: error %.3e (tolerance %.0e)" % (kernel, case, quantity, err, TOL[quantity]))
    _note(kernel, case, quantity, err, TOL[quantity])
    return err <= TOL[quantity], "%s %s %s: error %.3e above %.0e" % (kernel, case, quantity, err, TOL[quantity])


@pytest.mark.parametrize("case", RC.ROUNDING_CASES, ids=lambda s: _id(s[:4]))
def test_against_float64_with_rotations_that_are_not_exact(case):
    g, c, n, det, path = case
    gen = torch.Generator().manual_seed(100 * g + c + det)
    angles = (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 1.1 + 0.1) * (torch.randint(0, 2, (n, 3), generator=gen) * 2 - 1)
    assert float(angles.abs().min()) >= 0.1 and float(angles.abs().max()) <= 1.2
    rot = O.euler_angles_to_matrix(angles).float()                                   # rounded before both see it
    grid, gout = (torch.randn(n, g, g, g, c, generator=gen).float() for _ in range(2))
    ref = RC.reference(grid.double(), rot.double(), gout.double())
    d = [_dev(t) for t in (grid, rot, gout)]
    name, shape = PATH_NAMES[path], str((g, c, n))
    results = [_hold("rotate3d_fwd_kernel", shape, "out", _forward(d[0], d[1]).t, ref["out"])]
    with _Mode(det):
        assert _plan(n, g, c, det)[0] == path
        ggrid, grot = _backward(*d, True)
        only, _ = _backward(*d, False)
    results += [_hold(name, shape, "ggrid", ggrid.t, ref["ggrid"]), _hold(name, shape, "grot", grot.t, ref["grot"])]
    assert not bool(only.t.isnan().any())
    results.append(_hold(name, shape, "ggrid", only.t, ref["ggrid"]) if path != RC.DET else (torch.equal(only.t, ggrid.t), "grot == NULL changes ggrid"))
    for ok, why in results:
        assert ok, why


@pytest.mark.parametrize("n", [65, 130])
def test_euler_kernels_past_one_block(n):
    """fp32-representable angles across +-pi, all three non-zero, against float64 of the same angles"""
    from confignet_amd import ops
    angles = torch.linspace(-math.pi, math.pi, 3 * n, dtype=torch.float64).float()     # both ends: fp32 pi, just past pi
    angles[angles == 0] = 0.5
    angles = angles[torch.randperm(3 * n, generator=torch.Generator().manual_seed(n))].reshape(n, 3)
    assert float(angles.abs().min()) > 0 and float(angles.abs().max()) == float(np.float32(math.pi))
    a64 = angles.double().requires_grad_(True)
    R64 = O.euler_angles_to_matrix(a64)
    cot = torch.randn(n, 3, 3, generator=torch.Generator().manual_seed(n + 1)).float()
    (R64 * cot.double()).sum().backward()
    ad = _dev(angles)
    R, ga = Guarded((n, 3, 3)), Guarded((n, 3))
    from confignet_amd._lib import check, lib
    check(lib.cn_euler_matrix(ad.data_ptr(), R.t.data_ptr(), n, _stream()), "cn_euler_matrix")
    check(lib.cn_euler_matrix_bwd(ad.data_ptr(), _dev(cot).data_ptr(), ga.t.data_ptr(), n, _stream()), "cn_euler_matrix_bwd")
    edge = torch.full_like(R.buf[:GUARD], GUARD_VALUE)
    for t in (R, ga):
        assert torch.equal(t.buf[:GUARD], edge) and torch.equal(t.buf[-GUARD:], edge) and not bool(t.t.isnan().any())
    assert torch.equal(ops.euler_matrix(ad), R.t) and torch.equal(ops.euler_matrix_bwd(ad, _dev(cot)), ga.t)
    results = [_hold("euler_matrix_kernel", "n = %d" % n, "euler matrix", R.t, R64.detach(), 1.0),
               _hold("euler_matrix_bwd_kernel", "n = %d" % n, "euler gradient", ga.t, a64.grad, 1.0)]
    for ok, why in results:
        assert ok, why
