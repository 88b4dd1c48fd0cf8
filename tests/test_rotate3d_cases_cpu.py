"""What tests/test_rotate3d_edges_gpu.py stands on, checked without a GPU (tests/rotate3d_cases.py):
  * its float64 reference is oracle.ref_ops.transform_3d_grid under autograd -- output, grid gradient, matrix gradient -- on the exact
    cases and on random matrices, and passes the clamp's gradient on the closed interval as the oracle and the kernels do;
  * every exact case meets the condition under which fp32 holds every partial sum in any order: (sum of |contributions|) 2^k < 2^24
    for every output element (a condition, not a tolerance);
  * cn_rotate3d_bwd_plan (csrc/rotate3d.hip: plan_rotate3d_bwd is the function cn_rotate3d_bwd decides with) is the hand-written
    transcription of the launcher's former branches, on every shape of the GPU file, on both sides of every boundary of the rule and
    around them, and names the path and the channels per workgroup each case is meant to reach."""
import ctypes

import pytest
import torch

from oracle import ref_ops as O
from tests import rotate3d_cases as RC

CN_EINVAL = -1
FWD = [(g, c, n, RC.FWD_VALUE, 1) for g, c, n in RC.FWD_SHAPES]
BWD = sorted({(g, c, n, value, keep) for g, c, n, _, _, _, value, keep in RC.BWD_CASES})
EXACT = sorted(set(FWD + BWD))
_id = lambda s: "x".join(map(str, s))


def oracle(grid, rot, gout):
    gr, rr = grid.clone().requires_grad_(True), rot.clone().requires_grad_(True)
    out = O.transform_3d_grid(gr, rr)
    (out * gout).sum().backward()
    return {"out": out.detach(), "ggrid": gr.grad, "grot": rr.grad}


@pytest.mark.parametrize("case", EXACT, ids=_id)
def test_the_reference_is_the_oracle_on_the_exact_cases(case):
    """element for element: both are exact in float64 on these inputs.  (At most nine samples -- every matrix -- and twelve channels of
    a case: the oracle materialises eight gathers of the whole volume.)"""
    g, c, n, value, keep = case
    for start in RC.starts(n):
        grid, rot, gout = (t[:9] for t in RC.exact_inputs(g, c, n, value, keep, start))
        grid, gout = grid[..., :12].contiguous(), gout[..., :12].contiguous()
        got, want = RC.reference(grid, rot, gout), oracle(grid, rot, gout)
        for key in ("out", "ggrid", "grot"):
            assert torch.equal(got[key], want[key]), (case, start, key)


@pytest.mark.parametrize("g,c,n", [(2, 4, 3), (5, 4, 4), (8, 8, 3), (21, 4, 1)], ids=lambda v: str(v))
def test_the_reference_is_the_oracle_on_random_matrices(g, c, n):
    gen = torch.Generator().manual_seed(g)
    grid, gout = (torch.randn(n, g, g, g, c, generator=gen, dtype=torch.float64) for _ in range(2))
    for scale in (0.3, 1.0, 2.5):                                         # nothing clamps ... most voxels clamp
        rot = torch.randn(n, 3, 3, generator=gen, dtype=torch.float64) * scale
        got, want = RC.reference(grid, rot, gout), oracle(grid, rot, gout)
        for key in ("out", "ggrid", "grot"):
            err = float((got[key] - want[key]).abs().max() / want[key].abs().max())
            assert err < 1e-12, (key, scale, err)
        assert float(want["grot"].abs().max()) > 0


def test_the_clamp_passes_its_gradient_on_the_closed_interval():
    """Identity at G = 3: every coordinate is 0, 1 or 2.  On 0 the derivative is grid[1] - grid[0] and reaches the matrix only if the
    clamp passes it there: the oracle agrees with the closed interval, not the open one.  On G - 1 the clamp passes it too
    (torch.clamp, as tf.clip_by_value), but x1 = min(x0 + 1, G - 1) = x0 there: the two taps coincide and the derivative is zero
    whatever the clamp does -- opening the interval at G - 1 alone changes nothing."""
    g = 3
    grid, rot, gout = RC.exact_inputs(g, 4, 1, 4, 1, 0)
    assert torch.equal(rot[0], torch.eye(3, dtype=torch.float64))
    want = oracle(grid, rot, gout)["grot"]
    assert torch.equal(RC.reference(grid, rot, gout)["grot"], want)
    assert not torch.equal(RC.reference(grid, rot, gout, closed=(False, True))["grot"], want)
    assert torch.equal(RC.reference(grid, rot, gout, closed=(True, False))["grot"], want)          # G - 1: no difference to see
    x = torch.tensor([0.0, float(g - 1)], dtype=torch.float64, requires_grad=True)             # exactly on both ends
    torch.clamp(x, 0, g - 1).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0]


@pytest.mark.parametrize("case", [x + ("fwd",) for x in FWD] + [x + ("bwd",) for x in BWD], ids=_id)
def test_every_exact_case_is_exact_in_any_order(case):
    g, c, n, value, keep, kind = case
    for start in RC.starts(n):
        grid, rot, gout = RC.exact_inputs(g, c, n, value, keep, start)
        assert float(grid.abs().max()) == value and float(gout.abs().max()) == value
        _, stats = RC.reference(grid, rot, gout, stats=True)
        for key in (("out",) if kind == "fwd" else ("ggrid", "grot")):
            margin = RC.exact_margin(stats[key])
            assert 0 < margin < 2 ** 24, "%s start %d %s: (sum |contributions|) 2^k = %g" % (case, start, key, margin)


def test_what_the_matrices_exercise():
    """the permutations put every coordinate on an integer, 0 and G - 1 among them; 2 I, the shear and the mix clamp a good share of
    the voxels; consecutive samples differ"""
    assert all(RC.MATRICES[i] != RC.MATRICES[i + 1] for i in range(len(RC.MATRICES) - 1))
    for g in (2, 3, 4, 5, 16, 21):
        ar = torch.arange(g, dtype=torch.float64)
        pc = torch.stack([m.reshape(-1) for m in torch.meshgrid(ar, ar, ar, indexing="ij")]) - (g - 1) / 2
        q = torch.tensor(RC.MATRICES, dtype=torch.float64) @ pc + (g - 1) / 2                  # (9, 3, P)
        for i in range(4):
            assert torch.equal(q[i], q[i].round()) and float(q[i].min()) == 0 and float(q[i].max()) == g - 1
        clamped = ((q < 0) | (q > g - 1)).any(1).double().mean(1)
        assert 0.78 <= float(clamped[5]) <= 1.0 and float(clamped[4]) == 0
        assert all(0.28 <= float(x) <= (0.75 if g > 2 else 1.0) for x in clamped[6:8]), (g, clamped)
        assert torch.equal(q[8], torch.full_like(q[8], (g - 1) / 2))


# ---- the launch rule ----------------------------------------------------------------------------------------------------------------
def report(n, g, c, det):
    from confignet_amd._lib import lib
    out = (ctypes.c_int * 4)()
    assert lib.cn_rotate3d_bwd_plan(n, g, c, det, ctypes.byref(out)) == 0, (n, g, c, det)
    return list(out)


# (n, g, c, det) on both sides of each boundary: the deterministic slab (G = 16 | 17), the LDS slab (G = 20 | 21), and 255 | 256
# workgroups in the loop that shrinks CC -- as 1 x 255 | 256, as 5 x 51 | 52 (c = 40) and as 2 x 127 | 128 (c = 12)
BOUNDARIES = [(2, 16, 8, 1), (2, 17, 8, 1), (2, 16, 8, 0), (2, 17, 8, 0), (2, 20, 8, 0), (2, 21, 8, 0), (2, 20, 8, 1), (2, 21, 8, 1),
              (255, 4, 8, 0), (256, 4, 8, 0), (51, 4, 40, 0), (52, 4, 40, 0), (127, 4, 12, 0), (128, 4, 12, 0),
              (15, 16, 128, 0), (16, 16, 128, 0), (8, 16, 128, 0)]


def test_the_plan_of_every_gpu_case_is_the_one_it_is_meant_to_reach():
    for g, c, n, det, path, cc, _, _ in RC.BWD_CASES:
        got = report(n, g, c, det)
        assert got == RC.bwd_plan(n, g, c, det) and got[:2] == [path, cc], (g, c, n, det, got)
        assert report(n, g, c, 0)[0] != RC.DET
    for g, c, n, det, path in RC.ROUNDING_CASES:
        got = report(n, g, c, det)
        assert got == RC.bwd_plan(n, g, c, det) and got[0] == path, (g, c, n, det, got)
    # what the notes quote: the workload's launch, and the one the shrinking loop was written for
    assert report(16, 16, 128, 0) == [RC.LDS, 8, 16, 16] and report(8, 16, 128, 0) == [RC.LDS, 4, 32, 8]
    assert report(128, 4, 12, 0) == [RC.LDS, 8, 2, 128] and report(128, 2, 20, 0) == [RC.LDS, 16, 2, 128]
    assert report(2, 21, 4, 0) == [RC.GLOBAL, 4, 37, 2] and report(3, 5, 12, 1) == [RC.DET, 8, 2, 3]


def test_the_plan_on_both_sides_of_every_boundary():
    sides = {q: report(*q) for q in BOUNDARIES}
    for q, got in sides.items():
        assert got == RC.bwd_plan(*q), q
    assert [sides[q][0] for q in BOUNDARIES[:8]] == [RC.DET, RC.LDS, RC.LDS, RC.LDS, RC.LDS, RC.GLOBAL, RC.LDS, RC.GLOBAL]
    assert [sides[q][1] for q in BOUNDARIES[8:]] == [4, 8, 4, 8, 4, 8, 4, 8, 4]
    for n, g, c, det in BOUNDARIES[8:]:                                # the loop stops at 256 workgroups or at CC = 4
        path, cc, gx, gy = sides[(n, g, c, det)]
        assert gx * gy >= 256 or cc == 4
        assert cc * g ** 3 <= RC.SLAB_FLOATS and (gx - 1) * cc < c <= gx * cc and gy == n


def test_the_plan_is_the_transcription_around_every_shape():
    asked = [(n, g, c, det) for g, c, n, det, *_ in RC.BWD_CASES] + [(n, g, c, det) for g, c, n, det, _ in RC.ROUNDING_CASES] + BOUNDARIES
    seen = set()
    for n, g, c, det in asked:
        for dn in (-1, 0, 1):
            for dc in (-4, 0, 4):
                for d in (0, 1):
                    q = (n + dn, g, c + dc, d)
                    if q[0] > 0 and q[2] > 0 and q not in seen:
                        seen.add(q)
                        assert report(*q) == RC.bwd_plan(*q), q
    assert len(seen) > 8 * len(set(asked))
    for g in range(2, 40):                                             # every extent up to well past the last boundary
        for det in (0, 1):
            for n, c in ((1, 4), (16, 128), (300, 36)):
                assert report(n, g, c, det) == RC.bwd_plan(n, g, c, det), (n, g, c, det)


def test_bad_plan_requests_are_argument_errors():
    """what cn_rotate3d_bwd refuses: no samples, an extent below 2, no channels, channels that are no multiple of 4"""
    from confignet_amd._lib import lib
    out = (ctypes.c_int * 4)()
    for args in ((0, 4, 4, 0), (-1, 4, 4, 0), (1, 1, 4, 0), (1, 0, 4, 1), (1, 4, 0, 0), (1, 4, 6, 0), (1, 4, -4, 1)):
        assert lib.cn_rotate3d_bwd_plan(*args, ctypes.byref(out)) == CN_EINVAL, args
    assert lib.cn_rotate3d_bwd_plan(1, 4, 4, 0, None) == CN_EINVAL
    assert lib.cn_rotate3d_bwd(None, None, None, None, None, 1, 4, 6, None) == CN_EINVAL
