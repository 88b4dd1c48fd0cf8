"""What tests/test_rotate3d_cases_cpu.py and tests/test_rotate3d_edges_gpu.py share: a plain float64 statement of the 3-D resample
(csrc/rotate3d.hip: forward, grid gradient, matrix gradient), the matrices and data of its exact cases, the shapes that reach each
launch path, and the launch rule of cn_rotate3d_bwd written out once more in Python.  Nothing here needs a GPU.

bwd_plan() is a TRANSCRIPTION of the branches cn_rotate3d_bwd carried inline before plan_rotate3d_bwd existed, statement by
statement -- never generated from cn_rotate3d_bwd_plan, which it pins.

Exact cases.  Every matrix of MATRICES has entries that are multiples of 1/4 and every centred voxel coordinate is a multiple of
1/2, so every sample coordinate, fractional part and tap weight is a dyadic rational of a few bits; grid and gout hold small
integers.  Every product the kernels form is then a multiple of 2^-k, and where (sum of |contributions|) 2^k < 2^24 for an output
element fp32 holds each partial sum of its contributions exactly, in any order, fused or not: the kernels must give the float64
result element for element, whichever order their atomics land in.  reference(..., stats=True) returns that sum and that k per
output element (k as the exponent of the contribution's WEIGHT wherever its integer factor is non-zero: the smallest k if the
integer is odd, an upper bound of it otherwise, which only makes the condition stricter);
tests/test_rotate3d_cases_cpu.py holds the condition for every case."""
import functools

import torch

SLAB_FLOATS = 32768                                   # csrc/rotate3d.hip: floats of a workgroup's LDS slab
DET, LDS, GLOBAL = 0, 1, 2                            # the path codes of cn_rotate3d_bwd_plan

# each sample of a call takes the next one (rotations): consecutive samples differ, so a wrong rot + n * 9 stride shows
MATRICES = [
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]],                      # identity: every coordinate an integer, 0 and G - 1 among them
    [[0, 1, 0], [0, 0, 1], [1, 0, 0]],                      # a cyclic axis permutation
    [[1, 0, 0], [0, 0, -1], [0, 1, 0]],                     # a quarter turn about the first axis
    [[0, 1, 0], [1, 0, 0], [0, 0, -1]],                     # an axis swap with one negation
    [[.5, 0, 0], [0, .5, 0], [0, 0, .5]],                   # I / 2: nothing clamps
    [[2, 0, 0], [0, 2, 0], [0, 0, 2]],                      # 2 I: most voxels clamp
    [[1, .5, 0], [0, 1, .25], [-.5, 0, 1]],                 # a shear
    [[.5, -.5, 0], [.5, .5, 0], [0, 0, 1.5]],               # a scaled eighth turn with a stretch
    [[0, 0, 0], [0, 0, 0], [0, 0, 0]],                      # zero: every voxel reads the centre (even G: P voxels scatter to 8 addresses)
]

# (G, C, N): the smallest shape that reaches each edge
FWD_SHAPES = [(3, 4, 3),            # one partial block
              (5, 12, 2),           # two blocks, the second ragged
              (16, 8, 2)]           # the workload's grid extent
# (G, C, N, deterministic mode, path, channels per workgroup, largest |value| of grid and gout, one grid value in `keep` is non-zero).
# The values are what the exactness condition needs: [-4, 4] at small G, {-1, 0, 1} from G = 16.  The matrix gradient of
# (16, 128, 16) adds 2^19 voxel-channel terms of up to 2^-6 in unit, more than 2^24 holds even with {-1, 0, 1}; there seven grid
# values of eight are zero (every voxel still has about 128 non-zero source values among its 8 x 128; gout, which is all that the
# grid gradient depends on, stays dense).
BWD_CASES = [
    (2, 4, 2, 0, LDS, 4, 4, 1),        # 8 voxels under 256 threads
    (3, 12, 3, 0, LDS, 4, 4, 1),       # integer centre, three channel blocks
    (4, 12, 128, 0, LDS, 8, 4, 1),     # CC = 8, the last block with 4 live channels
    (2, 20, 128, 0, LDS, 16, 4, 1),    # CC = 16, the last block with 4
    (20, 4, 1, 0, LDS, 4, 1, 1),       # 32000 of the slab's 32768 floats
    (16, 128, 16, 0, LDS, 8, 1, 8),    # the workload's launch: CC = 8, the whole slab, 256 workgroups
    (21, 4, 2, 0, GLOBAL, 4, 1, 1),    # 36 full blocks and a tail of 45 voxels
    (21, 12, 1, 0, GLOBAL, 12, 1, 1),  # the loop over c / 4 channel groups
    (3, 4, 3, 1, DET, 8, 4, 1),        # P % 4 = 3, four dead lanes per tap
    (5, 12, 3, 1, DET, 8, 4, 1),       # P % 4 = 1, the second channel block half dead, two partial rows summed
    (16, 8, 2, 1, DET, 8, 1, 1),       # the full slab
    (2, 20, 2, 1, DET, 8, 4, 1),       # 8 voxels, second and third channel blocks
    (17, 4, 1, 1, LDS, 4, 1, 1),       # deterministic mode above G = 16 falls to the LDS kernel ...
    (21, 4, 1, 1, GLOBAL, 4, 1, 1),    # ... and above G = 20 to global atomics (values only: the order of their sums is free)
]
FWD_VALUE = 4                                          # largest |value| of the forward cases
# one shape per backward path for the float64 comparison with rotations that are not exact: (G, C, N, deterministic mode, path)
ROUNDING_CASES = [(16, 16, 2, 0, LDS), (16, 16, 2, 1, DET), (21, 4, 2, 0, GLOBAL)]


def cdiv(a, b):
    return (a + b - 1) // b


def bwd_plan(n, g, c, det):
    """[path, channels per workgroup, grid x, grid y]: the branches of cn_rotate3d_bwd"""
    P = g * g * g
    if det and P * 8 <= SLAB_FLOATS:
        cblocks = cdiv(c, 8)
        return [DET, 8, cblocks, n]
    if P * 4 <= SLAB_FLOATS:
        CC = SLAB_FLOATS // P
        if CC > c:
            CC = c
        CC = CC // 4 * 4
        while CC > 4 and cdiv(c, CC) * n < 256:
            CC -= 4
        return [LDS, CC, cdiv(c, CC), n]
    return [GLOBAL, c, cdiv(P, 256), n]


def starts(n):
    """the first matrix of each launch of an n-sample case: together the launches take every matrix"""
    return list(range(0, len(MATRICES), n))


def rotations(n, start=0):
    """(n, 3, 3) float64: sample i takes MATRICES[(start + i) % 9]"""
    return torch.tensor([MATRICES[(start + i) % len(MATRICES)] for i in range(n)], dtype=torch.float64)


def integers(shape, value, seed):
    """float64 integers, uniform in [-value, value]"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-value, value + 1, shape, generator=gen).double()


def dyadic_exponent(v, most=12):
    """the smallest k with v 2^k an integer, per element"""
    k = torch.zeros(v.shape, dtype=torch.int64, device=v.device)
    for i in range(most):
        s = v * 2.0 ** i
        k += s != s.round()
    s = v * 2.0 ** most
    assert bool((s == s.round()).all()), "not a dyadic rational of %d bits" % most
    return k


def _one_sample(grid, R, gout, stats, closed):
    """grid (G, G, G, C), R (3, 3), gout like grid or None -> out, ggrid, grot (the last two None without gout) and the statistics"""
    G, C = grid.shape[0], grid.shape[-1]
    P, dev = G ** 3, grid.device
    ctr = (G - 1) / 2
    ar = torch.arange(G, dtype=torch.float64, device=dev)
    pc = torch.stack([m.reshape(-1) for m in torch.meshgrid(ar, ar, ar, indexing="ij")]) - ctr         # (3, P), voxel p = (i G + j) G + k
    q = R @ pc + ctr                                                                                    # q = R (p - ctr) + ctr
    passes = ((q >= 0) if closed[0] else (q > 0)) & ((q <= G - 1) if closed[1] else (q < G - 1))        # clip_by_value passes the gradient
    q = q.clamp(0, G - 1)
    f = q.floor()
    i0 = f.long()
    i1 = (i0 + 1).clamp(max=G - 1)
    d = q - f
    taps = range(8)                                                                                     # bit 0: x, bit 1: y, bit 2: z
    pick = lambda a, t: (t >> a) & 1
    off = [((i1[0] if pick(0, t) else i0[0]) * G + (i1[1] if pick(1, t) else i0[1])) * G + (i1[2] if pick(2, t) else i0[2]) for t in taps]
    wa = lambda a, t: d[a] if pick(a, t) else 1 - d[a]                                                  # (P,)
    w = [wa(0, t) * wa(1, t) * wa(2, t) for t in taps]
    src = grid.reshape(P, C)
    v = [src[o] for o in off]                                                                           # (P, C) each
    dx, dy, dz = (d[a].unsqueeze(-1) for a in range(3))
    lerp = lambda a, b, t: a * (1 - t) + b * t
    c00, c10, c01, c11 = lerp(v[0], v[1], dx), lerp(v[2], v[3], dx), lerp(v[4], v[5], dx), lerp(v[6], v[7], dx)
    c0, c1 = lerp(c00, c10, dy), lerp(c01, c11, dy)
    res = {"out": lerp(c0, c1, dz).reshape(grid.shape), "ggrid": None, "grot": None}
    st = {}
    kw = [dyadic_exponent(x) for x in w] if stats else None
    if stats:
        st["out"] = (sum(w[t].unsqueeze(-1) * v[t].abs() for t in taps).reshape(grid.shape),
                     torch.stack([kw[t].unsqueeze(-1) * (v[t] != 0) for t in taps]).amax(0).reshape(grid.shape))
    if gout is None:
        return res, st
    go = gout.reshape(P, C)
    gg = torch.zeros(P, C, dtype=torch.float64, device=dev)
    for t in taps:
        gg.index_add_(0, off[t], w[t].unsqueeze(-1) * go)
    res["ggrid"] = gg.reshape(grid.shape)
    # d out / d q, axis by axis, through the same lerps
    gq = torch.stack([(go * lerp(lerp(v[1] - v[0], v[3] - v[2], dy), lerp(v[5] - v[4], v[7] - v[6], dy), dz)).sum(-1),
                      (go * lerp(c10 - c00, c11 - c01, dz)).sum(-1),
                      (go * (c1 - c0)).sum(-1)])                                                         # (3, P)
    res["grot"] = (gq * passes) @ pc.T                                                                   # [a][b] = sum_p gq[a] pc[b]
    if stats:
        ab = torch.zeros(P, C, dtype=torch.float64, device=dev)
        kk = torch.zeros(P, C, dtype=torch.int64, device=dev)
        for t in taps:
            ab.index_add_(0, off[t], w[t].unsqueeze(-1) * go.abs())
            kk.scatter_reduce_(0, off[t].unsqueeze(-1).expand(P, C), kw[t].unsqueeze(-1) * (go != 0), "amax")
        st["ggrid"] = (ab.reshape(grid.shape), kk.reshape(grid.shape))
        kd, kp = dyadic_exponent(d), dyadic_exponent(pc)
        ab, kk = torch.zeros(3, 3, dtype=torch.float64, device=dev), torch.zeros(3, 3, dtype=torch.int64, device=dev)
        for a in range(3):
            o1, o2 = [x for x in range(3) if x != a]                         # the weight of a tap's term: those of the other two axes
            per = sum((go.abs() * v[t].abs()).sum(-1) * wa(o1, t) * wa(o2, t) for t in taps) * passes[a]           # (P,)
            ab[a] = (pc.abs() * per).sum(-1)
            kk[a] = ((kd[o1] + kd[o2] + kp) * (per != 0)).amax(-1)
        st["grot"] = (ab, kk)
    return res, st


def reference(grid, rot, gout=None, stats=False, closed=(True, True)):
    """The operation in float64 on the device of `grid`: grid (N, G, G, G, C), rot (N, 3, 3), gout like grid.  q = R (p - ctr) + ctr,
    clamped to [0, G - 1] with the gradient passed where the raw coordinate lies in the CLOSED interval (closed=(low, high) opens an end,
    for the test that tells them apart), floor, x1 = min(x0 + 1, G - 1), lerp x, then y, then z.
    Returns {"out", "ggrid", "grot"}; with stats also {"out", "ggrid", "grot"} -> (sum of |contributions|, k) per element."""
    assert grid.dtype == torch.float64 and rot.dtype == torch.float64 and grid.shape[1] == grid.shape[2] == grid.shape[3]
    per = [_one_sample(grid[n], rot[n].to(grid.device), None if gout is None else gout[n], stats, closed) for n in range(grid.shape[0])]
    join = lambda xs: None if xs[0] is None else torch.stack(xs)
    res = {key: join([r[key] for r, _ in per]) for key in ("out", "ggrid", "grot")}
    if not stats:
        return res
    return res, {key: (torch.stack([s[key][0] for _, s in per]), torch.stack([s[key][1] for _, s in per])) for key in per[0][1]}


def exact_margin(stat):
    """the largest (sum of |contributions|) 2^k over the elements; the sums are exact in any order where it is below 2^24"""
    ab, k = stat
    return float((ab * 2.0 ** k.double()).max())


def exact_inputs(g, c, n, value, keep, start):
    """(grid, rot, gout) of an exact case, float64 on the CPU"""
    shape = (n, g, g, g, c)
    grid, gout = integers(shape, value, 1000 * g + c + n + start), integers(shape, value, 2000 * g + c + n + start)
    if keep > 1:
        gen = torch.Generator().manual_seed(3000 * g + c + n + start)
        grid = grid * (torch.randint(0, keep, shape, generator=gen) == 0)
    return grid, rotations(n, start), gout


@functools.lru_cache(maxsize=None)
def exact_case(g, c, n, value, keep, start, device="cpu"):
    """(grid, rot, gout, reference): exact_inputs and their reference, computed on `device` and kept on the CPU; shared by the tests that
    need it and never changed"""
    grid, rot, gout = exact_inputs(g, c, n, value, keep, start)
    ref = reference(grid.to(device), rot.to(device), gout.to(device))
    return grid, rot, gout, {k: v.cpu() for k, v in ref.items()}
