"""Shared helpers of the grouped filter-gradient tests (tests/test_wgrad_grouped_plan_cpu.py, tests/test_wgrad_grouped_gpu.py).
Plain Python: nothing here touches a device."""
from confignet_amd import ops
from confignet_amd.dnn_models.real_encoder import C1, C3, RESNET50_STACKS

# what cn_conv_wgrad_grouped_plan reports per job, in its order
FIELDS = ("tile", "stages", "slices", "rows", "tiles_x", "tiles_y", "first_wg", "wgs", "launch", "ws_floats")
# (filter rows, output channels, reduction rows per stage) of the tiles, by cn_conv_tune code
TILE = {0: (128, 128, 16), 4: (128, 96, 16), 2: (64, 64, 32), 3: (128, 32, 32), 5: (256, 64, 16)}


def trunk_jobs(n, res=256):
    """[(layer name, geometry)] of the 52 filter gradients ResNetTrunkFn.backward leaves to the end of its pass, in the order it
    records them: the blocks from the last to the first, in each its third, second and first convolution, then its shortcut (conv1,
    on the 3-channel image, is not the grouped kernel's).  The trunk's input is (n, res, res, 3)."""
    hw = res // 4                  # after conv1 (stride 2) and the 3x3 / 2 max pool
    cin = 64
    fwd = []
    for si, (f, blocks, stride1) in enumerate(RESNET50_STACKS):
        for bi in range(blocks):
            name = "conv%d_block%d" % (si + 2, bi + 1)
            s = stride1 if bi == 0 else 1
            out = hw // s
            block = [(name + "_3", C1[1].geom((n, out, out, f), 4 * f)), (name + "_2", C3.geom((n, out, out, f), f)),
                     (name + "_1", C1[s].geom((n, hw, hw, cin), f))]
            if bi == 0:
                block.append((name + "_0", C1[s].geom((n, hw, hw, cin), 4 * f)))
            fwd.append(block)
            hw, cin = out, 4 * f
    return [job for block in reversed(fwd) for job in block]


def plan(geoms, solo=False):
    """([{field: value} per job], (launches, jobs a launch holds, bytes of a launch's arguments, bytes an argument block holds))"""
    jobs, info = ops.conv_wgrad_grouped_plan(geoms, solo)
    return [dict(zip(FIELDS, j)) for j in jobs], info


def rows_of(g):
    return g.n * g.out_d * g.out_h * g.out_w


def ktot(g):
    return g.k_d * g.k_h * g.k_w * g.cin


# The lists of the GPU test: [(case in the form of tests/wgrad_edge_cases.py -- x shape, kernel, cout, stride, up, explicit pad --,
# accumulate)].  What the grouped plan makes of them is pinned in tests/test_wgrad_grouped_plan_cpu.py.
_TINY = [((1, 4, 4, 64), (1, 1), 64, 1, 0, None), ((2, 4, 4, 64), (1, 1), 64, 1, 0, None), ((1, 8, 8, 64), (1, 1), 64, 2, 0, None)]
LISTS = {
    # a 1x1 job, a 3x3 job with Ktot = 144 (128 + 16) and cout = 96, the stride-2 1x1 shortcut, a long job (M = 1440) that takes
    # many slices next to jobs with one, a job of 32 output channels (the 128 x 32 tile: a second configuration, a second launch),
    # a job of one short K step (M = 16); accumulate 0 and 1
    "mixed": [(((2, 8, 8, 64), (1, 1), 96, 1, 0, None), 0), (((2, 8, 8, 16), (3, 3), 96, 1, 0, None), 1),
              (((2, 8, 8, 64), (1, 1), 128, 2, 0, None), 0), (((3, 24, 20, 16), (3, 3), 100, 1, 0, None), 1),
              (((2, 8, 8, 32), (3, 3), 16, 1, 0, None), 0), (((1, 4, 4, 64), (1, 1), 64, 1, 0, None), 1)],
    # two jobs of equal work on one tile: each gets half a launch, fewer than 8 slices each would not fill it -- and M = 1440 is no
    # multiple of the slice: the XCD-round order with padded ids inside the grid, in front of another job's workgroups
    "two-long": [(((3, 24, 20, 16), (3, 3), 100, 1, 0, None), 0), (((3, 24, 20, 16), (3, 3), 100, 1, 0, None), 1)],
    # ONE launch with every way a job can lie in it: 15 slices (the XCD-round order, padded to 16: ids that return early in front
    # of the next job's workgroups), 8 slices (the XCD-round order, unpadded), 6 slices (the plain order), single slices
    "shares": [(((3, 24, 20, 16), (3, 3), 100, 1, 0, None), 1), (((2, 8, 8, 32), (3, 3), 128, 1, 0, None), 0),
               (((2, 16, 16, 16), (3, 3), 128, 1, 0, None), 0), (((1, 4, 4, 128), (1, 1), 128, 1, 0, None), 1),
               (((6, 8, 8, 32), (3, 3), 128, 1, 0, None), 1)],
    # more jobs than a launch holds
    "thirty": [(_TINY[k % 3], k % 2) for k in range(30)],
    "one": [(((2, 8, 8, 16), (3, 3), 96, 1, 0, None), 0)],
}
