"""GPU parity of the raw HIP ops (through the C ABI) against the CPU oracle (float64)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_ops as O


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda().contiguous()


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def close(got, ref, tol=2e-4, what=""):
    got = got.detach().cpu().double().numpy()
    ref = ref.detach().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    assert err <= tol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


CONV_CASES = [
    # (x shape, kernel, cout, stride, up, explicit_pad, act, slope)
    ((2, 16, 16, 64), (4, 4), 32, 1, 1, None, 1, 0.3),        # k4 + folded upsample, 128x32 tile
    ((2, 16, 16, 512), (4, 4), 256, 1, 0, None, 1, 0.3),      # map_2d_0
    ((2, 4, 4, 4, 512), (3, 3, 3), 256, 1, 1, None, 1, 0.3),  # map_3d_0 with folded upsample
    ((1, 8, 8, 8, 64), (3, 3, 3), 64, 1, 0, None, 1, 0.3),    # map_3d_post
    ((3, 16, 16, 1024), (1, 1), 512, 1, 0, None, 1, 0.2),     # projection conv
    ((2, 64, 64, 3), (3, 3), 48, 2, 0, None, 0, 0.0),         # D block 0 (scalar gather, stride 2)
    ((2, 37, 45, 3), (3, 3), 48, 2, 0, None, 0, 0.0),         # D block 0, odd extents (other SAME padding split)
    ((1, 100, 70, 3), (3, 3), 48, 2, 0, None, 0, 0.0),        # D block 0, extents that do not fill the 8x32 tiles
    ((2, 32, 32, 48), (3, 3), 96, 2, 0, None, 0, 0.0),        # D block 1
    ((2, 17, 13, 48), (3, 3), 96, 2, 0, None, 0, 0.0),        # ragged odd extents
    ((2, 32, 32, 3), (3, 3), 64, 1, 0, None, 2, 0.0),         # VGG conv1_1 + relu
    ((1, 9, 150, 3), (3, 3), 64, 1, 0, None, 0, 0.0),         # K = 27 filter gradient: three 64-pixel tiles per row, the last ragged
    ((1, 11, 301, 3), (3, 3), 20, 2, 0, None, 0, 0.0),        # ... stride 2, 151 outputs per row, cout below one column block
    ((1, 64, 64, 3), (7, 7), 64, 2, 0, 3, 0, 0.0),            # ResNet conv1 (pad 3, valid)
    ((2, 37, 45, 3), (7, 7), 64, 2, 0, 3, 2, 0.0),            # ... odd extents that do not fill the 8x32 tiles, two images, relu
    ((1, 70, 130, 3), (7, 7), 24, 2, 0, 3, 0, 0.0),           # ... one column block, a second (ragged) tile column
    ((2, 32, 32, 32), (4, 4), 3, 1, 1, None, 3, 0.0),         # map_final: thin cout + tanh + upsample
    ((1, 20, 13, 32), (4, 4), 3, 1, 1, None, 3, 0.0),         # map_final, extents that do not fill the 8x16 tiles
    ((2, 32, 32, 3), (1, 1), 3, 1, 0, None, 0, 0.0),          # from-RGB 1x1
    ((1, 5, 7, 3), (1, 1), 3, 1, 0, None, 1, 0.3),            # from-RGB 1x1, pixel count not a multiple of 4
    ((4, 8, 8, 256), (3, 3), 512, 1, 0, None, 2, 0.0),        # VGG block4 shape, 64x64 tiles
    ((1, 8, 8, 128), (1, 1), 512, 2, 0, None, 0, 0.0),        # ResNet strided 1x1
    ((2, 9, 7, 64), (1, 1), 36, 1, 0, None, 2, 0.0),          # 1x1 stride 1 (plain-GEMM kernel): 126 rows, 36 columns, bias + relu
    ((2, 16, 16, 512), (1, 1), 128, 1, 0, None, 2, 0.0),      # ... with a K split
]


def _oracle_conv(x, w, b, stride, up, explicit_pad, act, slope):
    if up:
        x = O.upsample2(x)
    if explicit_pad is not None:
        y = O.conv_valid_padded(x, w, b, stride, explicit_pad)
    else:
        y = O.conv_same(x, w, b, stride=stride)
    if act == 1:
        y = O.leaky_relu(y, slope)
    elif act == 2:
        y = torch.relu(y)
    elif act == 3:
        y = torch.tanh(y)
    return y


LOOP_VARIANTS = [(16, 3, 0), (16, 4, 0), (16, 3, 1), (16, 4, 2), (32, 3, 0)]     # (stage depth, stages, loader waves)


@pytest.mark.parametrize("shape", [((2, 16, 16, 64), (3, 3), 128, 1), ((1, 32, 32, 96), (3, 3), 192, 2), ((3, 8, 8, 256), (1, 1), 512, 1),
                                   ((1, 8, 8, 8, 64), (3, 3, 3), 64, 1)], ids=["k3", "k3s2", "1x1", "3d"])
def test_every_variant_of_the_lds_dma_loop_gives_the_same_bits(shape):
    """cn_conv_loop_select: the LDS-DMA main loop (fwd2.hip) with 16- / 32-deep stages, three / four stages and 0 / 1 / 2 loader
    waves walks the reduction in the same order, so an unsplit launch must give the SAME BITS in every variant -- forward and data
    gradient (the default rule picks one of them per launch size: small launches of the test suite would otherwise never run the
    variants the full-size layers use), and agree with the float64 oracle."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    xs, k, cout, stride = shape
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(xs, device="cuda", generator=gen)
    w = torch.randn(tuple(k) + (xs[-1], cout), device="cuda", generator=gen) * 0.05
    b = torch.randn(cout, device="cuda", generator=gen)
    g = ops.ConvSpec(k, stride=stride).geom(xs, cout)
    gy = torch.randn(ops.geom_out_shape(g), device="cuda", generator=gen)
    ref = _oracle_conv(x.cpu().double(), w.cpu().double(), b.cpu().double(), stride, 0, None, 1, 0.3)
    outs = {}
    try:
        ops.check(lib.cn_conv_tune(2, 1, 0), "cn_conv_tune")               # 64 x 64 tile (the one every variant exists for), unsplit
        for kb, ns, np_ in LOOP_VARIANTS:
            ops.check(lib.cn_conv_loop_select(1, kb, ns, np_), "cn_conv_loop_select")
            outs[(kb, ns, np_)] = (ops.conv_fwd(x, w, b, g, 1, 0.3).clone(), ops.conv_dgrad(gy, w, g).clone())
    finally:
        ops.check(lib.cn_conv_loop_select(-1, 0, 0, -1), "cn_conv_loop_select")
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
    torch.cuda.synchronize()
    y0, d0 = outs[LOOP_VARIANTS[0]]
    assert float((y0.cpu().double() - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    for v, (y, d) in outs.items():
        assert torch.equal(y, y0), ("forward", v)
        assert torch.equal(d, d0), ("data gradient", v)


@pytest.mark.parametrize("case", CONV_CASES, ids=[str(i) for i in range(len(CONV_CASES))])
def test_conv_fwd_dgrad_wgrad(case):
    from confignet_amd import ops
    xs, k, cout, stride, up, epad, act, slope = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    cin = xs[-1]
    x = rng.normal(size=xs)
    w = rng.normal(size=(*k, cin, cout)) / math.sqrt(np.prod(k) * cin)
    b = rng.normal(size=cout)
    spec = ops.ConvSpec(k, stride=stride, up=up, explicit_pad=epad)
    g = spec.geom(xs, cout)
    y = ops.conv_fwd(dev(x), dev(w), dev(b), g, act, slope)
    xr = t64(x).requires_grad_(True)
    wr = t64(w).requires_grad_(True)
    # reference on the upsampled tensor so dgrad can be compared at the upsampled extent
    xu = O.upsample2(xr) if up else xr
    xu.retain_grad()
    yr = _oracle_conv(xu, wr, t64(b), stride, 0, epad, act, slope)
    close(y, yr, what="fwd")
    # backward of the pre-activation (act none) for dgrad / wgrad
    yr0 = _oracle_conv(xu, wr, None, stride, 0, epad, 0, 0.0)
    gy = rng.normal(size=tuple(yr0.shape))
    (yr0 * t64(gy)).sum().backward()
    gu = ops.conv_dgrad(dev(gy), dev(w), g)
    close(gu, xu.grad, what="dgrad")
    if up:
        close(ops.sumpool2(gu), xr.grad, what="sumpool2(dgrad)")
    gw = ops.conv_wgrad(dev(x), dev(gy), g, tuple(w.shape))
    close(gw, wr.grad, tol=5e-4, what="wgrad")


PLANNED_LAUNCH_CASES = [
    # (x shape, kernel, cout, stride, up, explicit_pad, data gradient?): one per route of csrc/conv_dispatch.hip's plan
    ((1, 32, 32, 3), (3, 3), 48, 2, 0, None, False),          # 3x3 first layer
    ((1, 64, 64, 3), (7, 7), 64, 2, 0, 3, False),             # 7x7 stride-2 first layer
    ((1, 16, 16, 32), (4, 4), 3, 1, 1, None, False),          # map_final
    ((1, 32, 32, 3), (3, 3), 48, 2, 0, None, True),           # data gradient of the first case, into the image
    ((1, 16, 16, 8), (3, 3), 1, 1, 0, None, False),           # thin output: a launch without a profile bracket
    ((2, 16, 16, 64), (3, 3), 128, 1, 0, None, False),        # LDS-DMA loop
    ((2, 128, 128, 48), (3, 3), 96, 1, 0, None, False),       # ... 96 output channels
    ((1, 32, 32, 32), (3, 3), 32, 1, 0, None, False),         # ... 32 output channels
    ((1, 16, 16, 24), (3, 3), 64, 1, 0, None, False),         # cin % 16 != 0: the register-staged loop, scalar gather
    ((1, 8, 8, 512), (3, 3), 512, 1, 0, None, False),         # 16 K slices
]


@pytest.mark.parametrize("case", PLANNED_LAUNCH_CASES, ids=[str(i) for i in range(len(PLANNED_LAUNCH_CASES))])
def test_the_launch_is_the_one_the_plan_names(case):
    """cn_conv_fwd_plan says which launch a request gets; with profiling on, cn_conv_fwd / cn_conv_dgrad must then show exactly one
    launch, in the family the plan names (none where the plan's launch has no profile bracket) -- and compute the convolution."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    xs, k, cout, stride, up, epad, dgrad = case
    rng = np.random.default_rng(7 + cout + xs[-1])
    cin = xs[-1]
    x = rng.normal(size=xs)
    w = rng.normal(size=(*k, cin, cout)) / math.sqrt(np.prod(k) * cin)
    b = rng.normal(size=cout)
    g = ops.ConvSpec(k, stride=stride, up=up, explicit_pad=epad).geom(xs, cout)
    out = (ctypes.c_int * 8)()
    if dgrad:
        d = ops._copy_geom(g, in_d=g.out_d, in_h=g.out_h, in_w=g.out_w, cin=g.cout, out_d=1, out_h=g.in_h, out_w=g.in_w, cout=g.cin,
                           s_h=1, s_w=1, dl_h=g.s_h, dl_w=g.s_w, p_h=g.k_h - 1 - g.p_h, p_w=g.k_w - 1 - g.p_w)
        ops.check(lib.cn_conv_fwd_plan(ctypes.byref(d), 0, 0, 0, 0, 0, 0, 0, ctypes.byref(out)), "cn_conv_fwd_plan")
        xr = t64(x).requires_grad_(True)
        yr = _oracle_conv(xr, t64(w), None, stride, 0, epad, 0, 0.0)
        gy = rng.normal(size=tuple(yr.shape))
        (yr * t64(gy)).sum().backward()
        ref = xr.grad
        gyd, wt = dev(gy), ops.weight_tflip(dev(w))
        y = torch.empty(xs, device="cuda", dtype=torch.float32)
        call = lambda: lib.cn_conv_dgrad(ctypes.byref(g), ops._ptr(gyd), ops._ptr(wt), ops._ptr(y), ops._stream())
    else:
        ops.check(lib.cn_conv_fwd_plan(ctypes.byref(g), 0, 1, 1, 0, 0, 0, 0, ctypes.byref(out)), "cn_conv_fwd_plan")
        ref = _oracle_conv(t64(x), t64(w), t64(b), stride, up, epad, 1, 0.3)
        xd, wd, bd = dev(x), dev(w), dev(b)
        y = torch.empty(ops.geom_out_shape(g), device="cuda", dtype=torch.float32)
        call = lambda: lib.cn_conv_fwd(ctypes.byref(g), ops._ptr(xd), ops._ptr(wd), ops._ptr(bd), ops._ptr(y), 1, 0.3, ops._stream())
    family = out[4]
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        ops.check(call(), "convolution")
        torch.cuda.synchronize()
        shown = ops.prof_collect_by_family()
    finally:
        ops.prof_enable(False)
    print("plan", list(out), "profile", {name: v["launches"] for name, v in shown.items()})
    want = {} if family < 0 else {ops.PROF_FAMILIES[family]: 1}
    assert {name: v["launches"] for name, v in shown.items()} == want, (list(out), shown)
    close(y, ref, what="planned launch")


# The layer shapes of the 256x256, batch-16 iteration (BASELINE.json configs[1]): the tile / split-K / XCD-order / Winograd
# code paths are selected BY SIZE, so the small cases above never reach them.  Each layer is compared with the float64
# oracle on the FULL tensors (forward, data gradient, filter gradient: seconds per layer on the host), and -- second line of
# defence, size-independent -- the three kernels are checked against each other through the adjoint identities
#   <conv(x, w), gy> == <x_up, dgrad(gy, w)> == <w, wgrad(x, gy)>
# and through linearity in x, with the inner products accumulated in float64 on the device.
FULL_SIZE_LAYERS = [
    # (x shape, kernel, cout, stride, up)
    ((16, 256, 256, 3), (3, 3), 48, 2, 0),        # DiscrBlock 0: c3_fwd, s2_image_dgrad, K = 27 wgrad
    ((16, 128, 128, 48), (3, 3), 96, 2, 0),       # DiscrBlock 1: 128 x 96 tiles, parity-ordered dgrad
    ((16, 64, 64, 96), (3, 3), 192, 2, 0),        # DiscrBlock 2
    ((16, 16, 16, 384), (3, 3), 768, 2, 0),       # DiscrBlock 4: split-K forward and dgrad
    ((8, 8, 8, 8, 512), (3, 3, 3), 256, 1, 1),    # generator Conv3D 8^3 -> 16^3 with folded upsample
    ((8, 64, 64, 64), (4, 4), 32, 1, 1),          # generator k4 + upsample to 128^2
    ((8, 128, 128, 32), (4, 4), 3, 1, 1),         # map_final: thin cout
    ((16, 256, 256, 64), (3, 3), 64, 1, 0),       # VGG block1_conv2
    ((16, 64, 64, 256), (3, 3), 256, 1, 0),       # VGG block3
    ((8, 16, 16, 1024), (1, 1), 512, 1, 0),       # generator projection conv / ResNet 1x1
    ((16, 128, 128, 128), (3, 3), 128, 1, 0),     # VGG block2_conv2 (Winograd)
    ((8, 32, 32, 512), (3, 3), 512, 1, 0),        # VGG block4_conv2 (Winograd, cin = 512)
    ((16, 32, 32, 192), (3, 3), 384, 2, 0),       # DiscrBlock 3: 64 x 64 tiles, few rows
    ((96, 16, 16, 384), (3, 3), 768, 2, 0),       # DiscrBlock 4 under the batched R1 sweep (6 heads x 16 samples)
    ((8, 16, 16, 16, 256), (3, 3, 3), 128, 1, 1),  # generator Conv3D 16^3 -> 32^3 with folded upsample
    ((8, 32, 32, 256), (4, 4), 64, 1, 1),         # generator k4 + upsample to 64^2
    ((8, 256, 256, 3), (3, 3), 64, 1, 0),         # VGG block1_conv1: c3_fwd, s1_image_dgrad, thin filter gradient
    ((8, 64, 64, 256), (1, 1), 128, 2, 0),        # ResNet-50 conv3_block1_1 (1x1, stride 2): three of the four parity classes of its data gradient have no live tap
]


@pytest.mark.gpu
def test_data_gradient_tiles_without_a_live_tap_under_concurrency():
    """Regression (round 4): the parity-ordered data gradient of a 1x1 stride-2 convolution has whole workgroup tiles with NO K
    step (their parity class has no tap); such a workgroup went from filling its row map in LDS straight to the epilogue that
    reads entries written by other waves, without a barrier.  A wave that ran ahead stored its zero rows through stale LDS contents
    -- seen only when the step graphs were scheduled differently (other kernels resident on the CU, floats left in LDS): a memory
    fault in ResNet-50's first strided block.  Here: that launch many times next to launches on a second stream that leave float
    tiles in LDS; every result must equal the float64 reference (and be exactly zero at the positions no tap reaches)."""
    from confignet_amd import ops
    rng = np.random.default_rng(5)
    xs, cout = (8, 64, 64, 256), 128
    g = ops.ConvSpec((1, 1), stride=2).geom(xs, cout)
    w = dev(rng.normal(size=(1, 1, 256, cout)) / 16.0)
    gy = dev(rng.normal(size=ops.geom_out_shape(g)))
    ref = torch.zeros(xs, dtype=torch.float64)
    ref[:, ::2, ::2, :] = torch.einsum("nhwo,co->nhwc", gy.cpu().double(), w.cpu().double()[0, 0])
    g2 = ops.ConvSpec((3, 3)).geom((8, 32, 32, 128), 256)
    x2, w2 = dev(rng.normal(size=(8, 32, 32, 128))), dev(rng.normal(size=(3, 3, 128, 256)))
    from confignet_amd.graphs import independent_streams
    sa, sb = independent_streams(2)      # (two streams that provably run side by side: HIP streams share a few hardware queues)
    torch.cuda.synchronize()
    outs = []
    for _ in range(25):
        with torch.cuda.stream(sb):
            for _ in range(4):
                ops.conv_fwd(x2, w2, None, g2)
        with torch.cuda.stream(sa):
            outs += [ops.conv_dgrad(gy, w, g) for _ in range(4)]
    torch.cuda.synchronize()
    dead = torch.ones(64, 64, dtype=torch.bool)
    dead[::2, ::2] = False
    for o in outs:
        assert not bool(o[:, dead.to(o.device)].any()), "rows that no tap reaches must be exactly zero"
        close(o, ref, tol=2e-4, what="1x1 stride-2 data gradient")


@pytest.mark.gpu
def test_filter_gradient_kernel_under_lds_contention():
    """Regression (round 4): wgrad2_kernel<128x128> read its MFMA operands through inline-asm ds_reads whose hand-placed wait had
    tied ("+v") operands; the register allocator turned two of them into v_mov copies IN FRONT of the wait, which read the
    ds_read's destination before the data had landed.  Right in isolation (LDS answers within the ~100 cycles in between), wrong
    when another kernel's workgroups load the CU's LDS: tile-shaped errors of a few per cent in ~2 % of the launches of the
    generator's Conv3D filter gradients, NaN when the stale register held one -- the pipelined training loop went non-finite in
    about half of the 60-iteration runs.  Here: that filter gradient (no row split: 4^3 grid) next to forward convolutions on a
    second stream, every launch against its own serial result.  (The static check of the compiled loop: tests/test_abi_cpu.py.)"""
    from confignet_amd import ops
    torch.manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda") * 0.05
    g = ops.ConvSpec((3, 3, 3), up=1).geom((8, 4, 4, 4, 512), 256)
    _, wd, _, g2 = ops.upfold_prepare(r(3, 3, 3, 512, 256), g)
    x, gy = r(8, 4, 4, 4, 512), r(*ops.geom_out_shape(g))
    ga = ops.ConvSpec((3, 3)).geom((8, 64, 64, 64), 256)
    xa, wa = r(8, 64, 64, 64), r(3, 3, 64, 256)
    old, ops.WINOGRAD = ops.WINOGRAD, False
    try:
        ref = ops.conv_wgrad(gy, x, g2, tuple(wd.shape)).clone()
        torch.cuda.synchronize()
        scale = float(ref.abs().max())
        from confignet_amd.graphs import independent_streams
        sa, sb = independent_streams(2)  # (two streams that provably run side by side: HIP streams share a few hardware queues)
        worst = 0.0
        for _ in range(200):
            with torch.cuda.stream(sb):
                for _ in range(3):
                    ops.conv_fwd(xa, wa, None, ga)
            with torch.cuda.stream(sa):
                outs = [ops.conv_wgrad(gy, x, g2, tuple(wd.shape)) for _ in range(2)]
            torch.cuda.synchronize()
            worst = max(worst, max(float((o - ref).abs().max()) for o in outs))
    finally:
        ops.WINOGRAD = old
    assert worst <= 1e-5 * scale, "filter gradient differs from its serial result under contention: %.3e of %.3e" % (worst, scale)


@pytest.mark.gpu
def test_convolution_kernels_next_to_each_other_match_their_serial_results():
    """Every hand-scheduled kernel family of the path (LDS-DMA stages, inline-asm operand reads, hand-counted waits, bare barriers)
    as a victim on one stream while a mix of the others runs on a second stream: each launch must reproduce its own serial
    result -- bit for bit where the launch has no atomics, to 1e-5 of the result's scale where it splits K.  Isolated launches
    cannot see a wait that is only too short when LDS or the memory path is contended (round 4: wgrad2_kernel, igemm_fwd_kernel's
    row map); the training loop can, but does not say which kernel."""
    from confignet_amd import ops
    torch.manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda") * 0.05

    def fwd(xs, k, cout, stride=1, up=0):
        g = ops.ConvSpec(k, stride=stride, up=up).geom(xs, cout)
        x, w, b = r(*xs), r(*k, xs[-1], cout), r(cout)
        return lambda: ops.conv_fwd(x, w, b, g, 1, 0.2)

    def dgrad(xs, k, cout, stride=1):
        g = ops.ConvSpec(k, stride=stride).geom(xs, cout)
        gy, w = r(*ops.geom_out_shape(g)), r(*k, xs[-1], cout)
        return lambda: ops.conv_dgrad(gy, w, g)

    def wgrad(xs, k, cout, stride=1):
        g = ops.ConvSpec(k, stride=stride).geom(xs, cout)
        x, gy = r(*xs), r(*ops.geom_out_shape(g))
        return lambda: ops.conv_wgrad(x, gy, g, (*k, xs[-1], cout))

    victims = {
        "F(4x4) forward, VGG conv3": fwd((8, 64, 64, 256), (3, 3), 256),
        "F(4x4) forward, VGG conv1_2": fwd((4, 256, 256, 64), (3, 3), 64),
        "F(2x2) forward, VGG conv4": fwd((8, 32, 32, 512), (3, 3), 512),
        "F(2x2) data gradient": dgrad((8, 32, 32, 256), (3, 3), 512),
        "plain-GEMM loop 64x64, gathered": fwd((8, 16, 16, 256), (3, 3), 256),
        "plain-GEMM loop 1x1": fwd((8, 32, 32, 512), (1, 1), 128),
        "parity-ordered data gradient": dgrad((8, 64, 64, 96), (3, 3), 192, stride=2),
        "1x1 stride-2 data gradient": dgrad((8, 64, 64, 256), (1, 1), 128, stride=2),
        "Conv3D forward with folded upsample": fwd((8, 8, 8, 8, 256), (3, 3, 3), 128, up=1),
        "wgrad2 128x128": wgrad((8, 16, 16, 256), (3, 3), 256),
        "wgrad2 128x96": wgrad((8, 32, 32, 96), (3, 3), 192, stride=2),
        "wgrad2 64x64": wgrad((8, 16, 16, 128), (1, 1), 64),
        "igemm_wgrad (long reduction)": wgrad((16, 128, 128, 48), (3, 3), 96, stride=2),
    }

    def class_filter_wgrad(n, d, cin, cout):               # the generator's Conv3D + folded upsample: 4^3-tap class filters
        g = ops.ConvSpec((3, 3, 3), up=1).geom((n, d, d, d, cin), cout)
        _, wd, _, g2 = ops.upfold_prepare(r(3, 3, 3, cin, cout), g)
        x, gy = r(n, d, d, d, cin), r(*ops.geom_out_shape(g))
        return lambda: ops.conv_wgrad(gy, x, g2, tuple(wd.shape))
    victims["wgrad2 128x128, one row slice (Conv3D 4^3 class filters)"] = class_filter_wgrad(8, 4, 512, 256)
    victims["wgrad2 128x128, row splits (Conv3D 8^3 class filters)"] = class_filter_wgrad(8, 8, 256, 128)
    aggressors = [fwd((8, 64, 64, 64), (3, 3), 256), wgrad((8, 16, 16, 256), (3, 3), 256), fwd((8, 32, 32, 256), (1, 1), 1024),
                  dgrad((8, 64, 64, 96), (3, 3), 192, stride=2)]
    from confignet_amd.graphs import independent_streams
    sa, sb = independent_streams(2)      # (two streams that provably run side by side: HIP streams share a few hardware queues)
    from confignet_amd._lib import lib
    for name, v in victims.items():
        refs = [v() for _ in range(3)]
        torch.cuda.synchronize()
        exact = torch.equal(refs[0], refs[1]) and torch.equal(refs[0], refs[2])      # (no atomics in this launch)
        if exact and "wgrad" not in name:
            # three equal serial results do not prove it for a forward / data-gradient launch: a K split of two or three slices adds
            # its atomics in the same order whenever nothing else runs (round 5: a 3-way split passed this probe and then differed
            # by one ulp next to the aggressors).  Unsplit is what it says only if the forced-unsplit launch gives the same bits.
            ops.check(lib.cn_conv_tune(-1, 1, 0), "cn_conv_tune")
            exact = torch.equal(refs[0], v())
            ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")
        ref, scale = refs[0].clone(), float(refs[0].abs().max())
        del refs
        worst = 0.0
        for _ in range(40):
            with torch.cuda.stream(sb):
                for a in aggressors:
                    a()
            with torch.cuda.stream(sa):
                outs = [v() for _ in range(3)]
            torch.cuda.synchronize()
            for o in outs:
                assert bool(torch.isfinite(o).all()), name
                worst = max(worst, float((o - ref).abs().max()))
        assert worst <= (0.0 if exact else 1e-5 * scale), "%s: differs from its serial result by %.3e (scale %.3e, %s)" % (
            name, worst, scale, "no atomics: must be bit-identical" if exact else "split launch")
        if not exact and "wgrad" not in name:
            # the same main loop without its K split (one workgroup walks the whole reduction): no atomics, so bit for bit
            ops.check(lib.cn_conv_tune(-1, 1, 0), "cn_conv_tune")
            try:
                ref1 = v().clone()
                torch.cuda.synchronize()
                for _ in range(20):
                    with torch.cuda.stream(sb):
                        for a in aggressors:
                            a()
                    with torch.cuda.stream(sa):
                        outs = [v() for _ in range(3)]
                    torch.cuda.synchronize()
                    for o in outs:
                        assert torch.equal(o, ref1), "%s, unsplit: differs from its serial result by %.3e" % (name, float((o - ref1).abs().max()))
            finally:
                ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")


def _full_size_oracle(xs, k, cout, stride, up, x, w, gy):
    """float64 forward / data gradient (at the upsampled extent) / filter gradient of one layer on the host."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    xr, wr = x.detach().cpu().double().requires_grad_(True), w.detach().cpu().double().requires_grad_(True)
    xu = O.upsample2(xr) if up else xr
    xu.retain_grad()
    yr = O.conv_same(xu, wr, None, stride=stride)
    (yr * gy.detach().cpu().double()).sum().backward()
    return yr.detach(), xu.grad, wr.grad


@pytest.mark.parametrize("case", FULL_SIZE_LAYERS, ids=[str(i) for i in range(len(FULL_SIZE_LAYERS))])
def test_conv_full_size_vs_oracle(case):
    """building_blocks.py:29,65,91, perceptual_loss.py:19-26 at the sizes of configs[1]: every output element of the three
    kernels against the float64 oracle (a shifted SAME padding, a mis-ordered parity class or a wrong tile-boundary row
    passes the adjoint identities below as long as it is consistent; it does not pass this)."""
    from confignet_amd import ops
    xs, k, cout, stride, up = case
    gen = torch.Generator(device="cuda").manual_seed(sum(xs) + 7 * cout)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    cin = xs[-1]
    x = rnd(*xs)
    w = rnd(*k, cin, cout) / math.sqrt(np.prod(k) * cin)
    g = ops.ConvSpec(k, stride=stride, up=up).geom(xs, cout)
    y = ops.conv_fwd(x, w, None, g, 0, 0.0)
    gy = rnd(*y.shape)
    gu = ops.conv_dgrad(gy, w, g)
    gw = ops.conv_wgrad(x, gy, g, tuple(w.shape))
    yr, gur, gwr = _full_size_oracle(xs, k, cout, stride, up, x, w, gy)
    close(y, yr, what="fwd")
    close(gu, gur, what="dgrad")
    close(gw, gwr, tol=5e-4, what="wgrad")


SWEEP_LAYERS = [
    # (x shape, kernel, cout, stride): every tile configuration / split-K factor the heuristic can pick, forced one by one
    ((4, 64, 64, 96), (3, 3), 192, 2),
    ((4, 32, 32, 128), (3, 3), 128, 1),
    ((2, 30, 30, 64), (1, 1), 144, 1),            # 1x1 stride 1: the plain-GEMM kernel (gemm1x1.hip), rows and columns that fill no tile
    ((8, 16, 16, 256), (1, 1), 64, 1),            # ... ResNet bottleneck reduce
]


@pytest.mark.parametrize("case", SWEEP_LAYERS, ids=[str(i) for i in range(len(SWEEP_LAYERS))])
def test_conv_forced_tile_and_split_configurations_vs_oracle(case, monkeypatch):
    """cn_conv_tune sweep: tiles 128x128 / 128x64 / 64x64 / 128x32 / 128x96, split-K 1 / 3 / 8, forward and parity-ordered
    data gradient, every filter-gradient tile (256x64 included) and the filter-gradient workgroup targets -- each against the
    float64 oracle (Winograd off: the direct kernels are what is being configured)."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    monkeypatch.setattr(ops, "WINOGRAD", False)
    xs, k, cout, stride = case
    gen = torch.Generator(device="cuda").manual_seed(11 + cout)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    x = rnd(*xs)
    w = rnd(*k, xs[-1], cout) / math.sqrt(np.prod(k) * xs[-1])
    g = ops.ConvSpec(k, stride=stride).geom(xs, cout)
    y0 = ops.conv_fwd(x, w, None, g, 0, 0.0)
    gy = rnd(*y0.shape)
    yr, gur, gwr = _full_size_oracle(xs, k, cout, stride, 0, x, w, gy)
    try:
        for cfg in (0, 1, 2, 3, 4, 5):
            # the filter gradient reads the same hook: 0 / 4 / 2 / 3 / 5 -> its 128x128 / 128x96 / 64x64 / 128x32 / 256x64 tile (1: its
            # own choice), any of them on any cout.  5 exists for it alone: the forward plan has no such tile.
            ops.check(lib.cn_conv_tune(cfg, 0, 0), "cn_conv_tune")
            close(ops.conv_wgrad(x, gy, g, tuple(w.shape)), gwr, tol=5e-4, what="wgrad cfg %d" % cfg)
            if cfg == 5 or (cfg == 4 and cout % 96):
                continue
            for splits in (1, 3, 8):
                ops.check(lib.cn_conv_tune(cfg, splits, 0), "cn_conv_tune")
                close(ops.conv_fwd(x, w, None, g, 0, 0.0), yr, what="fwd cfg %d splits %d" % (cfg, splits))
                if cfg != 4 or xs[-1] % 96 == 0:
                    wt = ops.weight_tflip(w)
                    gu = torch.empty_like(x)
                    ops.check(lib.cn_conv_dgrad(__import__("ctypes").byref(g), ops._ptr(gy), ops._ptr(wt), ops._ptr(gu), ops._stream()), "cn_conv_dgrad")
                    close(gu, gur, what="dgrad cfg %d splits %d" % (cfg, splits))
                    close(ops.conv_dgrad(gy, w, g), gur, what="dgrad from the original filter, cfg %d splits %d" % (cfg, splits))
        for wg_blocks in (256, 1024, 4096):
            ops.check(lib.cn_conv_tune(-1, 0, wg_blocks), "cn_conv_tune")
            close(ops.conv_wgrad(x, gy, g, tuple(w.shape)), gwr, tol=5e-4, what="wgrad wg_blocks %d" % wg_blocks)
    finally:
        ops.check(lib.cn_conv_tune(-1, 0, 0), "cn_conv_tune")


@pytest.mark.parametrize("case", FULL_SIZE_LAYERS, ids=[str(i) for i in range(len(FULL_SIZE_LAYERS))])
def test_conv_adjoint_identities_full_size(case):
    from confignet_amd import ops
    xs, k, cout, stride, up = case
    gen = torch.Generator(device="cuda").manual_seed(sum(xs) + cout)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    cin = xs[-1]
    x, x2 = rnd(*xs), rnd(*xs)
    w = rnd(*k, cin, cout) / math.sqrt(np.prod(k) * cin)
    spec = ops.ConvSpec(k, stride=stride, up=up)
    g = spec.geom(xs, cout)
    y = ops.conv_fwd(x, w, None, g, 0, 0.0)
    gy = rnd(*y.shape)
    dot = lambda a, b: float((a.double() * b.double()).sum())
    lhs = dot(y, gy)
    gu = ops.conv_dgrad(gy, w, g)                    # gradient at the (upsampled) input extent
    gx = ops.sumpool2(gu) if up else gu
    gw = ops.conv_wgrad(x, gy, g, tuple(w.shape))
    scale = math.sqrt(dot(y, y) * dot(gy, gy))                         # Cauchy-Schwarz bound of the inner product
    assert abs(lhs - dot(x, gx)) <= 2e-5 * scale, ("dgrad adjoint", lhs, dot(x, gx), scale)
    assert abs(lhs - dot(w, gw)) <= 2e-5 * scale, ("wgrad adjoint", lhs, dot(w, gw), scale)
    y12 = ops.conv_fwd(x + 0.5 * x2, w, None, g, 0, 0.0)
    y2 = ops.conv_fwd(x2, w, None, g, 0, 0.0)
    err = float((y12 - (y + 0.5 * y2)).abs().max())
    assert err <= 2e-4 * max(1.0, float(y.abs().max())), ("linearity", err)


@pytest.mark.parametrize("m,n,k,ta,tb", [(16, 148, 32768, 0, 0), (16, 1, 32768, 0, 0), (8, 145, 145, 0, 0), (4096, 217, 145, 0, 0),
                                         (16, 32768, 148, 0, 1), (32768, 148, 16, 1, 0), (7, 5, 3, 1, 1), (130, 70, 33, 0, 1),
                                         (16, 3, 2048, 0, 0), (16, 1, 768, 0, 0), (5, 4, 129, 0, 0),
                                         # the small-layer kernels (round 3): row-skinny NN / NT at M <= 32, depth-skinny TN at K <= 32
                                         (16, 128, 145, 0, 0), (8, 512, 128, 0, 0), (16, 145, 128, 0, 1), (3, 70, 62, 0, 0), (32, 65, 256, 0, 1),
                                         (9, 30, 53, 0, 1), (1, 145, 145, 0, 0), (145, 128, 16, 1, 0), (62, 30, 8, 1, 0), (128, 512, 3, 1, 0)])
def test_gemm(m, n, k, ta, tb):
    from confignet_amd import ops
    rng = np.random.default_rng(m * 7 + n)
    a = rng.normal(size=(k, m) if ta else (m, k))
    b = rng.normal(size=(n, k) if tb else (k, n)) / math.sqrt(k)
    bias = rng.normal(size=n)
    ref = (t64(a).T if ta else t64(a)) @ (t64(b).T if tb else t64(b)) + t64(bias)
    close(ops.gemm(dev(a), dev(b), bool(ta), bool(tb), dev(bias)), ref, what="gemm")
    if k < 1000 or n <= 4:
        close(ops.gemm(dev(a), dev(b), bool(ta), bool(tb), dev(bias), act=1, slope=0.3), O.leaky_relu(ref, 0.3), what="gemm+lrelu")
    # C += op(A) op(B) (cn_gemm_acc: a Dense layer's weight gradient added into its gradient-arena slot)
    c0 = rng.normal(size=(m, n))
    out = dev(c0)
    ops.gemm_acc(dev(a), dev(b), out, bool(ta), bool(tb))
    close(out, t64(c0) + ref - t64(bias), what="gemm_acc")


@pytest.mark.parametrize("shape", [(2, 16, 16, 48), (3, 8, 8, 8, 128), (2, 128, 128, 32), (2, 5, 7, 3), (4, 1, 1, 2048),
                                   (2, 64, 64, 48), (3, 40, 24, 20), (5, 64, 64, 3)])
def test_nc_reduce_and_lin2(shape):
    from confignet_amd import ops
    rng = np.random.default_rng(sum(shape))
    x1, x2 = rng.normal(size=shape), rng.normal(size=shape)
    n, c = shape[0], shape[-1]
    axes = tuple(range(1, len(shape) - 1))
    s1, s2 = ops.nc_reduce(dev(x1), dev(x2))
    close(s1, t64(x1).sum(dim=axes), tol=1e-4, what="sum")
    close(s2, (t64(x1) * t64(x2)).sum(dim=axes), tol=1e-4, what="dot")
    s1, s2 = ops.nc_reduce(dev(x1), None, flags=1, slope=0.3)
    a = O.leaky_relu(t64(x1), 0.3)
    close(s1, a.sum(dim=axes), tol=1e-4, what="sum lrelu")
    close(s2, (a * a).sum(dim=axes), tol=1e-4, what="sumsq lrelu")
    s1, _ = ops.nc_reduce(dev(x1), None, want_dot=False, per_channel=True)
    close(s1, t64(x1).sum(dim=(0,) + axes).reshape(1, c), tol=1e-4, what="colsum")
    A1, A2, B = rng.normal(size=(n, c)), rng.normal(size=(n, c)), rng.normal(size=(n, c))
    bc = lambda v: t64(v).reshape(n, *([1] * len(axes)), c)
    y = ops.nc_lin2(shape, dev(x1), dev(A1), dev(x2), dev(A2), dev(B))
    close(y, bc(A1) * t64(x1) + bc(A2) * t64(x2) + bc(B), what="lin2")
    y = ops.nc_lin2(shape, dev(x1), dev(A1), dev(x2), dev(A2), dev(B), flags=2 | 4, slope=0.3)
    ref = (bc(A1) * t64(x1) + bc(A2) * O.leaky_relu(t64(x2), 0.3) + bc(B)) * torch.where(t64(x2) > 0, 1.0, 0.3)
    close(y, ref, what="lin2 flags")
    y = ops.nc_lin2(shape, dev(x1), dev(A1[0]), None, None, dev(B[0]), flags=8, per_channel=True)
    close(y, torch.relu(t64(A1[0]) * t64(x1) + t64(B[0])), what="lin2 per-channel relu")
    y = ops.nc_lin2(shape, None, None, None, None, dev(B))
    close(y, bc(B).expand(shape), what="lin2 broadcast")
    # per-channel sum + dot (long reductions are spread over partial rows and re-added)
    s1, s2 = ops.nc_reduce(dev(x1), dev(x2), per_channel=True)
    close(s1, t64(x1).sum(dim=(0,) + axes).reshape(1, c), tol=2e-4, what="colsum (pair)")
    close(s2, (t64(x1) * t64(x2)).sum(dim=(0,) + axes).reshape(1, c), tol=2e-4, what="coldot")
    # third coefficient pair (tangent pass of the DiscrBlock tail): masked sum + a3*x2 + b3
    A3, B3 = rng.normal(size=(n, c)), rng.normal(size=(n, c))
    y = ops.nc_lin2(shape, dev(x1), dev(A1), dev(x2), dev(A2), dev(B), flags=4, slope=0.3, a3=dev(A3), b3=dev(B3))
    ref = (bc(A1) * t64(x1) + bc(A2) * t64(x2) + bc(B)) * torch.where(t64(x2) > 0, 1.0, 0.3) + bc(A3) * t64(x2) + bc(B3)
    close(y, ref, what="lin2 a3/b3")


@pytest.mark.parametrize("shape", [(16, 128, 128, 48), (16, 256, 256, 64), (8, 16, 16, 16, 128), (16, 256, 256, 3)])
def test_elementwise_full_size_against_torch_float64(shape):
    """The statistics / affine / streaming kernels at the activation sizes of the 256x256 batch-16 iteration, against
    torch float64 arithmetic on the device (an independent implementation; the float64 CPU oracle covers small sizes)."""
    from confignet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(len(shape) + shape[-1])
    x1, x2 = torch.randn(*shape, device="cuda", generator=gen), torch.randn(*shape, device="cuda", generator=gen)
    n, c = shape[0], shape[-1]
    axes = tuple(range(1, len(shape) - 1))
    spatial = int(np.prod(shape[1:-1]))
    d1, d2 = x1.double(), x2.double()
    rel = lambda got, ref: float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1.0))
    s1, s2 = ops.nc_reduce(x1, x2, flags=2, slope=0.3)
    l2 = torch.where(d2 > 0, d2, 0.3 * d2)
    assert rel(s1, d1.sum(dim=axes)) < 1e-5 * math.sqrt(spatial) and rel(s2, (d1 * l2).sum(dim=axes)) < 1e-5 * math.sqrt(spatial)
    sc, sd = ops.nc_reduce(x1, x2, per_channel=True)
    assert rel(sc, d1.sum(dim=(0,) + axes).reshape(1, c)) < 1e-5 * math.sqrt(n * spatial)
    assert rel(sd, (d1 * d2).sum(dim=(0,) + axes).reshape(1, c)) < 1e-5 * math.sqrt(n * spatial)
    A1, A2, B = (torch.randn(n, c, device="cuda", generator=gen) for _ in range(3))
    bc = lambda v: v.double().reshape(n, *([1] * len(axes)), c)
    y = ops.nc_lin2(shape, x1, A1, x2, A2, B, flags=2 | 4, slope=0.3)
    ref = (bc(A1) * d1 + bc(A2) * l2 + bc(B)) * torch.where(d2 > 0, 1.0, 0.3)
    assert rel(y, ref) < 1e-5
    y = ops.nc_lin2(shape, x1, A1[0], x2, A2[0], B[0], flags=8, per_channel=True)
    assert rel(y, torch.relu(A1[0].double() * d1 + A2[0].double() * d2 + B[0].double())) < 1e-5
    out = ops.act_fwd(x1, 1, 0.3)
    assert rel(ops.act_bwd(x2, out, 1, 0.3), d2 * torch.where(d1 > 0, 1.0, 0.3)) < 1e-6
    assert rel(ops.axpby(x1, x2, 2.0, -0.5), 2 * d1 - 0.5 * d2) < 1e-6
    assert rel(ops.sqdiff_sum(x1, x2, 0.25), (0.25 * ((d1 - d2) ** 2).sum()).reshape(1)) < 1e-5
    assert rel(ops.row_sumsq(x1), (d1 ** 2).reshape(n, -1).sum(1)) < 1e-5
    s = torch.randn(n, device="cuda", generator=gen)
    assert rel(ops.row_scale(x1, s, 2.0), d1 * 2.0 * s.double().reshape(n, *([1] * (len(shape) - 1)))) < 1e-6


def test_adam_ema_full_arena():
    """Adam + EMA over an encoder-sized arena (23.6 M parameters): first step is lr_t * g / (|g| + eps) (a sign step),
    then the fp32 recurrences against float64 on the device for 3 more steps with the shared-counter lr_t."""
    from confignet_amd import ops
    n = 23_600_000
    gen = torch.Generator(device="cuda").manual_seed(7)
    theta = torch.randn(n, device="cuda", generator=gen)
    m, v, ema = torch.zeros_like(theta), torch.zeros_like(theta), theta.clone()
    t64_, m64, v64, e64 = theta.double(), m.double(), v.double(), ema.double()
    lr, b1, b2, eps = 4e-4, 0.0, 0.9, 1e-7
    for t in range(1, 5):
        g = torch.randn(n, device="cuda", generator=gen)
        lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        ops.adam_step(theta, g, m, v, None, torch.full((1,), lr_t, device="cuda"), b1, b2, eps)
        ops.ema_step(ema, theta, 0.999)
        g64 = g.double()
        m64 = b1 * m64 + (1 - b1) * g64
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        step = lr_t * m64 / (v64.sqrt() + eps)
        if t == 1:                                  # first step: |delta| = lr wherever |g| >> eps (R10)
            assert float(((step.abs() - lr).abs() * (g64.abs() > 1e-2)).max()) < 1e-4 * lr
        t64_ = t64_ - step
        e64 = 0.999 * e64 + 0.001 * t64_
    assert float((theta.double() - t64_).abs().max()) < 4e-6        # 4 steps x one fp32 ulp at |theta| ~ 5
    assert float((ema.double() - e64).abs().max()) < 4e-6


def test_elementwise_and_losses():
    from confignet_amd import ops
    rng = np.random.default_rng(5)
    x, y = rng.normal(size=(3, 9, 11, 5)), rng.normal(size=(3, 9, 11, 5))
    for act, f in [(1, lambda v: O.leaky_relu(v, 0.3)), (2, torch.relu), (3, torch.tanh)]:
        out = ops.act_fwd(dev(x), act, 0.3)
        close(out, f(t64(x)), what="act")
        xr = t64(x).requires_grad_(True)
        (f(xr) * t64(y)).sum().backward()
        close(ops.act_bwd(dev(y), out, act, 0.3), xr.grad, what="act_bwd")
        gx, gb = ops.act_bwd_bias(dev(y), out, act, 0.3)              # fused with the channel sums (bias gradient)
        close(gx, xr.grad, what="act_bwd_bias gx")
        close(gb, xr.grad.reshape(-1, 5).sum(0), tol=1e-4, what="act_bwd_bias gb")
    xl, yl = rng.normal(size=(2, 96, 96, 8)), rng.normal(size=(2, 96, 96, 8))      # >= 8192 rows: partial rows + final add
    ol = ops.act_fwd(dev(xl), 1, 0.3)
    gx, gb = ops.act_bwd_bias(dev(yl), ol, 1, 0.3)
    ref = t64(yl) * torch.where(t64(xl) > 0, 1.0, 0.3)
    close(gx, ref, what="act_bwd_bias gx (long)")
    close(gb, ref.reshape(-1, 8).sum(0), tol=1e-4, what="act_bwd_bias gb (long)")
    close(ops.axpby(dev(x), dev(y), 2.0, -0.5), 2 * t64(x) - 0.5 * t64(y))
    close(ops.mul(dev(x), dev(y)), t64(x) * t64(y))
    close(ops.sqdiff_sum(dev(x), dev(y), 0.25), (0.25 * ((t64(x) - t64(y)) ** 2).sum()).reshape(1), tol=1e-4)
    close(ops.row_sumsq(dev(x)), (t64(x) ** 2).reshape(3, -1).sum(1), tol=1e-4)
    s = rng.normal(size=3)
    close(ops.row_scale(dev(x), dev(s), 2.0), t64(x) * 2.0 * t64(s).reshape(3, 1, 1, 1))
    mask = (rng.uniform(size=(3, 9, 11)) > 0.5).astype(np.uint8)
    close(ops.masked_diff(dev(x), dev(y), torch.as_tensor(mask).cuda()), (t64(x) - t64(y)) * t64(mask).unsqueeze(-1))
    sc = rng.normal(size=(16, 1)) * 3
    for label in (0.0, 1.0):
        sr = t64(sc).requires_grad_(True)
        ref = O.gan_d_loss(torch.full((16, 1), label, dtype=torch.float64), sr)
        close(ops.gan_loss_fwd(dev(sc), label), ref.reshape(1), tol=1e-5)
        ref.backward()
        close(ops.gan_loss_bwd(dev(sc), dev([1.0]), label), sr.grad, tol=1e-5)


def test_gan_losses_of_several_heads_in_one_launch():
    """F.gan_losses (cn_gan_loss_grouped) == one F.gan_loss per head: values and score gradients, with different sizes, labels
    and cotangents per head, and with a head whose scalar is not used."""
    from confignet_amd import functional as F
    rng = np.random.default_rng(21)
    shapes = [(16, 1), (16, 1), (7, 1), (16, 1), (33, 1), (16, 1)]
    labels = [1.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    weights = [1.0, 0.5, -2.0, 0.0, 3.0, 1.0]
    scs = [rng.normal(size=s) * 3 for s in shapes]
    a = [dev(s).requires_grad_(True) for s in scs]
    b = [dev(s).requires_grad_(True) for s in scs]
    la = F.gan_losses(a, labels)
    lb = [F.gan_loss(x, l) for x, l in zip(b, labels)]
    for x, y in zip(la, lb):
        assert float((x.detach() - y.detach()).abs()) == 0.0
    used = [0, 1, 2, 4, 5]                                  # head 3 gets no cotangent at all
    ga = torch.autograd.grad(sum(weights[j] * la[j] for j in used), [a[j] for j in used])
    gb = torch.autograd.grad(sum(weights[j] * lb[j] for j in used), [b[j] for j in used])
    for x, y in zip(ga, gb):
        assert float((x - y).abs().max()) == 0.0             # (the same expression per element as the one-head kernels)
    for j, (sc, label) in enumerate(zip(scs, labels)):
        sr = t64(sc)
        ref = O.gan_d_loss(torch.full(sr.shape, label, dtype=torch.float64), sr)
        close(la[j].reshape(1), ref.reshape(1), tol=1e-5)


@pytest.mark.parametrize("deterministic", [False, True])
def test_mlp_bank_equals_the_separate_dense_layers(deterministic):
    """F.mlp_bank (cn_gemm_rows_grouped, one launch per MLP layer for six MLPs) == six chains of F.linear: outputs bit for bit
    (the same per-element arithmetic as gemm_rows_kernel), gradients of the weights, the biases and of the latents -- three of
    the six inputs are ONE tensor, whose gradient the bank adds itself -- with one output left without a cotangent."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    rng = np.random.default_rng(31)
    n, latent, hidden = 8, 145, 128
    outs = [512, 256, 512, 128, 64, 64]
    za, zb = dev(rng.normal(size=(n, latent))), dev(rng.normal(size=(n, latent)))
    sets = [[dev(rng.normal(size=(latent, hidden)) * 0.1), dev(rng.normal(size=hidden) * 0.1), dev(rng.normal(size=(hidden, o)) * 0.1),
             dev(rng.normal(size=o) * 0.1)] for o in outs]
    cot = [dev(rng.normal(size=(n, o))) for o in outs]
    res = {}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(deterministic)
    try:
        for bank in (False, True):
            z1, z2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
            zs = [z1, z2, z1, z1, z2, z1]
            ws = [[t.clone().requires_grad_(True) for t in st] for st in sets]
            if bank:
                sb = F.mlp_bank(zs, ws, 0.2)
            else:
                sb = [F.linear(F.linear(z, w[0], w[1], ops.ACT_LRELU, 0.2), w[2], w[3]) for z, w in zip(zs, ws)]
            loss = sum((o * c).sum() for k, (o, c) in enumerate(zip(sb, cot)) if k != 3)          # MLP 3 gets no cotangent
            leaves = [z1, z2] + [t for k, st in enumerate(ws) if k != 3 for t in st]
            grads = torch.autograd.grad(loss, leaves)
            res[bank] = ([o.detach() for o in sb], grads)
    finally:
        ops.set_deterministic(prev)
    for a, b in zip(res[False][0], res[True][0]):
        assert float((a - b).abs().max()) == 0.0
    for k, (a, b) in enumerate(zip(res[False][1], res[True][1])):
        err = float((a - b).norm() / a.norm())
        assert err < 2e-6, "gradient %d: rel-L2 %.3e" % (k, err)


def test_pools_preproc_uint8():
    from confignet_amd import ops
    rng = np.random.default_rng(6)
    for (k, s, pad), c in [((2, 2, 0), 8), ((3, 2, 1), 8), ((3, 2, 1), 6), ((2, 2, 0), 6)]:   # 4-channel-group and scalar kernels
        x = rng.normal(size=(2, 16, 16, c))
        xr = t64(np.maximum(x, 0) if pad else x).requires_grad_(True)
        ref = O.maxpool(xr, k, s, pad)
        close(ops.maxpool_fwd(dev(xr.detach().numpy()), k, s, pad), ref, what="maxpool")
        gy = rng.normal(size=tuple(ref.shape))
        (ref * t64(gy)).sum().backward()
        close(ops.maxpool_bwd(dev(xr.detach().numpy()), dev(gy), k, s, pad), xr.grad, what="maxpool_bwd")
    # tie rule of the max-pool backward (what oracle.ref_ops.BranchControl(forced=...) relies on): on inputs FULL of exact ties
    # the gradient goes to the first maximum of a window in row-major order -- bit for bit the gather by torch-CPU's
    # max_pool2d(return_indices=True) winners on the same fp32 input (zero padding cells take part and take it nowhere)
    import torch.nn.functional as F
    for (k, s, pad) in ((2, 2, 0), (3, 2, 1)):
        xq = rng.integers(0, 3, size=(2, 12, 12, 8)).astype(np.float32)
        gyq = rng.normal(size=(2, 6, 6, 8)).astype(np.float32)
        xc = torch.tensor(xq).permute(0, 3, 1, 2)
        xp = F.pad(xc, [pad] * 4) if pad else xc
        _, idx = F.max_pool2d(xp, k, s, return_indices=True)
        gxp = torch.zeros_like(xp).flatten(2)
        gxp.scatter_add_(2, idx.flatten(2), torch.tensor(gyq).permute(0, 3, 1, 2).flatten(2))
        gxp = gxp.reshape(xp.shape)
        if pad:
            gxp = gxp[:, :, pad:-pad, pad:-pad]
        got = ops.maxpool_bwd(torch.tensor(xq).cuda(), torch.tensor(gyq).cuda(), k, s, pad).cpu()
        assert torch.allclose(got, gxp.permute(0, 2, 3, 1), atol=1e-6), "max-pool backward tie rule (k=%d s=%d pad=%d)" % (k, s, pad)
    img = rng.uniform(-1, 1, size=(2, 8, 8, 3))
    close(ops.chan_affine3_fwd(dev(img), (2, 1, 0), 127.5, (127.5 - 103.939, 127.5 - 116.779, 127.5 - 123.68)),
          O.caffe_preprocess(t64(img)), tol=1e-5)
    close(ops.chan_affine3_fwd(dev(img), (0, 1, 2), 127.5, (127.5 - 93.5940, 127.5 - 104.7624, 127.5 - 129.1863)),
          O.vggface_preprocess(t64(img)), tol=1e-5)
    ir = t64(img).requires_grad_(True)
    gy = rng.normal(size=img.shape)
    (O.caffe_preprocess(ir) * t64(gy)).sum().backward()
    close(ops.chan_affine3_bwd(dev(gy), (2, 1, 0), 127.5), ir.grad, tol=1e-5)
    # byte output is bit-exact territory: every float32 whose image lies next to an integer boundary included
    big = np.concatenate([rng.uniform(-1.3, 1.3, size=60000).astype(np.float32),
                          np.nextafter((np.arange(0, 256, dtype=np.float32) / np.float32(127.5) - 1).astype(np.float32), np.float32(-2)),
                          (np.arange(0, 256, dtype=np.float32) / np.float32(127.5) - 1).astype(np.float32),
                          np.nextafter((np.arange(0, 256, dtype=np.float32) / np.float32(127.5) - 1).astype(np.float32), np.float32(2))])
    big = np.resize(big, (4, 40, 128, 3)).astype(np.float32)
    ref = ((np.clip(big, np.float32(-1.0), np.float32(1.0)) + np.float32(1)) * np.float32(127.5)).astype(np.uint8)
    got = ops.to_uint8(torch.as_tensor(big).cuda()).cpu().numpy()
    assert np.array_equal(got, ref), "to_uint8: %d of %d bytes differ from NumPy's float32 result" % ((got != ref).sum(), ref.size)
    pool = rng.integers(0, 256, size=(10, 8, 8, 3), dtype=np.uint8)
    idx = np.array([3, 9, 0, 3])
    flip = np.array([0, 1, 1, 0], dtype=np.uint8)
    out = ops.gather_images_u8(torch.as_tensor(pool).cuda(), torch.as_tensor(idx).cuda(), torch.as_tensor(flip).cuda())
    ref = pool[idx].astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    for i in range(4):
        if flip[i]:
            ref[i] = np.fliplr(ref[i])
    assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32))          # integer -> float32: bit-exact as well


@pytest.mark.parametrize("g,c,n", [(4, 8, 2), (16, 128, 2)])
def test_rotate3d(g, c, n):
    from confignet_amd import ops
    rng = np.random.default_rng(g)
    grid = rng.normal(size=(n, g, g, g, c))
    ang = rng.uniform(-0.5, 0.5, size=(n, 3))
    ang[:, 2] = 0
    gr = t64(grid).requires_grad_(True)
    ar = t64(ang).requires_grad_(True)
    Rm = O.euler_angles_to_matrix(ar)
    Rm.retain_grad()
    ref = O.transform_3d_grid(gr, Rm)
    out = ops.rotate3d_fwd(dev(grid), dev(Rm.detach().numpy()))
    close(out, ref, tol=2e-4, what="rotate fwd")
    gout = rng.normal(size=grid.shape)
    (ref * t64(gout)).sum().backward()
    gg, grot = ops.rotate3d_bwd(dev(grid), dev(Rm.detach().numpy()), dev(gout), True)
    close(gg, gr.grad, tol=5e-4, what="rotate ggrid")
    close(grot, Rm.grad, tol=2e-3, what="rotate grot")
    # identity rotation is an exact identity
    eye = torch.eye(3).expand(n, 3, 3).contiguous().cuda()
    assert torch.equal(ops.rotate3d_fwd(dev(grid), eye), dev(grid))
    # euler_angles_to_matrix as one launch (cn_euler_matrix) and its gradient (cn_euler_matrix_bwd), all three angles non-zero
    from confignet_amd import functional as F
    ang3 = rng.uniform(-1.2, 1.2, size=(n + 3, 3))
    a64 = t64(ang3).requires_grad_(True)
    R64 = O.euler_angles_to_matrix(a64)
    cot = rng.normal(size=tuple(R64.shape))
    (R64 * t64(cot)).sum().backward()
    ad = dev(ang3).requires_grad_(True)
    Rd = F.euler_angles_to_matrix(ad)
    close(Rd, R64, tol=1e-6, what="euler matrix")
    (Rd * dev(cot)).sum().backward()
    close(ad.grad, a64.grad, tol=1e-5, what="euler matrix gradient")


def test_adam_ema():
    from confignet_amd import ops
    rng = np.random.default_rng(9)
    th, g = rng.normal(size=1000), rng.normal(size=1000)
    p = t64(th).clone()
    opt = O.KerasAdam(lr=4e-4, beta_1=0.0, beta_2=0.9)
    dth, m, v, ema = dev(th), torch.zeros(1000).cuda(), torch.zeros(1000).cuda(), dev(th)
    ema_ref = t64(th).clone()
    for t in range(1, 5):
        gt = g * t
        opt.apply_gradients([(t64(gt), p)])
        ema_ref = 0.999 * ema_ref + 0.001 * p
        lr_t = 4e-4 * math.sqrt(1 - 0.9 ** t) / (1 - 0.0 ** t)
        ops.adam_step(dth, dev(gt), m, v, ema, dev([lr_t]), 0.0, 0.9, 1e-7, 0.999)
    close(dth, p, tol=1e-6)
    close(ema, ema_ref, tol=1e-6)


UPFOLD_CASES = [
    # (x shape, kernel, cout): UpSampling + Conv(SAME) layers of the generator (hologan_generator.py:139-170)
    ((2, 4, 4, 4, 512), (3, 3, 3), 256),     # map_3d_0
    ((1, 8, 8, 8, 256), (3, 3, 3), 128),     # map_3d_1
    ((2, 16, 16, 256), (4, 4), 64),          # map_2d_1
    ((2, 32, 32, 64), (4, 4), 32),           # map_2d_2
    ((1, 5, 7, 16), (4, 4), 8),              # odd extents
    ((1, 3, 5, 4, 8), (3, 3, 3), 8),         # odd extents, 3-D
    ((2, 6, 6, 16), (3, 3), 16),             # k3 in 2-D
]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", UPFOLD_CASES, ids=[str(i) for i in range(len(UPFOLD_CASES))])
def test_upsample_folded_conv_collapsed_per_parity_class(case, dtype):
    """F.conv with a folded x2 upsample runs as per-parity-class filters (cn_upfold_*): forward (+ bias + LeakyReLU), data
    gradient at the stored extent and filter gradient against the float64 oracle of UpSampling -> Conv(SAME).
    fp32: 2e-4 like every other convolution.  bf16: the oracle on the bf16-rounded x; the class filters are sums of up to 8 taps
    rounded to bf16 AFTER summing, so |err| <= 2^-8 (|y| + sum |terms|) -- asserted as 1.5e-2 of the output scale."""
    upfold_layer_close(case, dtype)


def upfold_layer_close(case, dtype, folded=True):
    """the body of the test above, for tests/test_filter_prep_gpu.py as well; folded: what ops.upfold_ok must say of the layer"""
    from confignet_amd import functional as F
    from confignet_amd import ops
    xs, k, cout = case
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    cin = xs[-1]
    x = rng.normal(size=xs)
    w = rng.normal(size=(*k, cin, cout)) / math.sqrt(np.prod(k) * cin)
    b = rng.normal(size=cout)
    ops.set_activation_dtype(dtype)
    try:
        spec = ops.ConvSpec(k, up=1)
        assert ops.upfold_ok(spec.geom(xs, cout)) == folded
        xt = dev(x)
        if dtype == "bf16":
            xt = xt.to(torch.bfloat16)
        xt.requires_grad_(True)
        wt, bt = dev(w).requires_grad_(True), dev(b).requires_grad_(True)
        xr = (xt.detach().double().cpu()).requires_grad_(True)
        wr, br = t64(w).requires_grad_(True), t64(b).requires_grad_(True)
        tol = 2e-4 if dtype == "f32" else 1.5e-2
        # forward with the fused bias + LeakyReLU epilogue
        close(F.conv(xt, wt, bt, spec, 1, 0.3).float(), O.leaky_relu(O.conv_same(O.upsample2(xr), wr, br), 0.3), tol=tol, what="upfold fwd")
        # gradients of the linear layer (no activation in between: a LeakyReLU whose input is within rounding of zero takes
        # the other branch than in the oracle, which is a property of the comparison, not of the kernels)
        y = F.conv(xt, wt, bt, spec)
        yr = O.conv_same(O.upsample2(xr), wr, br)
        cot = rng.normal(size=tuple(yr.shape))
        cot_t = dev(cot).to(y.dtype)
        gx, gw, gb = torch.autograd.grad((y * cot_t).float().sum(), [xt, wt, bt])
        gxr, gwr, gbr = torch.autograd.grad((yr * cot_t.double().cpu()).sum(), [xr, wr, br])
        close(gx.float(), gxr, tol=tol, what="upfold dgrad")
        close(gw, gwr, tol=5e-4 if dtype == "f32" else 1.5e-2, what="upfold wgrad")
        close(gb, gbr, tol=5e-4 if dtype == "f32" else 1.5e-2, what="upfold bias grad")
    finally:
        ops.set_activation_dtype("f32")


WINO_CASES = [
    # (x shape, cout): 3x3 stride-1 SAME layers routed to cn_conv_fwd_wino (threshold lowered for the small cases)
    ((2, 16, 16, 64), 64),
    ((1, 32, 32, 128), 256),
    ((2, 9, 7, 16), 64),          # odd extents: partial tiles on both axes
    ((1, 5, 6, 16), 128),
    ((2, 40, 24, 32), 64),        # several blocks per image, ragged on one axis
    ((3, 8, 8, 256), 512),
    ((1, 37, 21, 64), 64),
]


@pytest.mark.parametrize("case", WINO_CASES, ids=[str(i) for i in range(len(WINO_CASES))])
def test_winograd_3x3_forward_and_data_gradient(case):
    """Winograd F(2x2, 3x3) forward (+ bias + ReLU epilogue) and data gradient against the float64 oracle of the direct
    convolution, at the same 2e-4 bar as the implicit-GEMM kernels (fp32: the transforms add a few roundings, ~1e-6)."""
    from confignet_amd import ops
    xs, cout = case
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    cin = xs[-1]
    x = rng.normal(size=xs)
    w = rng.normal(size=(3, 3, cin, cout)) / math.sqrt(9 * cin)
    b = rng.normal(size=cout)
    g = ops.ConvSpec((3, 3)).geom(xs, cout)
    keep, ops.WINO_MIN_WGS, ops.WINO_MIN_FILL = (ops.WINO_MIN_WGS, ops.WINO_MIN_FILL), 0, 0.0
    try:
        assert ops._wino_ok(g, cin, cout)
        y = ops.conv_fwd(dev(x), dev(w), dev(b), g, 2, 0.0)
        xr, wr = t64(x).requires_grad_(True), t64(w)
        close(y, torch.relu(O.conv_same(xr, wr, t64(b))), what="winograd fwd")
        yr0 = O.conv_same(xr, wr, None)
        gy = rng.normal(size=tuple(yr0.shape))
        (yr0 * t64(gy)).sum().backward()
        if cin % 64 == 0:
            assert ops._wino_ok(g, cout, cin)
        close(ops.conv_dgrad(dev(gy), dev(w), g), xr.grad, what="winograd dgrad")
    finally:
        ops.WINO_MIN_WGS, ops.WINO_MIN_FILL = keep


@pytest.mark.parametrize("shape,cout,stride", [((2, 16, 16, 256), 1024, 1), ((2, 32, 32, 64), 256, 1), ((1, 8, 8, 512), 2048, 1),
                                               ((2, 16, 16, 128), 96, 1), ((2, 16, 16, 64), 128, 2)])
def test_conv_with_residual_epilogue_and_folded_batchnorm(shape, cout, stride):
    """ops.conv_fwd_res -- relu(conv(x, w) + bias + res), the Add + ReLU of a ResNet block in the last convolution's epilogue
    (cn_conv_fwd_res; with a pass of its own where the launch cannot carry it) -- and cn_scale_columns_segments (BatchNorm
    folded into the filters) against float64: bn(conv(x, w) + b) == conv(x, w * a) + shift."""
    from confignet_amd import ops
    from confignet_amd.ops import ACT_RELU, ConvSpec
    from oracle import ref_ops as O
    rng = np.random.default_rng(5)
    cin = shape[-1]
    x, w = rng.normal(size=shape), rng.normal(size=(1, 1, cin, cout)) / np.sqrt(cin)
    b, a = rng.normal(size=cout), rng.uniform(0.5, 1.5, size=cout)
    spec = ConvSpec((1, 1), stride=stride)
    g = spec.geom(shape, cout)
    res = rng.normal(size=ops.geom_out_shape(g))
    ref = torch.relu(O.conv_same(t64(x), t64(w * a), t64(b), stride) + t64(res))
    # folded filter through the segment kernel: two segments so that the bisection and the packed offsets are exercised
    arena = torch.tensor(np.concatenate([np.zeros(8), w.reshape(-1), np.zeros(4), w.reshape(-1)]), dtype=torch.float32).cuda()
    seg = torch.tensor([[8, 0, w.size, cout, 0], [8 + w.size + 4, w.size, w.size, cout, cout]], dtype=torch.int32).cuda()
    packed = ops.scale_columns_segments(arena, seg, dev(np.concatenate([a, 2 * a])), 2 * w.size)
    wf = packed[:w.size].view(1, 1, cin, cout)
    np.testing.assert_allclose(packed[w.size:].cpu().numpy(), (w * 2 * a).astype(np.float32).reshape(-1), rtol=1e-6)
    got = ops.conv_fwd_res(dev(x), wf, dev(b), dev(res), g, ACT_RELU)
    close(got, ref, tol=2e-4, what="conv + residual + relu")


@pytest.mark.parametrize("shape", [(2, 64, 64, 48), (3, 8, 8, 512), (16, 4, 4, 96), (1, 128, 128, 8)])
def test_tail_statistics_in_one_pass(shape):
    """cn_nc_reduce4: sum x, sum x^2, sum l, sum l^2 (l = leaky_relu(x, 0.3)) per (sample, channel) -- the style statistics and the
    instance-norm statistics of a DiscrBlock's pre-activation tensor (building_blocks.py:97-106) -- against float64, with and
    without the step's zero pool."""
    from confignet_amd import ops
    rng = np.random.default_rng(9)
    x = rng.normal(size=shape)
    xd = dev(x)
    x64 = t64(x)
    l64 = torch.where(x64 > 0, x64, 0.3 * x64)
    refs = [x64.sum((1, 2)), (x64 ** 2).sum((1, 2)), l64.sum((1, 2)), (l64 ** 2).sum((1, 2))]
    for pooled in (False, True):
        if pooled:
            ops.zero_pool_begin("test", xd.device)
        try:
            got = ops.nc_reduce4(xd, 0.3)
            for g, r in zip(got, refs):
                close(g, r, tol=2e-5, what="nc_reduce4")
        finally:
            if pooled:
                ops.zero_pool_end()


WINO4_CASES = [
    # (x shape, cout): 3x3 stride-1 SAME layers whose image divides into 16 x 32-pixel blocks (cn_conv_fwd_wino4)
    ((1, 16, 32, 16), 64),        # one block, one raw stage pair
    ((2, 32, 64, 64), 64),        # several blocks per image: every border of the zero padding
    ((1, 16, 64, 32), 128),       # two channel blocks, reduction channels != output channels
    ((2, 48, 32, 128), 64),
    ((1, 64, 64, 256), 256),      # VGG-19 conv3_x at one sample
]


@pytest.mark.parametrize("case", WINO4_CASES, ids=[str(i) for i in range(len(WINO4_CASES))])
def test_winograd_f4x4_forward_and_data_gradient(case):
    """Winograd F(4x4, 3x3) forward (+ bias + ReLU epilogue) and data gradient against the float64 oracle of the direct convolution
    at the same 2e-4 bar as every other convolution kernel (its larger transform coefficients cost about one digit more than
    F(2x2): the margin is printed)."""
    from confignet_amd import ops
    xs, cout = case
    rng = np.random.default_rng(abs(hash(case)) % 2 ** 31)
    cin = xs[-1]
    x = rng.normal(size=xs)
    w = rng.normal(size=(3, 3, cin, cout)) / math.sqrt(9 * cin)
    b = rng.normal(size=cout)
    g = ops.ConvSpec((3, 3)).geom(xs, cout)
    keep, ops.WINO4_MIN_WGS = ops.WINO4_MIN_WGS, 0
    try:
        assert ops._wino4_ok(g, cin, cout)
        y = ops.conv_fwd(dev(x), dev(w), dev(b), g, 2, 0.0)
        xr, wr = t64(x).requires_grad_(True), t64(w)
        ref = torch.relu(O.conv_same(xr, wr, t64(b)))
        print("F(4x4) fwd max abs err %.2e of scale %.2e" % (float((y.cpu().double() - ref.detach()).abs().max()), float(ref.abs().max())))
        close(y, ref, what="winograd F(4x4) fwd")
        yr0 = O.conv_same(xr, wr, None)
        gy = rng.normal(size=tuple(yr0.shape))
        (yr0 * t64(gy)).sum().backward()
        if cin % 64 == 0:
            assert ops._wino4_ok(g, cout, cin)
        close(ops.conv_dgrad(dev(gy), dev(w), g), xr.grad, what="winograd F(4x4) dgrad")
    finally:
        ops.WINO4_MIN_WGS = keep


@pytest.mark.gpu
def test_convolution_epilogue_statistics_match_the_separate_passes():
    """cn_conv_fwd_stats: the sums AdaIn (building_blocks.py:37-44: of the activated output) and the DiscrBlock tail
    (building_blocks.py:97-106: of the pre-activation output and of its LeakyReLU) need, taken in the convolution's epilogue, against
    the separate statistics passes over the stored output and against float64 sums; the output itself must be the same bits as
    the convolution without statistics.  Includes an upsample-folded layer (parity-ordered rows: a tile's sample comes from the
    class-major index) and a layer whose tiles straddle samples (must NOT fuse)."""
    from confignet_amd import functional as F, ops
    rng = np.random.default_rng(7)
    cases = [  # (x shape, kernel, cout, stride, up, kind, must fuse)
        ((4, 16, 16, 64), (3, 3), 128, 1, 0, "act", True),
        ((4, 16, 16, 64), (1, 1), 128, 1, 0, "act", True),          # plain 1x1 product: launched without a geometry (sample count from the row counts)
        ((4, 16, 16, 64), (1, 1), 128, 1, 0, "pre4", True),
        ((8, 16, 16, 16, 64), (3, 3, 3), 64, 1, 0, "act", True),    # Conv3dAdaIn at 16^3 (the generator's map_3d_post at batch 8)
        ((8, 32, 32, 128), (4, 4), 64, 1, 1, "act", None),          # Conv2dAdaIn with the folded upsample (k4: classes of 9 / 6 / 6 / 4 taps -> K slices even them out: may split)
        ((8, 8, 8, 8, 128), (3, 3, 3), 64, 1, 1, "act", True),      # Conv3dAdaIn with the folded upsample (16^3 outputs: 512 rows per class and sample)
        ((2, 8, 8, 8, 64), (3, 3, 3), 64, 1, 0, "act", None),       # 16 tiles: the launch splits K -> no statistics (either answer is fine for the caller)
        ((16, 32, 32, 96), (3, 3), 192, 2, 0, "pre4", True),        # DiscrBlock 2
        ((5, 64, 64, 48), (3, 3), 96, 2, 0, "pre4", True),          # DiscrBlock 1 (128 x 96 tile or 64 x 64)
        ((6, 8, 8, 384), (3, 3), 768, 2, 0, "pre4", False),         # 16 rows per sample: tiles straddle samples
    ]
    for xs, k, cout, stride, up, kind, must in cases:
        if ops.DETERMINISTIC:
            must = False                             # (the sums are added with atomics: refused in deterministic mode, the consumer runs its own pass)
        spec = ops.ConvSpec(k, stride=stride, up=up)
        x = torch.tensor(rng.normal(size=xs).astype(np.float32)).cuda()
        w = torch.tensor((rng.normal(size=(*k, xs[-1], cout)) / math.sqrt(np.prod(k) * xs[-1])).astype(np.float32)).cuda()
        b = torch.tensor(rng.normal(size=cout).astype(np.float32)).cuda()
        act, slope = (ops.ACT_LRELU, 0.3) if kind == "act" else (ops.ACT_NONE, 0.0)
        with torch.no_grad():
            y0 = F.conv(x, w, b, spec, act, slope)
            ops.zero_pool_begin("stats_test", x.device)
            try:
                with ops.request_stats(kind, 0.3):
                    y1 = F.conv(x, w, b, spec, act, slope)
                st = ops.take_stats(y1, kind)
                assert must is None or (st is not None) == must, (xs, kind, st is not None)
                if st is None:
                    continue
                assert torch.equal(y0, y1)           # (a launch that carries statistics has no K split: same bits every time)
                st = [t.clone() for t in st]
            finally:
                ops.zero_pool_end()
        y64 = y1.double().reshape(xs[0], -1, cout)
        l64 = torch.where(y64 > 0, y64, 0.3 * y64)
        ref = [y64.sum(1), (y64 * y64).sum(1)] + ([l64.sum(1), (l64 * l64).sum(1)] if kind == "pre4" else [])
        for got, r in zip(st, ref):
            assert tuple(got.shape) == (xs[0], cout)
            assert float((got.double() - r).abs().max()) <= 1e-5 * float(r.abs().max()) + 1e-4, (xs, kind)
        sep = ops.nc_reduce(y1) if kind == "act" else ops.nc_reduce4(y1, 0.3)
        for got, r in zip(st, sep):
            assert float((got - r).abs().max()) <= 2e-5 * float(r.abs().max()) + 1e-4


@pytest.mark.gpu
def test_keras_form_apply_gradients_checks_a_variable_list_once_per_state_of_the_moments():
    """optim.Adam.apply_gradients(zip(grads, vars)) (the Keras form train scripts use): a variable list that leaves out a weight which
    already has optimizer state must fail -- and that check, a masked reduction with a host synchronisation, must run once per list
    and state of the moments, not on every call: A, A, A checks once; A, superset B, A fails on the third call."""
    from confignet_amd import optim
    from confignet_amd.nn import Net
    net = Net()
    for i in range(3):
        net.add_weight("w%d" % i, np.ones((8, 4), np.float32) * (i + 1))
    net.finalize()
    opt = optim.Adam(lr=1e-3, beta_1=0.0, beta_2=0.9)
    w = net.trainable_weights
    g = [torch.ones_like(t) for t in w]
    syncs = []
    real_any = torch.Tensor.any

    def counting_any(self, *a, **k):
        syncs.append(1)
        return real_any(self, *a, **k)

    torch.Tensor.any = counting_any
    try:
        a_list = lambda: list(zip(g[:2], w[:2]))
        for _ in range(4):
            opt.apply_gradients(a_list())
        assert len(syncs) == 1, len(syncs)                # (first call: no state yet; second: checked; then cached)
        opt.apply_gradients(list(zip(g, w)))              # superset B: lists w2 for the first time -> new moments
        n = len(syncs)
        opt.apply_gradients(list(zip(g, w)))
        assert len(syncs) == n                            # B itself: cached
        with pytest.raises(AssertionError, match="unlisted weight"):
            opt.apply_gradients(a_list())                 # A again: w2 has moments now
    finally:
        torch.Tensor.any = real_any


@pytest.mark.gpu
def test_slab_reductions_of_a_backward_pass_as_one_grouped_launch_give_the_same_bits():
    """Round 6: inside a backward pass (ops.grad_sink) a filter gradient that splits its rows leaves its slabs behind
    (cn_conv_wgrad_ws_slabs) and the pass adds the slabs of ALL its filter gradients at its join with cn_sum_parts_grouped -- one
    launch per 80 jobs instead of one per layer.  Every job is reduced as cn_conv_wgrad_ws reduces it: SAME BITS, in store and in
    accumulate mode, for both reduction schemes (< 64 and >= 64 slices), more than 80 jobs in one pass, two streams."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    gen = torch.Generator(device="cuda").manual_seed(21)
    shapes = [((8, 32, 32, 128), (3, 3), 128, 1), ((16, 32, 32, 96), (3, 3), 192, 2), ((8, 16, 16, 256), (1, 1), 1024, 1),
              ((4, 16, 16, 16, 64), (3, 3, 3), 64, 1), ((16, 64, 64, 48), (3, 3), 96, 2)]
    cases = []
    for xs, k, cout, stride in shapes:
        g = ops.ConvSpec(k, stride=stride).geom(xs, cout)
        assert int(lib.cn_conv_wgrad_workspace_bytes(ctypes.byref(g))) > 0, "the case must split its rows"
        x = torch.randn(xs, device="cuda", generator=gen)
        gy = torch.randn(ops.geom_out_shape(g), device="cuda", generator=gen)
        cases.append((x, gy, g, tuple(k) + (xs[-1], cout)))
    cases = cases + [cases[2]] * 84                     # > 80 jobs: a second launch of the grouped kernel
    base = [torch.randn(c[3], device="cuda", generator=gen) for c in cases]
    ref = []
    for (x, gy, g, ws), b in zip(cases, base):          # outside a pass: slabs + the per-layer reduction launch
        ref.append(ops.conv_wgrad(x, gy, g, ws, out=b.clone()).clone())
    params = []
    for b in base:
        p = torch.zeros_like(b).requires_grad_(True)
        p.grad = b.clone()
        params.append(p)
    side = torch.cuda.Stream()
    with ops.grad_sink(params):
        for i, ((x, gy, g, ws), p) in enumerate(zip(cases, params)):
            if i % 2:                                    # every other filter gradient on a second stream (a forked step has two)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    ops.sink_conv_wgrad(x, gy, g, ws, p.grad)
            else:
                ops.sink_conv_wgrad(x, gy, g, ws, p.grad)
    torch.cuda.synchronize()
    for i, (p, r) in enumerate(zip(params, ref)):
        assert torch.equal(p.grad, r), (i, float((p.grad - r).abs().max()))


@pytest.mark.gpu
def test_dense_weight_gradients_of_a_backward_pass_as_one_grouped_launch_give_the_same_bits():
    """Round 6: inside a backward pass the weight gradients of dense layers over <= 32 rows (x^T gy: the AdaIN MLPs, encoders, regressor)
    are queued and launched together at the pass' join (cn_gemm_depth_grouped); per job the arithmetic of cn_gemm_acc(ta = 1): same
    bits, more than 64 jobs in one pass, a destination used twice (two launches, fixed order), rows > 32 fall back to cn_gemm_acc."""
    from confignet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(33)
    dims = [(16, 145, 128), (8, 128, 512), (32, 43, 43), (16, 128, 64), (5, 7, 130), (48, 64, 64)] + [(16, 128, 256)] * 70
    jobs = [(torch.randn(k, m, device="cuda", generator=gen), torch.randn(k, n, device="cuda", generator=gen)) for k, m, n in dims]
    base = [torch.randn(m, n, device="cuda", generator=gen) for _, m, n in dims]
    ref = [ops.gemm_acc(a, b, c.clone(), True, False).clone() for (a, b), c in zip(jobs, base)]
    params = []
    for c in base:
        p = torch.zeros_like(c).requires_grad_(True)
        p.grad = c.clone()
        params.append(p)
    with ops.grad_sink(params):
        for (a, b), p in zip(jobs, params):
            ops.sink_gemm(a, b, p.grad, True, False)
        ops.sink_gemm(jobs[0][0], jobs[0][1], params[0].grad, True, False)       # the first weight used a second time in the pass
    torch.cuda.synchronize()
    ref0 = ops.gemm_acc(jobs[0][0], jobs[0][1], ref[0].clone(), True, False)
    assert torch.equal(params[0].grad, ref0)
    for i, (p, r) in enumerate(zip(params, ref)):
        if i:
            assert torch.equal(p.grad, r), (i, dims[i], float((p.grad - r).abs().max()))


@pytest.mark.gpu
def test_undeferred_sink_launches_are_complete_before_the_pass_joins():
    """defer=False inside a backward pass (ops.grad_sink): sink_conv_wgrad_to on a geometry that splits its rows and sum_rows_into
    behave as outside one -- the whole result is in the destination on the launching stream BEFORE the sink is left, nothing is
    kept for its join (a node whose network the sink does not hold: ResNetTrunkFn) -- and has the bits of the call outside a sink."""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    gen = torch.Generator(device="cuda").manual_seed(57)
    xs, k, cout = (8, 32, 32, 128), (3, 3), 128
    g = ops.ConvSpec(k, stride=1).geom(xs, cout)
    assert int(lib.cn_conv_wgrad_workspace_bytes(ctypes.byref(g))) > 0, "the case must split its rows"
    x = torch.randn(xs, device="cuda", generator=gen)
    gy = torch.randn(ops.geom_out_shape(g), device="cuda", generator=gen)
    ws = k + (xs[-1], cout)
    part = torch.randn(48, 200, device="cuda", generator=gen)
    base = torch.randn(200, device="cuda", generator=gen)
    ref_w = torch.full(ws, float("nan"), device="cuda")           # (a scratch the call WRITES: every element must be replaced)
    ops.sink_conv_wgrad_to(x, gy, g, ws, ref_w)
    ref_s = base.clone()
    ops.sum_rows_into(part, ref_s)
    assert not torch.isnan(ref_w).any()
    p = torch.zeros(4, device="cuda").requires_grad_(True)
    p.grad = torch.zeros_like(p)
    got_w, got_s = torch.full(ws, float("nan"), device="cuda"), base.clone()
    with ops.grad_sink([p]):
        assert ops.sink_for(p) is not None
        ops.sink_conv_wgrad_to(x, gy, g, ws, got_w, defer=False)
        ops.sum_rows_into(part, got_s, defer=False)
        seen_w, seen_s = got_w.clone(), got_s.clone()          # read on the launching stream, inside the pass
    torch.cuda.synchronize()
    assert torch.equal(seen_w, ref_w), float((seen_w - ref_w).abs().max())
    assert torch.equal(seen_s, ref_s), float((seen_s - ref_s).abs().max())
    assert torch.equal(got_w, ref_w) and torch.equal(got_s, ref_s)      # (and the join added nothing on top)


@pytest.mark.gpu
def test_work_queued_on_the_sink_by_a_post_function_is_refused():
    """A sink_post function runs after the join has issued the pass' grouped launches: work it queues on the sink would never be
    launched.  The join raises instead of dropping it (host-side, nothing is launched for the stray job), and the failed pass
    leaves no sink behind."""
    from confignet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(58)
    a = torch.randn(16, 64, device="cuda", generator=gen)
    b = torch.randn(16, 32, device="cuda", generator=gen)
    p = torch.zeros(64, 32, device="cuda").requires_grad_(True)
    p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="queued work on the gradient sink"):
        with ops.grad_sink([p]):
            ops.sink_post(lambda: ops.sink_gemm(a, b, p.grad, True, False))
    with ops.grad_sink([p]):
        assert ops.sink_for(p) is p.grad
    torch.cuda.synchronize()
    assert not p.grad.any()


# ---------------------------------------------------------------------------------------------
# round 6 (second half): the entry points behind the restructured tape, each against a float64 statement of what it computes
# ---------------------------------------------------------------------------------------------
def _lrelu64(x, slope):
    return torch.where(x > 0, x, slope * x)


@pytest.mark.parametrize("with_g,rows", [(True, 1), (False, 1), (True, 3)])
def test_tap_backward_in_one_pass(with_g, rows):
    """cn_tap_bwd: (g + (y - target) s[row] k) relu'(y) -- the feature-loss term's gradient, the gradient from the next layer and
    the layer's own ReLU derivative (perceptual_loss.py:74-82) -- with one scale for the whole tensor and with one per sample."""
    from confignet_amd import ops
    rng = np.random.default_rng(41)
    shape = (3, 10, 12, 8)
    y = np.maximum(rng.normal(size=shape), 0.0)
    tgt, g = rng.normal(size=shape), rng.normal(size=shape)
    s = rng.uniform(0.5, 2.0, size=rows)
    k = 0.37
    out = ops.tap_bwd(dev(y), dev(tgt), dev(g) if with_g else None, dev(s), k, ops.ACT_RELU)
    sb = t64(s).reshape(rows, 1, 1, 1) if rows > 1 else t64(s)
    ref = ((t64(g) if with_g else 0.0) + (t64(y) - t64(tgt)) * sb * k) * (t64(y) > 0)
    close(out, ref, tol=1e-6, what="tap_bwd")


@pytest.mark.parametrize("tap", [False, True])
def test_relu_maxpool_backward_in_one_pass(tap):
    """cn_maxpool2_bwd_act: the gradient of ReLU -> MaxPooling2D(2, 2) w.r.t. the ReLU's input side (the routed gradient times
    relu'(x)), with the tap's own term added before the mask, against autograd on the float64 composite."""
    from confignet_amd import ops
    rng = np.random.default_rng(42)
    n, h, w, c = 2, 12, 16, 8
    x = np.maximum(rng.normal(size=(n, h, w, c)), 0.0)             # a ReLU output (zeros included)
    gy = rng.normal(size=(n, h // 2, w // 2, c))
    tgt = rng.normal(size=(n, h, w, c))
    s, k = rng.uniform(0.5, 2.0, size=n), 0.21
    out = ops.maxpool2_bwd_relu(dev(x), dev(gy), dev(tgt) if tap else None, dev(s) if tap else None, k if tap else 0.0)
    assert out is not None
    xr = t64(x).requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(xr.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    (routed,) = torch.autograd.grad((pooled * t64(gy)).sum(), xr)
    ref = routed + ((t64(x) - t64(tgt)) * t64(s).reshape(n, 1, 1, 1) * k if tap else 0.0)
    ref = ref * (t64(x) > 0)
    # (ties inside a window can only occur between zeros of the ReLU output, and those positions are masked out)
    close(out, ref, tol=1e-6, what="maxpool2_bwd_relu")
    assert ops.maxpool2_bwd_relu(dev(x[:, :11]), dev(gy[:, :5]), None, None, 0.0) is None       # odd extent: the caller's two passes


@pytest.mark.parametrize("lazy", [False, True])
def test_r1_tail_backward_reductions_and_gradients_in_two_passes(lazy):
    """cn_nc_reduce_hxt (sum h, sum h lrelu(x), sum h ta per (n, c) over a stack of heads against one copy of x) and
    cn_dual_tail_gx_tx (the gradient w.r.t. the primal activation AND w.r.t. the stacked tangent input from one pass) against
    float64 statements of the same sums / maps; lazy: ta = lrelu'(x) tx formed inside the passes from the tangent input."""
    from confignet_amd import ops
    rng = np.random.default_rng(43)
    n, heads, hh, ww, c, slope = 2, 3, 6, 10, 8, 0.3
    x = rng.normal(size=(n, hh, ww, c))
    tx = rng.normal(size=((heads + 1) * n, hh, ww, c))
    h = rng.normal(size=(heads * n, hh, ww, c))
    x64, tx64, h64 = t64(x), t64(tx), t64(h)
    xr = x64.repeat(heads, 1, 1, 1)
    mask = torch.where(xr > 0, 1.0, slope)
    ta64 = mask * tx64[n:]
    ta = (dev(tx)[n:] if lazy else dev(ta64.numpy()))
    H1, H2, E = ops.nc_reduce_hxt(dev(h), dev(x), ta, slope, ta_is_tx=lazy)
    close(H1, h64.sum((1, 2)), tol=1e-5, what="sum h")
    close(H2, (h64 * _lrelu64(xr, slope)).sum((1, 2)), tol=1e-5, what="sum h lrelu(x)")
    close(E, (h64 * ta64).sum((1, 2)), tol=1e-5, what="sum h ta")
    names = ("kh", "kt", "ka", "kc", "K1", "K2", "K0")
    co = {k: rng.normal(size=(heads * n, c)) for k in names}
    co.update({k: rng.normal(size=(n, c)) for k in ("et", "ex", "e0", "D2", "D0")})
    cod = {k: dev(v) for k, v in co.items()}
    gx, gtx = ops.dual_tail_gx_tx(dev(h), ta, dev(tx), dev(x), cod, slope, ta_is_tx=lazy)
    b = lambda k, rows: t64(co[k]).reshape(rows, 1, 1, c)
    a64 = _lrelu64(xr, slope)
    per_head = mask * (b("kh", heads * n) * h64 + b("kt", heads * n) * ta64 + b("ka", heads * n) * a64 + b("kc", heads * n))
    ref_gx = per_head.reshape(heads, n, hh, ww, c).sum(0) + b("et", n) * tx64[:n] + b("ex", n) * x64 + b("e0", n)
    ref_gtx = torch.cat([b("D2", n) * x64 + b("D0", n), mask * (b("K1", heads * n) * h64 + b("K2", heads * n) * a64 + b("K0", heads * n))])
    close(gx, ref_gx, tol=1e-5, what="g_x")
    close(gtx, ref_gtx, tol=1e-5, what="g_tx")


@pytest.mark.parametrize("mode", ["adain", "instance"])
def test_norm_apply_with_inline_coefficients(mode):
    """cn_norm_apply (AdaIn / instance norm apply and backward map with the coefficient algebra inline) against float64 autograd
    on the layer's definition (building_blocks.py:132-149: layer norm over space, eps inside the root, x (s + 1) + b;
    instance_normalization.py:108-131 behind LeakyReLU: (l - mean) / (std + eps) gamma + beta)."""
    from confignet_amd import ops
    rng = np.random.default_rng(44)
    n, hh, ww, c, slope, eps = 2, 64, 64, 16, 0.3, 1e-3
    x = rng.normal(size=(n, hh, ww, c)) * 2 + 0.5
    gy = rng.normal(size=(n, hh, ww, c))
    S = hh * ww
    xr = t64(x).requires_grad_(True)
    if mode == "adain":
        sb = rng.normal(size=(n, 2 * c)) * 0.5
        sbr = t64(sb).requires_grad_(True)
        mu = xr.mean((1, 2), keepdim=True)
        var = ((xr - mu) ** 2).mean((1, 2), keepdim=True)
        ref = (xr - mu) / torch.sqrt(var + eps) * (sbr[:, :c].reshape(n, 1, 1, c) + 1.0) + sbr[:, c:].reshape(n, 1, 1, c)
        s1, s2 = ops.nc_reduce(dev(x))
        fwd = ops.norm_apply_fwd(ops.NORM_ADAIN, dev(x), s1, s2, dev(sb), None, eps)
        assert fwd is not None
        y, mean, r = fwd
        close(y, ref, tol=2e-5, what="adain apply")
        gxr, gsbr = torch.autograd.grad((ref * t64(gy)).sum(), (xr, sbr))
        t1, t2 = ops.nc_reduce(dev(gy), dev(x))
        gx, gsb, _ = ops.norm_apply_bwd(ops.NORM_ADAIN, dev(gy), dev(x), t1, t2, mean, r, dev(sb), eps)
        close(gx, gxr, tol=5e-5, what="adain d x")
        close(gsb, gsbr, tol=2e-4, what="adain d [s|b]")
    else:
        gamma, beta = rng.normal(size=c) * 0.5 + 1.0, rng.normal(size=c) * 0.1
        gr, br = t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
        l = _lrelu64(xr, slope)
        mu = l.mean((1, 2), keepdim=True)
        sd = torch.sqrt(((l - mu) ** 2).mean((1, 2), keepdim=True))
        ref = (l - mu) / (sd + eps) * gr + br
        a1, a2 = ops.nc_reduce(dev(x), flags=1, slope=slope)
        fwd = ops.norm_apply_fwd(ops.NORM_INSTANCE, dev(x), a1, a2, dev(gamma), dev(beta), eps, flags=1, slope=slope)
        assert fwd is not None
        y, mean, q = fwd
        close(y, ref, tol=2e-5, what="instance norm apply")
        gxr, ggr, gbr = torch.autograd.grad((ref * t64(gy)).sum(), (xr, gr, br))
        t1, t2 = ops.nc_reduce(dev(gy), dev(x), flags=2, slope=slope)
        gx, gg, gb = ops.norm_apply_bwd(ops.NORM_INSTANCE, dev(gy), dev(x), t1, t2, mean, q, dev(gamma), eps, flags=2 | 4, slope=slope)
        close(gx, gxr, tol=5e-5, what="instance norm d x")
        close(gg, ggr, tol=2e-4 * S ** 0.5, what="d gamma")
        close(gb, gbr, tol=2e-4 * S ** 0.5, what="d beta")


def test_batchnorm_fold_adjoint():
    """cn_bn_fold_bwd against float64 autograd through the folding  w' = w a, shift = beta + a (b - mean), a = gamma rsqrt(var + eps)
    for three filters of different shapes laid out in one arena (offsets as RealEncoder._fold_table9 builds them)."""
    from confignet_amd import ops
    rng = np.random.default_rng(45)
    shapes = [(3, 3, 8, 64), (1, 1, 64, 128), (1, 1, 32, 64)]
    eps = 1.001e-5
    arena, offs, rows, packed, aoff, blk = [], {}, [], 0, 0, 0
    def put(name, a):
        offs[name] = sum(len(v) for v in arena)
        arena.append(np.asarray(a, np.float64).reshape(-1))
    params = []
    for i, shp in enumerate(shapes):
        cout = shp[-1]
        w, b, gam, bet = rng.normal(size=shp) * 0.1, rng.normal(size=cout) * 0.1, rng.uniform(0.5, 1.5, size=cout), rng.normal(size=cout) * 0.1
        mean, var = rng.normal(size=cout) * 0.1, rng.uniform(0.5, 2.0, size=cout)
        for nm, a in (("w%d" % i, w), ("b%d" % i, b), ("g%d" % i, gam), ("be%d" % i, bet)):
            put(nm, a)
        params.append((w, b, gam, bet, mean, var))
        rows.append([offs["w%d" % i], packed, w.size, cout, aoff, offs["b%d" % i], offs["g%d" % i], offs["be%d" % i], blk])
        packed, aoff, blk = packed + w.size, aoff + cout, blk + cout // 64
    flat = np.concatenate(arena)
    gwf = rng.normal(size=packed)
    gsh = rng.normal(size=aoff)
    a_cat = np.concatenate([p[2] / np.sqrt(p[5] + eps) for p in params])
    rs_cat = np.concatenate([1.0 / np.sqrt(p[5] + eps) for p in params])
    bm_cat = np.concatenate([p[1] - p[4] for p in params])
    gout = torch.zeros(flat.size, device="cuda", dtype=torch.float32)
    seg9 = torch.tensor(rows, dtype=torch.int32, device="cuda")
    ops.bn_fold_bwd(seg9, blk, dev(gwf), dev(gsh), dev(flat), dev(a_cat), dev(rs_cat), dev(bm_cat), gout)
    ref = torch.zeros(flat.size, dtype=torch.float64)
    po = ao = 0
    for i, (w, b, gam, bet, mean, var) in enumerate(params):
        cout = w.shape[-1]
        wr, br_, gr, ber = (t64(v).requires_grad_(True) for v in (w, b, gam, bet))
        a = gr / torch.sqrt(t64(var) + eps)
        obj = (wr * a * t64(gwf[po:po + w.size]).reshape(w.shape)).sum() + ((ber + a * (br_ - t64(mean))) * t64(gsh[ao:ao + cout])).sum()
        gs = torch.autograd.grad(obj, (wr, br_, gr, ber))
        for nm, g_ in zip(("w%d" % i, "b%d" % i, "g%d" % i, "be%d" % i), gs):
            ref[offs[nm]:offs[nm] + g_.numel()] = g_.reshape(-1)
        po, ao = po + w.size, ao + cout
    close(gout, ref, tol=1e-5, what="bn_fold_bwd")


def test_grouped_rows_gemm_against_float64():
    """cn_gemm_rows_grouped: four jobs of different shapes in one launch -- plain, transposed B with bias and LeakyReLU, the
    activation-derivative epilogue (mask), and two jobs accumulating into ONE output."""
    from confignet_amd import ops
    rng = np.random.default_rng(46)
    A = [rng.normal(size=s) for s in ((8, 145), (8, 128), (5, 64), (8, 64), (8, 64))]
    B = [rng.normal(size=(145, 128)), rng.normal(size=(300, 128)), rng.normal(size=(64, 96)), rng.normal(size=(64, 40)), rng.normal(size=(64, 40))]
    bias1 = rng.normal(size=300)
    mask = rng.normal(size=(5, 96))
    outs = [torch.empty((8, 128), device="cuda"), torch.empty((8, 300), device="cuda"), torch.empty((5, 96), device="cuda"), torch.zeros((8, 40), device="cuda")]
    jobs = [(dev(A[0]), dev(B[0]), outs[0], None, None, False, ops.ACT_NONE, 0.0, False),
            (dev(A[1]), dev(B[1]), outs[1], dev(bias1), None, True, ops.ACT_LRELU, 0.2, False),
            (dev(A[2]), dev(B[2]), outs[2], None, dev(mask), False, ops.ACT_LRELU, 0.2, False),
            (dev(A[3]), dev(B[3]), outs[3], None, None, False, ops.ACT_NONE, 0.0, True),
            (dev(A[4]), dev(B[4]), outs[3], None, None, False, ops.ACT_NONE, 0.0, True)]
    ops.gemm_rows_grouped(jobs)
    close(outs[0], t64(A[0]) @ t64(B[0]), tol=1e-5, what="plain")
    close(outs[1], _lrelu64(t64(A[1]) @ t64(B[1]).T + t64(bias1), 0.2), tol=1e-5, what="B^T + bias + lrelu")
    close(outs[2], (t64(A[2]) @ t64(B[2])) * torch.where(t64(mask) > 0, 1.0, 0.2), tol=1e-5, what="activation-derivative epilogue")
    close(outs[3], t64(A[3]) @ t64(B[3]) + t64(A[4]) @ t64(B[4]), tol=1e-5, what="two jobs into one output")
