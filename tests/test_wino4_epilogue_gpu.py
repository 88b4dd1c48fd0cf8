"""Epilogue modes of the Winograd F(4x4) launch (cn_conv_fwd_wino4_ep: POOL, POOL_ONLY, MASK) against the launches and passes they
replace, bit for bit where the arithmetic is the same; the 4-channel-group max-pool forward kernel against the generic one; and
VGGLossFn with the fused epilogues on against off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU = 0, 2
EP_POOL, EP_POOL_ONLY, EP_MASK = 1, 2, 3
# (n, h, w, cin, cout): one workgroup / a workgroup count that is no multiple of 8 (no XCD remap) / 16 workgroups (remap on, two channel
# blocks, interior block borders in both directions)
GEOMS = [(1, 16, 32, 16, 64), (3, 16, 32, 16, 64), (2, 32, 64, 32, 128)]


def _lib():
    from confignet_amd import _lib
    return _lib.lib


def _p(t):
    return None if t is None else t.data_ptr()


def _ok(rc, what):
    assert rc == 0, "%s: rc %d (%s)" % (what, rc, _lib().cn_last_error_string())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape, what
    bad = int((_bits(a) != _bits(b)).sum())
    assert bad == 0, "%s: %d of %d elements differ in their bits" % (what, bad, a.numel())


_CASES = {}


def _case(geom):
    """Operands of one geometry and the plain launch's results, computed once and shared (nothing below writes to them)."""
    if geom in _CASES:
        return _CASES[geom]
    n, h, w, cin, cout = geom
    rng = np.random.default_rng(sum(geom))
    dev = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda().contiguous()
    x = dev(rng.normal(size=(n, h, w, cin)))
    wt = dev(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9.0 * cin))
    bias = dev(rng.normal(size=(cout,)) * 0.3)
    u = torch.empty((36, cin, cout), device="cuda", dtype=torch.float32)
    _ok(_lib().cn_conv_wino4_filter(_p(wt), _p(u), cin, cout, 0, None), "cn_conv_wino4_filter")
    c = {"x": x, "u": u, "bias": bias, "plain": {}}
    for key, (b, act) in {"relu": (bias, ACT_RELU), "none": (None, ACT_NONE)}.items():
        y = torch.empty((n, h, w, cout), device="cuda", dtype=torch.float32)
        _ok(_lib().cn_conv_fwd_wino4(n, h, w, cin, cout, _p(x), _p(u), _p(b), _p(y), act, 0.0, None), "cn_conv_fwd_wino4")
        pooled = torch.empty((n, h // 2, w // 2, cout), device="cuda", dtype=torch.float32)
        _ok(_lib().cn_maxpool_fwd(_p(y), _p(pooled), n, h, w, cout, 2, 2, 0, 0, None), "cn_maxpool_fwd")
        c["plain"][key] = (y, pooled)
    _CASES[geom] = c
    return c


def _ep(geom, c, bias, act, mode, y, pooled=None, ym=None, target=None, s=None, k=0.0):
    n, h, w, cin, cout = geom
    _ok(_lib().cn_conv_fwd_wino4_ep(n, h, w, cin, cout, _p(c["x"]), _p(c["u"]), _p(bias), _p(y), act, 0.0, mode, _p(pooled), _p(ym), _p(target),
                                    _p(s), 1 if s is None else s.numel(), k, None), "cn_conv_fwd_wino4_ep")


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("key", ["relu", "none"])
def test_pool_and_pool_only_equal_the_plain_launch_and_the_pool_pass(geom, key):
    n, h, w, cin, cout = geom
    c = _case(geom)
    y0, p0 = c["plain"][key]
    bias, act = (c["bias"], ACT_RELU) if key == "relu" else (None, ACT_NONE)
    y = torch.full_like(y0, float("nan"))
    pooled = torch.full_like(p0, float("nan"))
    _ep(geom, c, bias, act, EP_POOL, y, pooled)
    _same(y, y0, "POOL: full-size output")
    _same(pooled, p0, "POOL: pooled output")
    sentinel = torch.full_like(y0, -7.25)
    pooled = torch.full_like(p0, float("nan"))
    _ep(geom, c, bias, act, EP_POOL_ONLY, sentinel, pooled)
    _same(pooled, p0, "POOL_ONLY: pooled output")
    _same(sentinel, torch.full_like(y0, -7.25), "POOL_ONLY: the full-size buffer")
    pooled = torch.full_like(p0, float("nan"))
    _ep(geom, c, bias, act, EP_POOL_ONLY, None, pooled)                     # (no full-size buffer at all)
    _same(pooled, p0, "POOL_ONLY without y: pooled output")


def _two_launch(geom, g, ym, target, s, k):
    """cn_act_bwd / cn_tap_bwd on the plain launch's result g."""
    out = torch.empty_like(g)
    if target is None:
        _ok(_lib().cn_act_bwd(_p(g), _p(ym), _p(out), g.numel(), ACT_RELU, 0.0, 0, None), "cn_act_bwd")
    else:
        _ok(_lib().cn_tap_bwd(_p(ym), _p(target), _p(g), _p(s), _p(out), s.numel(), g.numel() // s.numel(), k, ACT_RELU, 0.0, 0, None), "cn_tap_bwd")
    return out


@pytest.mark.parametrize("geom", GEOMS)
def test_mask_on_exact_inputs_equals_the_two_launches(geom):
    """y and t small integers, s k a power of two: (y - t) s k is exact, so the fused and the separate multiply-add round once, alike."""
    n, h, w, cin, cout = geom
    c = _case(geom)
    g = c["plain"]["none"][0]
    rng = np.random.default_rng(5 + n)
    ym = torch.as_tensor(rng.integers(-3, 4, size=tuple(g.shape)).astype(np.float32)).cuda()
    target = torch.as_tensor(rng.integers(-3, 4, size=tuple(g.shape)).astype(np.float32)).cuda()
    tiles = (ym > 0).reshape(n, h // 4, 4, w // 4, 4, cout).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16 * cout)
    assert bool(tiles.any(1).all()) and not bool(tiles.all(1).any())        # both mask outcomes in every tile
    s1 = torch.tensor([0.5], device="cuda")
    sn = torch.as_tensor((2.0 ** rng.integers(-3, 3, size=n)).astype(np.float32)).cuda()
    for what, t_, s_, k_ in (("no target", None, None, 0.0), ("one scale", target, s1, 0.25), ("n scales", target, sn, 0.25)):
        out = torch.full_like(g, float("nan"))
        _ep(geom, c, None, ACT_NONE, EP_MASK, out, ym=ym, target=t_, s=s_, k=k_)
        _same(out, _two_launch(geom, g, ym, t_, s_, k_), "MASK, " + what)


@pytest.mark.parametrize("geom", GEOMS)
def test_mask_on_random_inputs_differs_by_one_contraction_at_most(geom):
    """|fused - two-launch| <= 2^-23 (|g| + |(y - t) s k|): the two forms differ by the contraction of one multiply-add and nothing else."""
    n, h, w, cin, cout = geom
    c = _case(geom)
    g = c["plain"]["none"][0]
    rng = np.random.default_rng(11 + n)
    ym = torch.as_tensor(rng.normal(size=tuple(g.shape)).astype(np.float32)).cuda()
    ym = torch.where(ym > 0, ym, torch.zeros_like(ym))                      # (a ReLU output: zeros where the mask is off)
    target = torch.as_tensor(rng.normal(size=tuple(g.shape)).astype(np.float32)).cuda()
    sn = torch.as_tensor(rng.uniform(0.5, 2.0, size=n).astype(np.float32)).cuda()
    k = 0.37
    out = torch.empty_like(g)
    _ep(geom, c, None, ACT_NONE, EP_MASK, out, ym=ym, target=target, s=sn, k=k)
    ref = _two_launch(geom, g, ym, target, sn, k)
    term = (ym.double() - target.double()) * (sn.double() * float(np.float32(k))).reshape(n, 1, 1, 1)
    bound = 2.0 ** -23 * (g.double().abs() + term.abs())
    diff = (out.double() - ref.double()).abs()
    worst = float((diff - bound).max())
    print("MASK random: largest difference %.3e, largest (difference - bound) %.3e" % (float(diff.max()), worst))
    assert worst <= 0.0


def _pool_ref(x, k, s, pad):
    """Zero padding cells take part when pad > 0 (keras MaxPooling2D after ZeroPadding2D); a max has no rounding."""
    import torch.nn.functional as F
    xc = x.cpu().permute(0, 3, 1, 2)
    if pad:
        xc = F.pad(xc, [pad, pad, pad, pad])
    return F.max_pool2d(xc, k, s).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape,k,s,pad", [((2, 9, 14, 8), 3, 2, 1), ((1, 4, 6, 4), 2, 2, 0), ((2, 9, 14, 6), 3, 2, 1)])
def test_maxpool_fwd_group_kernel_equals_the_generic_kernel(shape, k, s, pad):
    """c % 4 == 0 on 16-byte aligned tensors takes the 4-channel-group kernel; the same values at an address that is not 16-byte aligned
    take the generic kernel, as does c = 6."""
    n, h, w, c = shape
    rng = np.random.default_rng(h * w + c)
    x = torch.as_tensor((rng.normal(size=shape) - 0.5).astype(np.float32)).cuda()       # (mostly negative: the padding cells win some windows)
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    y = torch.full((n, oh, ow, c), float("nan"), device="cuda")
    _ok(_lib().cn_maxpool_fwd(_p(x), _p(y), n, h, w, c, k, s, pad, 0, None), "cn_maxpool_fwd")
    store = torch.empty(x.numel() + 1, device="cuda")
    xg = store[1:].view(shape)                                                           # 4 bytes off a 16-byte boundary
    xg.copy_(x)
    assert xg.data_ptr() % 16 == 4
    yg = torch.full((n, oh, ow, c), float("nan"), device="cuda")
    _ok(_lib().cn_maxpool_fwd(_p(xg), _p(yg), n, h, w, c, k, s, pad, 0, None), "cn_maxpool_fwd (generic)")
    _same(y, yg, "group kernel against generic kernel")
    _same(y.cpu(), _pool_ref(x, k, s, pad), "against the window maxima computed on the host")


def test_vgg_loss_fused_epilogues_on_against_off():
    """VGG-19 at n = 2, 32 x 64, every F(4x4)-shaped layer on F(4x4) (WINO4_MIN_WGS = 0), deterministic mode: POOL at conv1_2 / conv2_2,
    POOL_ONLY at conv2_2 of the target pass, MASK with the tap term in the data gradient of conv1_2 and without in that of conv2_2.
    The forward changes are exact: same loss bits.  The backward forms differ by multiply-add contractions at the tap; the bound is
    propagated through the stack by measuring against a float64 run of the same stack that takes the product's own ReLU / arg-max
    decisions (oracle BranchControl(forced=...)): the unfused path's relative L2 error e_off against it is fp32 rounding of the
    same operations, one more rounding per tapped element cannot double it, so the fused path is held to 2 e_off."""
    from confignet_amd import ops
    from confignet_amd.dnn_models import vgg
    from oracle import ref_nets as R
    from oracle import ref_ops as O
    rng = np.random.default_rng(77)
    net = vgg.VGGFeatures(vgg.VGG19_CFG, vgg.VGG19_TAPS)
    ws = net.get_weights()
    for i, a in enumerate(ws):
        if a.ndim == 1:
            ws[i] = (a + rng.normal(size=a.shape) * 0.1).astype(np.float32)
    net.set_weights(ws)
    xa = rng.normal(size=(2, 32, 64, 3)) * 50.0
    xb = rng.normal(size=(2, 32, 64, 3)) * 50.0
    prev = (ops.DETERMINISTIC, ops.WINO4_MIN_WGS, vgg.VGG_FUSED_EPILOGUES, ops.conv_fwd_pool, ops.conv_dgrad_masked)
    out, taken = {}, {False: [], True: []}

    def counted(fn, name):                      # (which fused launches a pass really took: the comparison must not be off against off)
        def call(*a, **k):
            r = fn(*a, **k)
            if r is not None:
                taken[vgg.VGG_FUSED_EPILOGUES].append((name, k.get("keep_full", True), name == "mask" and len(a) > 4 and a[4] is not None))
            return r
        return call
    try:
        ops.conv_fwd_pool, ops.conv_dgrad_masked = counted(prev[3], "pool"), counted(prev[4], "mask")
        ops.set_deterministic(True)
        ops.WINO4_MIN_WGS = 0
        for fused in (False, True):
            vgg.VGG_FUSED_EPILOGUES = fused
            with torch.no_grad():
                targets = [t.detach() for t in net(net.to_device(xb))]
            x = torch.tensor(xa, device="cuda", dtype=torch.float32, requires_grad=True)
            loss = vgg.VGGLossFn.apply(net, x, None, *targets)
            with ops.branch_log() as log:
                (gx,) = torch.autograd.grad(loss, x)
            out[fused] = (loss.detach().clone(), gx.detach().clone(), log, targets)
    finally:
        ops.set_deterministic(prev[0])
        ops.WINO4_MIN_WGS, vgg.VGG_FUSED_EPILOGUES, ops.conv_fwd_pool, ops.conv_dgrad_masked = prev[1:]
    # target pass: conv1_2 (a tap: POOL) and conv2_2 (POOL_ONLY); live pass: POOL twice; backward: MASK with the tap term (conv1_2's data
    # gradient, layer conv1_1) and without (conv2_2's, layer conv2_1)
    assert taken[False] == []
    assert sorted(taken[True]) == sorted([("pool", True, False), ("pool", False, False), ("pool", True, False), ("pool", True, False),
                                          ("mask", True, False), ("mask", True, True)]), taken[True]
    (l0, g0, log0, t0), (l1, g1, log1, t1) = out[False], out[True]
    for a, b in zip(t0, t1):
        _same(a, b, "target features")
    _same(l0.reshape(1), l1.reshape(1), "loss")
    assert len(log0) == len(log1) and len(log0) > 0
    for r0, r1 in zip(log0, log1):
        assert r0[0] == r1[0] and tuple(r0[2:]) == tuple(r1[2:]) and torch.equal(r0[1], r1[1]), "BRANCH_LOG records differ"
    w64 = [torch.tensor(a, dtype=torch.float64) for a in net.get_weights()]
    t64 = [t.cpu().double() for t in t0]
    O.BranchControl.start(forced=log0)
    try:
        xr = torch.tensor(xa, dtype=torch.float64, requires_grad=True)
        feats = R.vgg_features(w64, xr, vgg.VGG19_CFG, vgg.VGG19_TAPS)
        ref = sum(((a - b) ** 2).mean() for a, b in zip(feats, t64))
        (gr,) = torch.autograd.grad(ref, xr)
        rep = O.BranchControl.forced_report()
    finally:
        O.BranchControl.stop()
    assert not rep["unmatched"] and rep["forced_calls"] > 0
    e_off = float((g0.cpu().double() - gr).norm() / gr.norm())
    e_on = float((g1.cpu().double() - gr).norm() / gr.norm())
    print("VGGLossFn gradient against float64 with forced decisions: rel-L2 off %.3e, on %.3e; on against off %.3e" %
          (e_off, e_on, float((g1.double() - g0.double()).norm() / g0.double().norm())))
    assert e_off <= 5e-3, "the unfused path itself is off: rel-L2 %.3e" % e_off     # (the bar of every forced-decision gradient check)
    assert e_on <= 2.0 * e_off, "fused epilogues: rel-L2 %.3e against float64, unfused %.3e" % (e_on, e_off)
