"""The ResNet-50 trunk's backward with the ReLU backward and the shift sums in the data gradients' epilogues
(RealEncoder.fused_relu_bwd; ops.conv_dgrad_mask -> cn_conv_dgrad_w_mask / cn_conv_fwd_wino_ep) against the walk that runs a pass
behind every data gradient.

RealEncoder at 64 x 64, n = 2, with and without a gradient sink, as tests/test_wgrad_grouped_gpu.py: every trunk parameter gradient and
the input gradient of both walks against the float64 oracle.  Every data gradient of the fused walk has the bits of the unfused one
(tests/test_dgrad_mask_gpu.py), so the filter gradients are the same launches on the same operands; only the order in which the shift
sums are added differs (a workgroup's columns, then atomics, instead of row slices added in order).  The fused walk's rel-L2 error
of EACH tensor may therefore be at most TWICE the unfused walk's error of that tensor, the unfused walk being the reference.

That argument needs a step whose convolutions give the same bits from run to run.  With the built-in plan they do not: at this size
(M = 8 .. 512 rows) the forward pass and most data gradients of conv4_x / conv5_x split K and add their slices with fp32 atomics, and so
do the two dense heads behind the trunk -- two steps of ONE walk then differ in every tensor (measured on an MI355X: 3.7e-7 rel-L2 of
the arena, none of 212 tensors with the same bits).  So the comparison runs in a setting where they do, "unsplit":
  * K splits switched off for both walks (cn_conv_tune(-1, 1, 0)), as the Winograd threshold is lowered for both (below);
  * the loss is taken on the trunk's own output, sum(features * c) with a fixed c, so no dense head lies between the loss and the trunk.
What is then left to differ between two steps are the sums that end in atomics: the shift sums (and the tensors derived from them:
bias, beta, gamma gradients) and the filter gradient of the atomic kernel (conv1).  The test runs the unfused walk twice; the input
gradient and every filter gradient that has the same bits in those two runs -- at least 52 of the 53, asserted -- must have the SAME
BITS in the fused walk, and every tensor, those included, is held to twice its own unfused error (measured: the largest ratio of one
tensor is 1.05, the two walks' arenas are 5e-9 apart).

The built-in plan -- what the benchmark runs, split launches falling back to the pass -- is run as well, through the whole encoder, and
held as tests/test_wgrad_grouped_gpu.py holds the grouped filter gradients (arena and worst tensor to twice the unfused walk's).

At this size the trunk's 3x3 layers are below Winograd F(2x2)'s workgroup threshold (16 x 16 pixels, n = 2: two workgroups), so the
threshold is lowered for BOTH walks: conv2_x's 3x3 data gradients then run on F(2x2), and the test asserts that launches of both
kinds fused.  Deterministic mode must take the old walk."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _randomize(net, seed, scale):
    rng = np.random.default_rng(seed)
    ws = net.get_weights()
    for i, w in enumerate(ws):
        if w.ndim == 1:
            ws[i] = (w + rng.normal(size=w.shape) * scale).astype(np.float32)
    net.set_weights(ws)


def _loss(enc, img, c):
    """c None: the encoder's two heads (as tests/test_wgrad_grouped_gpu.py); else the trunk's output against the fixed c"""
    if c is None:
        emb, rot = enc(img)
        return (emb ** 2).sum() + (rot ** 2).sum() * 10
    return (enc.features(img) * c).sum()


def _step(enc, img_np, sink, c=None):
    """one forward + backward: (gradient arena, input gradient) as float64 on the CPU"""
    from confignet_amd import nn as cnn
    base = enc.arena.data_ptr()
    img = torch.tensor(img_np, device="cuda", requires_grad=True)
    loss = _loss(enc, img, c)
    if sink:
        gimg = cnn.backward_into_arenas(loss, [enc], extra=[img])[0]
    else:
        grads = torch.autograd.grad(loss, list(enc.trainable_weights) + [img], allow_unused=True)
        gimg = grads[-1]
        enc.grad_arena.zero_()
        for p_, g_ in zip(enc.trainable_weights, grads[:-1]):
            if g_ is not None:
                o = (p_.data_ptr() - base) // 4
                enc.grad_arena[o:o + p_.numel()] += g_.reshape(-1)
    torch.cuda.synchronize()
    return enc.grad_arena.detach().double().cpu(), gimg.detach().double().cpu()


@functools.lru_cache(maxsize=None)
def _setup():
    """the encoder, its input, the fixed c, the table (name, offset, size) of the trunk's trainable tensors and, per loss ("heads" /
    "trunk"), the float64 oracle's gradients laid out like the gradient arena and its input gradient -- made once, shared, never changed"""
    from confignet_amd.dnn_models.real_encoder import RealEncoder
    from oracle import ref_nets as R
    from oracle import ref_ops as O
    rng = np.random.default_rng(11)
    enc = RealEncoder(43, (64, 64, 3), ((-30, 30), (-10, 10), (0, 0)), rng=rng)
    _randomize(enc, 7, 0.05)
    img_np = rng.uniform(-1, 1, size=(2, 64, 64, 3)).astype(np.float32)
    c_np = rng.normal(size=(2, 2048)).astype(np.float32)
    base = enc.arena.data_ptr()
    every = [(enc._entries[i][0], (enc.weights[i].data_ptr() - base) // 4, enc.weights[i].numel()) for i in enc._trainable_idx]
    trunk = {enc.weights[i].data_ptr() for i in range(len(enc.weights) - 4)}
    table = [t for t, i in zip(every, enc._trainable_idx) if enc.weights[i].data_ptr() in trunk]
    refs = {}
    for kind in ("heads", "trunk"):
        wr = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in enc.get_weights()]
        img64 = torch.tensor(img_np, dtype=torch.float64, requires_grad=True)
        if kind == "heads":
            e, r = R.real_encoder_forward(wr, img64)
            loss = (e ** 2).sum() + (r ** 2).sum() * 10
        else:
            loss = (R.resnet50_features(R._W(wr), O.caffe_preprocess(img64)) * torch.tensor(c_np, dtype=torch.float64)).sum()
        g64 = torch.autograd.grad(loss, [wr[i] for i in enc._trainable_idx] + [img64], allow_unused=True)
        ref = torch.zeros(enc.arena.numel(), dtype=torch.float64)
        for (_, o, n), g_ in zip(every, g64[:-1]):
            if g_ is not None:
                ref[o:o + n] = g_.reshape(-1)
        refs[kind] = (ref, g64[-1].detach())
    return enc, img_np, torch.tensor(c_np, device="cuda"), table, refs


@functools.lru_cache(maxsize=None)
def _trunk_runs(unsplit):
    """{(sink, walk): (gradient arena, input gradient, log of conv_dgrad_mask)}, walk = False (unfused), True (fused), "again" (unfused,
    a second time); for the built-in plan also the same of a deterministic-mode step"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    from confignet_amd.dnn_models.real_encoder import RealEncoder
    enc, img_np, c = _setup()[:3]
    runs, det = {}, None
    was_wgs, was_det = ops.WINO_MIN_WGS, ops.DETERMINISTIC
    assert RealEncoder.fused_relu_bwd is True
    try:
        ops.WINO_MIN_WGS = 1
        ops.set_deterministic(False)
        ops.check(lib.cn_conv_tune(-1, 1 if unsplit else 0, 0), "cn_conv_tune")
        for sink in (False, True):
            for walk in (False, True, "again"):
                RealEncoder.fused_relu_bwd = walk is True
                ops.MASK_LOG = log = []
                arena, gimg = _step(enc, img_np, sink, c if unsplit else None)
                runs[(sink, walk)] = (arena, gimg, tuple(log))
        RealEncoder.fused_relu_bwd = True
        if not unsplit:
            ops.set_deterministic(True)
            ops.MASK_LOG = det_log = []
            det = _step(enc, img_np, True) + (tuple(det_log),)
    finally:
        RealEncoder.fused_relu_bwd = True
        ops.MASK_LOG = None
        ops.WINO_MIN_WGS = was_wgs
        ops.set_deterministic(was_det)
        lib.cn_conv_tune(-1, 0, 0)
    return runs, det


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _measure(unsplit, sink):
    enc, img_np, c, table, refs = _setup()
    ref, gimg_ref = refs["trunk" if unsplit else "heads"]
    runs, _ = _trunk_runs(unsplit)
    (a_u, x_u, log_u), (a_f, x_f, log_f), (a_2, x_2, _) = runs[(sink, False)], runs[(sink, True)], runs[(sink, "again")]
    assert np.isfinite(a_f.numpy()).all() and np.isfinite(x_f.numpy()).all()
    assert log_u == () and len(log_f) == 47, (len(log_u), len(log_f))          # 16 blocks x 3 passes - the topmost one
    m = {"err_u": {name: _rel(a_u[o:o + n], ref[o:o + n]) for name, o, n in table},
         "err_f": {name: _rel(a_f[o:o + n], ref[o:o + n]) for name, o, n in table},
         "repro": [name for name, o, n in table if torch.equal(a_u[o:o + n], a_2[o:o + n])],
         "same": [name for name, o, n in table if torch.equal(a_u[o:o + n], a_f[o:o + n])],
         "whole": (_rel(a_u, ref), _rel(a_f, ref)), "x": (_rel(x_u, gimg_ref), _rel(x_f, gimg_ref)),
         "x_repro": torch.equal(x_u, x_2), "x_same": torch.equal(x_u, x_f), "log": log_f}
    worst_u, worst_f = max(m["err_u"].values()), max(m["err_f"].values())
    ratio = max((m["err_f"][k] / m["err_u"][k], k) for k in m["err_u"] if m["err_u"][k] > 0.0)
    kern = [name for name, o, n in table if name.endswith("kernel")]
    print("trunk vs float64, %s plan, sink=%s, %d tensors: unfused arena %.3e worst tensor %.3e; fused arena %.3e worst tensor %.3e; largest "
          "fused / unfused ratio of one tensor %.3f (%s); input gradient unfused %.3e fused %.3e; unfused twice: %d tensors (%d of %d filter "
          "gradients) and the input gradient (%s) with the same bits; fused vs unfused: %d tensors and the input gradient (%s) with the same bits, "
          "arena %.3e apart (unfused twice %.3e); launches fused: %d fwd2, %d wino, %d pass"
          % ("unsplit" if unsplit else "built-in", sink, len(table), m["whole"][0], worst_u, m["whole"][1], worst_f, ratio[0], ratio[1], m["x"][0], m["x"][1],
             len(m["repro"]), len(set(m["repro"]) & set(kern)), len(kern), m["x_repro"], len(m["same"]), m["x_same"], _rel(a_f, a_u), _rel(a_2, a_u),
             log_f.count("fwd2"), log_f.count("wino"), log_f.count("pass")))
    m.update(worst=(worst_u, worst_f), kernels=kern, not_repro=sorted(set(kern) - set(m["repro"])))
    return m


@pytest.mark.parametrize("sink", [False, True])
def test_every_tensor_of_the_fused_walk_within_twice_its_unfused_error(sink):
    """The unsplit setting: measured on an MI355X in profiles/resnet_relu_epilogue_ab.txt, section 5."""
    m = _measure(True, sink)
    assert len(m["kernels"]) == 53 and m["worst"][0] > 0.0 and m["x"][0] > 0.0
    # what two unfused steps reproduce: the input gradient and every filter gradient but conv1's (the atomic kernel: 3 input channels)
    assert m["x_repro"] and set(m["not_repro"]) <= {"conv1_conv/kernel"}, m["not_repro"]
    # ... has the same bits in the fused walk
    assert m["x_same"], "the input gradient of the fused walk differs from the unfused walk's"
    # (the filter gradients: bias, beta and gamma gradients come from the shift sums, whose order of additions is what changed)
    missing = sorted((set(m["repro"]) & set(m["kernels"])) - set(m["same"]))
    assert len(set(m["repro"]) & set(m["kernels"])) >= 52
    assert not missing, "filter gradients reproducible in the unfused walk, different in the fused one: %s" % missing[:8]
    # every tensor: at most twice its own unfused error
    for name in m["err_u"]:
        assert m["err_f"][name] <= 2.0 * m["err_u"][name], "%s: fused rel-L2 %.3e, unfused %.3e" % (name, m["err_f"][name], m["err_u"][name])
    assert m["x"][1] <= 2.0 * m["x"][0]


@pytest.mark.parametrize("sink", [False, True])
def test_the_built_in_plan_within_twice_the_unfused_error(sink):
    """Split launches keep their pass; two steps of one walk differ in every tensor here (see the head of the file), so the whole arena,
    the worst tensor and the input gradient are held, as tests/test_wgrad_grouped_gpu.py holds the grouped filter gradients."""
    m = _measure(False, sink)
    assert m["worst"][0] > 0.0 and m["whole"][0] > 0.0 and m["x"][0] > 0.0
    assert m["whole"][1] <= 2.0 * m["whole"][0], "gradient arena: fused rel-L2 %.3e, unfused %.3e" % (m["whole"][1], m["whole"][0])
    assert m["worst"][1] <= 2.0 * m["worst"][0], "worst tensor: fused %.3e, unfused %.3e" % (m["worst"][1], m["worst"][0])
    assert m["x"][1] <= 2.0 * m["x"][0], "input gradient: fused rel-L2 %.3e, unfused %.3e" % (m["x"][1], m["x"][0])


def test_launches_of_both_kinds_fuse_at_this_size_and_deterministic_mode_takes_the_old_walk():
    for unsplit in (True, False):
        runs, det = _trunk_runs(unsplit)
        for sink in (False, True):
            log = runs[(sink, True)][2]
            assert log.count("fwd2") >= 1 and log.count("wino") >= 1, log
    det_log = det[2]
    assert len(det_log) == 47 and set(det_log) == {"pass"}, det_log
    assert np.isfinite(det[0].numpy()).all()
