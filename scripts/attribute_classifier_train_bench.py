"""Times one training step of the CelebA attribute classifier (AttributeClassifierNet.train_on_batch) at the reference's
setting, 256 x 256 input and batch 32, and the kernel families that training added, layer by layer.

    python scripts/attribute_classifier_train_bench.py [--size 256] [--batch 32] [--steps 30] [--warmup 5]
        [--out profiles/attribute_classifier_training.txt]

Step time: a host clock around `steps` steps that end in a device synchronise, after `warmup` steps.  Kernel families: every
depthwise layer and every BatchNormalization of the network at this input size is launched `reps` times between two device
events, on tensors of the layer's shape; a family's time is the sum over its layers of the mean launch time.  The byte model of
each family ("Training") gives achieved bytes per second; these kernels are memory bound, so the share of
the HBM rate is the roofline figure.  Back-to-back launches on the same tensors: a layer whose tensors fit the 256 MiB
last-level cache is flattered by it, which the per-layer lines let a reader see.  Needs a GPU; nothing is measured without one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s (HBM3E specification of the MI355X)


def layer_shapes(size, batch):
    """[(kind, stride, input shape NHWC, output shape NHWC)] of the 52 triples at this input size"""
    from confignet_amd.metrics.mobilenet_v2 import mobilenet_v2_graph
    shapes, out = {}, []
    for name, kind, ins, p in mobilenet_v2_graph():
        if kind == "input":
            shapes[name] = (batch, size, size, 3)
        elif kind in ("conv", "dw"):
            n, h, w, c = shapes[ins[0]]
            s = p["stride"]
            shapes[name] = (n, -(-h // s), -(-w // s), p["filters"] if kind == "conv" else c)
            out.append((kind, s, shapes[ins[0]], shapes[name]))
        else:
            shapes[name] = shapes[ins[0]]
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def families(size, batch, reps):
    """{family: (seconds, model bytes)} summed over the network's layers, and the per-layer lines"""
    from confignet_amd import ops
    from confignet_amd._lib import lib
    fam, lines = {}, []

    def add(name, sec, nbytes, what):
        t, b = fam.get(name, (0.0, 0.0))
        fam[name] = (t + sec, b + nbytes)
        lines.append("    %-16s %-28s %9.1f us %8.1f MB %7.2f TB/s" % (name, what, sec * 1e6, nbytes / 1e6, nbytes / sec / 1e12))

    g = torch.Generator(device="cuda").manual_seed(0)
    for idx, (kind, s, xin, xout) in enumerate(layer_shapes(size, batch)):
        c = xout[-1]
        fx, fy = 4.0 * np.prod(xin), 4.0 * np.prod(xout)
        act = ops.ACT_NONE if (kind == "conv" and idx > 0 and xin[-1] > c) else ops.ACT_RELU6      # the projections are linear
        z = torch.randn(xout, device="cuda", generator=g)
        gy = torch.randn(xout, device="cuda", generator=g)
        gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        what = "%s %dx%dx%d" % ("relu6" if act else "linear", xout[1], xout[2], c)
        add("bn_fwd_reduce", timed(lambda: ops.nc_reduce(z, None, per_channel=True), reps), fy, what)
        y, saved = ops.bn_train_fwd(z, gamma, beta, None, None, act)
        co = torch.empty((5, c), device="cuda")
        m = int(np.prod(xout[:-1]))
        add("bn_apply", timed(lambda: lib.cn_bn_train_apply(z.data_ptr(), saved[3].data_ptr(), co[4].data_ptr(), y.data_ptr(), m, c, act,
                                                           torch.cuda.current_stream().cuda_stream), reps), 2 * fy, what)
        reads = 3 if act else 2
        slices = lib.cn_bn_train_bwd_slices(m, c)
        part, sums, gx = torch.empty((slices, 2 * c), device="cuda"), torch.zeros(2 * c, device="cuda"), torch.empty_like(z)
        yp = y.data_ptr() if act else None
        st = torch.cuda.current_stream().cuda_stream
        add("bn_bwd_reduce", timed(lambda: lib.cn_bn_train_bwd_reduce(gy.data_ptr(), yp, z.data_ptr(), saved[0].data_ptr(), saved[2].data_ptr(),
                                                                     part.data_ptr(), slices, m, c, act, st), reps), reads * fy, what)
        add("bn_bwd_apply", timed(lambda: lib.cn_bn_train_bwd_apply(gy.data_ptr(), yp, z.data_ptr(), saved[0].data_ptr(), saved[2].data_ptr(),
                                                                   saved[3].data_ptr(), sums.data_ptr(), gx.data_ptr(), m, c, act, st), reps),
            (reads + 1) * fy, what)
        if kind == "dw":
            x = torch.randn(xin, device="cuda", generator=g)
            w = torch.randn((3, 3, c, 1), device="cuda", generator=g)
            what = "s%d %dx%dx%d" % (s, xin[1], xin[2], c)
            add("dw_fwd", timed(lambda: ops.dwconv3x3_fwd(x, w, None, s), reps), fx + fy, what)
            add("dw_dgrad", timed(lambda: ops.dwconv3x3_dgrad(gy, w, xin, s, out=x), reps), fx + fy, what)
            nsl = lib.cn_dwconv3x3_wgrad_slices(xin[0], xin[1], xin[2], c, s)
            wp = torch.empty((nsl, 9 * c), device="cuda")
            add("dw_wgrad", timed(lambda: lib.cn_dwconv3x3_wgrad(x.data_ptr(), gy.data_ptr(), wp.data_ptr(), nsl, xin[0], xin[1], xin[2], c, s, st),
                                  reps), fx + fy + 4.0 * wp.numel(), what + " %d slices" % nsl)
        del z, gy, y, gx
    return fam, lines


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--attributes", type=int, default=38)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribute_classifier_training.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("attribute_classifier_train_bench.py needs an MI355X: nothing is measured without one")
    from confignet_amd.metrics.celeba_attribute_prediction import AttributeClassifierNet
    from confignet_amd.optim import Adam
    net = AttributeClassifierNet((args.size, args.size, 3), args.attributes, seed=0)
    opt = Adam(lr=1e-3)
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.uniform(-1, 1, (args.batch, args.size, args.size, 3)).astype(np.float32)).cuda()
    t = torch.as_tensor(rng.integers(0, 2, (args.batch, args.attributes)).astype(np.float32)).cuda()
    for _ in range(args.warmup):
        net.train_on_batch(x, t, opt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, _ = net.train_on_batch(x, t, opt)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / args.steps
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    fam, lines = families(args.size, args.batch, args.reps)
    out = ["attribute classifier training step: input %d x %d, batch %d, %d attributes, fp32" % (args.size, args.size, args.batch, args.attributes),
           "%.2f ms per step (%d steps after %d warm-up steps, host clock around synchronised work), %.1f images/s, loss %.4f, "
           "peak device memory %.1f GiB" % (step * 1e3, args.steps, args.warmup, args.batch / step, float(loss), peak), "",
           "kernel time by family per step (sum over the network's layers of the mean of %d back-to-back launches, device events)," % args.reps,
           "model bytes (DESIGN.md section 3, Training), achieved rate and its share of the %.1f TB/s HBM specification:" % (HBM_PEAK / 1e12),
           "  %-16s %10s %10s %9s %7s" % ("family", "ms", "MB", "TB/s", "of HBM")]
    total = 0.0
    for name, (sec, nbytes) in fam.items():
        total += sec
        out.append("  %-16s %10.3f %10.1f %9.2f %6.1f%%" % (name, sec * 1e3, nbytes / 1e6, nbytes / sec / 1e12, 100.0 * nbytes / sec / HBM_PEAK))
    out += ["  %-16s %10.3f" % ("these families", total * 1e3),
            "  %-16s %10.3f   (full convolutions and their gradients, the head, the loss, Adam, launch gaps)" % ("everything else", (step - total) * 1e3),
            "", "per layer:"] + lines
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
