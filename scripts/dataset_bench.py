#!/usr/bin/env python
"""Stage rates of dataset creation (confignet_amd/face_image_normalizer.py, neural_renderer_dataset.py) on synthetic files:
N 1024 x 1024 PNG sources -> pre-normalisation warp (1024 x 1024) -> head-centre warp (256 x 256) -> UV nearest warp and eye masks
-> Inception features -> PNG + memmap write, for the HIP path (device="cuda") and the numpy path (16 threads) on the same machine.

    python scripts/dataset_bench.py [--n 256] [--numpy_n 64] [--uv_n 32] [--out profiles/dataset_creation.txt]

Every rate is images per second of wall clock around work that ends in a device synchronise (the HIP warps include the copies
to and from the device, which the pipeline pays; the kernel alone is timed with device events as well).  Decoding, writing and the
features are the same code on both paths.  The numpy warps are timed on --numpy_n pictures, the 12 MB UV maps on --uv_n.  A GPU is
required: this measures, it does not fall back."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def smooth_image(rng, size):
    """a picture that compresses like a render: low-frequency colour plus a little noise"""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    base = np.stack([np.sin(6.0 * xx + rng.uniform(0, 6)) * np.cos(5.0 * yy + rng.uniform(0, 6)) for _ in range(3)], axis=-1)
    return np.clip(128 + 100 * base + rng.normal(0, 4, size=base.shape), 0, 255).astype(np.uint8)


def transforms(rng, n, src, dst):
    """similarities like the normaliser's: a few degrees, the scale that takes src to dst +- 20 %, small shifts"""
    Ms = []
    for _ in range(n):
        a, s = np.deg2rad(rng.uniform(-15, 15)), dst / src * rng.uniform(0.8, 1.2)
        A = s * np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        t = np.array([dst / 2, dst * 0.42]) - A @ np.array([src / 2 + rng.uniform(-20, 20), src / 2 + rng.uniform(-20, 20)])
        Ms.append(np.hstack([A, t[:, None]]))
    return Ms


def rate(n, seconds):
    return "%8.1f img/s (%d in %.3f s)" % (n / seconds, n, seconds)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--numpy_n", type=int, default=64)
    ap.add_argument("--uv_n", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "dataset_bench.py measures on the GPU"
    from confignet_amd import exr, ops
    from confignet_amd import face_image_normalizer as F
    from confignet_amd.metrics import InceptionFeatureExtractor
    from confignet_amd.neural_renderer_dataset import eye_mask_from_uv

    rng = np.random.default_rng(0)
    n, lines = args.n, []

    def note(line):
        print(line, flush=True)
        lines.append(line)

    note("dataset creation, %d sources of 1024 x 1024 -> 1024 x 1024 -> 256 x 256; %s; %d decode / numpy threads"
         % (n, torch.cuda.get_device_name(0), F.MAX_THREADS))
    with tempfile.TemporaryDirectory() as tmp:
        few = [smooth_image(rng, 1024) for _ in range(8)]
        paths = [os.path.join(tmp, "img_%05d.png" % i) for i in range(n)]
        F.thread_map(lambda a: F.imwrite(*a), [(p, np.roll(few[i % 8], 37 * i, axis=1)) for i, p in enumerate(paths)])
        uv_paths = [os.path.join(tmp, "uv_%05d.exr" % i) for i in range(args.uv_n)]
        F.thread_map(lambda p: exr.imwrite(p, rng.random((1024, 1024, 3)).astype(np.float32)), uv_paths)

        t = time.perf_counter()
        images = np.stack(F.thread_map(F.imread, paths))
        note("decode PNG 1024^2 (Pillow)          " + rate(n, time.perf_counter() - t))
        t = time.perf_counter()
        uvs = np.stack(F.thread_map(exr.imread, uv_paths))
        note("decode EXR 1024^2 FLOAT (exr.py)    " + rate(len(uv_paths), time.perf_counter() - t))

        M_pre, M_head = transforms(rng, n, 1024, 1024), transforms(rng, n, 1024, 256)
        results = {}
        for device, count in (("cuda", n), (None, min(n, args.numpy_n))):
            name = "HIP  " if device else "numpy"
            for rep in range(2 if device else 1):                      # the first HIP pass loads the code objects
                torch.cuda.synchronize()
                t = time.perf_counter()
                pre = np.concatenate([F.warp_affine(images[b:b + F.CHUNK], M_pre[b:b + F.CHUNK], (1024, 1024), device)
                                      for b in range(0, count, F.CHUNK)])
                t_pre = time.perf_counter() - t
                t = time.perf_counter()
                small = np.concatenate([F.warp_affine(pre[b:b + F.CHUNK], M_head[b:b + F.CHUNK], (256, 256), device)
                                        for b in range(0, count, F.CHUNK)])
                t_head = time.perf_counter() - t
                k = min(count, len(uvs))
                t = time.perf_counter()
                uv_small = F.warp_affine_nearest(uvs[:k], M_head[:k], (256, 256), device)
                t_uv = time.perf_counter() - t
                uv_many = np.concatenate([uv_small] * (count // k))
                t = time.perf_counter()
                masks = eye_mask_from_uv(uv_many, device)
                t_mask = time.perf_counter() - t
            note("%s warp u8 1024^2 -> 1024^2        " % name + rate(count, t_pre))
            note("%s warp u8 1024^2 -> 256^2         " % name + rate(count, t_head))
            note("%s warp f32 nearest 1024^2 -> 256^2" % name + rate(k, t_uv))
            note("%s eye mask 256^2                  " % name + rate(len(uv_many), t_mask))
            results[device] = (pre[:args.numpy_n], small[:args.numpy_n], uv_small, masks[:k])
        same = all(np.array_equal(a, b) for a, b in zip(results["cuda"][:2], results[None][:2]))
        k = min(len(results["cuda"][2]), len(results[None][2]))
        same = same and np.array_equal(results["cuda"][2][:k].view(np.uint32), results[None][2][:k].view(np.uint32)) \
            and np.array_equal(results["cuda"][3][:k], results[None][3][:k])
        note("HIP and numpy outputs bit-equal on the %d pictures both did: %s" % (min(n, args.numpy_n), same))

        # the kernels alone, device events around launches on resident data
        dev_imgs = torch.from_numpy(images[:F.CHUNK]).cuda()
        for (oh, ow), Ms in (((1024, 1024), M_pre), ((256, 256), M_head)):
            tabs = [torch.from_numpy(x).cuda() for x in F.batch_tables(Ms[:F.CHUNK], oh, ow, F.ROUND_DELTA_LINEAR)]
            out = ops.warp_affine_u8(dev_imgs, tabs, oh, ow)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(100):
                ops.warp_affine_u8(dev_imgs, tabs, oh, ow, out=out)
            end.record()
            torch.cuda.synchronize()
            ms = start.elapsed_time(end) / 100
            moved = out.numel() + min(dev_imgs.numel(), 4 * out.numel())          # written once; read: the source once, or four taps per pixel if that is less
            note("cn_warp_affine_u8 kernel, %d x 1024^2 -> %d^2: %.3f ms per launch, %.0f img/s, %.0f GB/s of algorithmic bytes"
                 % (len(dev_imgs), oh, ms, len(dev_imgs) / ms * 1e3, moved / ms / 1e6))

        small = results["cuda"][1] if len(results["cuda"][1]) == n else np.concatenate([results["cuda"][1]] * (n // len(results["cuda"][1])))
        extractor = InceptionFeatureExtractor((256, 256, 3))
        extractor.get_features(small[:32])
        torch.cuda.synchronize()
        t = time.perf_counter()
        feats = extractor.get_features(small)
        torch.cuda.synchronize()
        note("InceptionV3 features 256^2 (HIP)    " + rate(len(small), time.perf_counter() - t))
        assert feats.shape == (len(small), 2048) and np.isfinite(feats).all()

        t = time.perf_counter()
        out_dir = os.path.join(tmp, "normalized")
        os.makedirs(out_dir)
        F.thread_map(lambda a: F.imwrite(*a), [(os.path.join(out_dir, "img_%05d.png" % i), im) for i, im in enumerate(small)])
        mm = np.memmap(os.path.join(tmp, "set_imgs.dat"), np.uint8, "w+", shape=small.shape)
        mm[:] = small
        mm.flush()
        note("write PNG 256^2 + memmap            " + rate(len(small), time.perf_counter() - t))
    if args.out:
        with open(args.out, "a") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
