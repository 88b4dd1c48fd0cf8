#!/usr/bin/env python
"""Times the HDRI environment-map encoding (confignet_amd/hdri.py, csrc/hdri.hip) at the workload's own size on one MI355X:
synthetic 1024 x 2048 pictures -> 64 x 128, 50 components, for
  (a) a 90-rotation turntable of one picture (hdri_encoding/generate_hdri_turntable_inputs.py),
  (b) 4096 dataset samples over a pool of 16 pictures (hdri_encoding/process_hdri_metadata.py).
A timed window is a BATCH of back-to-back launches of one stage between two device events, sized to last about --window-ms (a
single 16 us launch between two events measures the events); the figure is window / launches, so it holds the launch cost and the
wrapper's output allocation (caching allocator) as a user pays them.  Median, min and max over --reps windows after --warmup
untimed ones, one process.  Two byte counts per stage, both computed here from the shapes:
  touched  what the kernel's loads and stores add up to (a sample of the horizontal pass reads its picture's reduced copy) -> an
           EFFECTIVE rate; re-reads of a resident buffer come from the caches, so it is not an HBM rate;
  hbm      what must cross HBM at least once (every distinct operand once, the result once) -> floor = hbm / 6.3 TB/s, and
           floor / time is the share of the streaming rate a float4 copy reaches.  Buffers that repeated launches leave in
           the 256 MiB Infinity Cache make that share an upper estimate for a cold call.
Host <-> device copies are timed with a host clock around a synchronise.  Needs a GPU: there is nothing to measure without one.

    python scripts/hdri_bench.py [--reps 20] [--warmup 3] [--window-ms 2] > profiles/hdri_encoding.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from confignet_amd import hdri, ops  # noqa: E402

H, W, OH, OW, K = 1024, 2048, 64, 128, 50
HBM_GBS = 6300.0          # achievable streaming rate of the part (float4 copy), the yardstick of the "share" column


WINDOW_MS = 2.0


def device_ms(fn, reps, warmup):
    """(median, min, max) ms per launch and the launches per window."""
    def window(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(count):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    window(3)
    torch.cuda.synchronize()
    count = int(min(1000, max(1, round(WINDOW_MS / max(window(10) / 10, 1e-4)))))
    for _ in range(warmup):
        window(count)
    times = [window(count) / count for _ in range(reps)]
    return statistics.median(times), min(times), max(times), count


def host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return statistics.median(times), min(times), max(times), 1


def line(stage, ms, touched, hbm=None):
    med, lo, hi, count = ms
    text = "  %-34s %9.4f ms (min %8.4f max %8.4f, %4d per window)  touched %8.1f MB -> %7.1f GB/s effective" \
        % (stage, med, lo, hi, count, touched / 1e6, touched / med / 1e6)
    if hbm is not None:
        floor = hbm / HBM_GBS / 1e6
        text += "; hbm %7.1f MB, floor %.4f ms = %4.1f%% of the time" % (hbm / 1e6, floor, 100 * floor / med)
    print(text)


def synthetic_model(rng):
    model = hdri.HDRIModelPCA((OH, OW), 5)
    pca = hdri.PCAResult()
    f = OH * OW * 3
    pca.mean_ = rng.uniform(0.2, 1.5, f).astype(np.float32)
    pca.components_ = (rng.standard_normal((K, f)) / np.sqrt(f)).astype(np.float32)
    pca.explained_variance_ = np.sort(rng.uniform(0.5, 40.0, K))[::-1].astype(np.float32)
    pca.explained_variance_ratio_ = (pca.explained_variance_ / pca.explained_variance_.sum()).astype(np.float32)
    pca.singular_values_ = np.sqrt(pca.explained_variance_ * 79).astype(np.float32)
    pca.noise_variance_, pca.n_components_, pca.n_samples_, pca.n_features_ = np.float32(0.1), K, 80, f
    model.pca_model = pca
    return model


def scenario(title, model, pool, idx, rotations, reps, warmup):
    n, p = len(idx), len(pool)
    print("%s: pool of %d picture(s) %d x %d x 3 fp32, %d samples -> %d x %d, %d components" % (title, p, H, W, n, OH, OW, K))
    dev = torch.device("cuda")
    proj = model._projection()
    pool_images, image_idx, shifts = model._check_pool(pool, idx, rotations)
    y0, wy, x0, wx = model._tables(H, W)
    d_pool = torch.as_tensor(pool_images, device=dev)
    d_idx, d_shift = torch.as_tensor(image_idx, device=dev), torch.as_tensor(shifts, device=dev)
    v = ops.hdri_rows_v(d_pool, y0, wy, OH)
    rows = ops.hdri_rows_h(v, d_idx, d_shift, x0, wx, OW, proj["mean"]).reshape(n, -1)
    emb = ops.gemm(rows, proj["whiten"], trans_b=True)
    f = OH * OW * 3
    line("upload of the pool (host -> device)", host_ms(lambda: torch.as_tensor(pool_images, device=dev), max(3, reps // 4), 1), p * H * W * 12)
    line("cn_hdri_rows_v", device_ms(lambda: ops.hdri_rows_v(d_pool, y0, wy, OH), reps, warmup), p * (H + OH) * W * 12, p * (H + OH) * W * 12)
    line("cn_hdri_rows_h (mean subtracted)", device_ms(lambda: ops.hdri_rows_h(v, d_idx, d_shift, x0, wx, OW, proj["mean"]), reps, warmup),
         n * OH * W * 12 + n * f * 4 + f * 4, len(set(image_idx.tolist())) * OH * W * 12 + n * f * 4 + f * 4)
    gemm_bytes = n * f * 4 + K * f * 4 + n * K * 4
    line("cn_gemm (rows x whitened basis)", device_ms(lambda: ops.gemm(rows, proj["whiten"], trans_b=True), reps, warmup), gemm_bytes, gemm_bytes)
    line("download of the embeddings", host_ms(lambda: emb.cpu(), reps, warmup), n * K * 4)
    med, lo, hi, _ = host_ms(lambda: model.transform_indexed(pool, idx, rotations), max(3, reps // 4), 1)
    print("  %-34s %9.3f ms  (min %8.3f  max %8.3f)  end to end from host arrays, %.3f ms per sample" % ("transform_indexed", med, lo, hi, med / n))
    # the form the reference computes: every sample reads a whole picture
    print("  per-sample form would read %.1f MB per sample (%.1f GB in all) instead of %.1f MB per picture once + %.2f MB per sample\n"
          % (H * W * 12 / 1e6, n * H * W * 12 / 1e9, H * W * 12 / 1e6, OH * W * 12 / 1e6))
    return emb


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=2.0, help="length a timed window of back-to-back launches is sized to")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "hdri_bench.py measures on the GPU"
    global WINDOW_MS
    WINDOW_MS = args.window_ms
    rng = np.random.default_rng(0)
    model = synthetic_model(rng)
    pool = np.exp(rng.standard_normal((16, H, W, 3), dtype=np.float32))
    print("HDRI encoding on %s, torch %s; per-launch medians over %d windows of ~%.1f ms of back-to-back launches after %d warm-up windows, one process"
          % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.window_ms, args.warmup))
    print("touched: bytes the loads and stores add up to (effective rate, caches included); hbm: bytes that must cross HBM once, floor at %.1f TB/s\n"
          % (HBM_GBS / 1e3))
    scenario("(a) turntable", model, pool[:1], np.zeros(90, np.int64), np.linspace(-180, 180, 90), args.reps, args.warmup)
    scenario("(b) dataset metadata", model, pool, rng.integers(0, 16, 4096), rng.uniform(-180, 180, 4096), args.reps, args.warmup)
    x = torch.as_tensor(rng.standard_normal((4096, K)).astype(np.float32), device="cuda")
    print("inverse_transform of 4096 embeddings")
    y = ops.gemm(x, model._projection()["colour"], bias=model._projection()["mean"])
    f = OH * OW * 3
    inv_bytes = 4096 * K * 4 + K * f * 4 + f * 4 + 4096 * f * 4
    line("cn_gemm (+ mean)", device_ms(lambda: ops.gemm(x, model._projection()["colour"], bias=model._projection()["mean"]), args.reps, args.warmup),
         inv_bytes, inv_bytes)
    line("cn_exp2m1", device_ms(lambda: ops.exp2m1(y), args.reps, args.warmup), 2 * 4096 * f * 4, 2 * 4096 * f * 4)


if __name__ == "__main__":
    main(sys.argv[1:])
