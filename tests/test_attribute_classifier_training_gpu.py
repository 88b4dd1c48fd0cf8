"""Training the CelebA attribute classifier on the HIP kernels (metrics/mobilenet_v2.py: forward_train, metrics/
celeba_attribute_prediction.py: forward_train / train_on_batch / train, train_attribute_classifier.py) against the float64
statement tests/mobilenet_train_ref.py.

1. Whole-network gradient at 64 x 64 (final map 2 x 2), batch 4, 3 attributes, seeded weights, a given dropout mask: the loss and
   the gradient of every trainable tensor (156 of the base, 4 of the head).  The ReLU6 decisions of the product's backward pass
   are logged (ops.branch_log, entries "relu6") and FORCED in both CPU evaluations, so the three differ by rounding only.  Bound
   per tensor: relative L2 error at most MULT = 32 times that of float32 torch-CPU autograd of the same statement against
   float64; the moving statistics after the pass at the same multiple of their float32 yardstick.
2. Adam: the product's own gradient through the float64 Keras-Adam statement; weights after one train_on_batch within 4 ulp of
   fp32 at each tensor's largest magnitude (the update is ~lr = 1e-3 next to weights of 0.1 .. 1: a wrong rule -- epsilon inside
   the root, a missing bias correction -- moves a tensor by 1e-4 .. 1e-3 of that, the kernel's fp32 constants by ~1e-8).
3. train() on a synthetic data set whose two attributes are functions of the picture: files, logs, a falling loss, the
   checkpoint predicting exactly what the in-memory model predicts (trained moving statistics reach the folded inference
   path), bit-identical weights of two deterministic runs.
4. The command line in a child process.
Set ATTRIBUTE_CLASSIFIER_TRAINING_ERRORS to a path to get the measured ratios (profiles/attribute_classifier_training_errors.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mobilenet_train_ref as TR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULT = 32.0
N_ATTR = 3


def _net(seed=1):
    """a classifier at 64 x 64 with every BatchNormalization parameter and moving statistic moved off its default"""
    from confignet_amd.metrics.celeba_attribute_prediction import AttributeClassifierNet
    net = AttributeClassifierNet((64, 64, 3), N_ATTR, seed=seed)
    rng = np.random.default_rng(seed + 100)
    ws = net.get_weights()
    for i in list(range(0, 260, 5)) + [259]:                     # the 52 layers of the base, then the head (gamma at 260)
        c = ws[i + 1].shape[0]
        ws[i + 1] = (1.0 + 0.1 * rng.standard_normal(c)).astype(np.float32)          # gamma
        ws[i + 2] = (0.1 * rng.standard_normal(c)).astype(np.float32)                # beta
        ws[i + 3] = (0.1 * rng.standard_normal(c)).astype(np.float32)                # moving mean
        ws[i + 4] = (1.0 + 0.5 * rng.random(c)).astype(np.float32)                   # moving variance
    ws[-1] = (0.1 * rng.standard_normal(N_ATTR)).astype(np.float32)
    net.set_weights(ws)
    return net, ws


def _batch(seed=5, n=4):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, 64, 64, 3)).astype(np.float32)
    t = rng.integers(0, 2, (n, N_ATTR)).astype(np.float32)
    mask = ((rng.random((n, 1280)) >= 0.5) * 2.0).astype(np.float32)
    return x, t, mask


def _trainable_positions():
    pos = []
    for i in range(0, 260, 5):
        pos += [i, i + 1, i + 2]
    return pos + [260, 261, 264, 265]


def _cpu_gradients(ws, x, t, mask, relu_masks, dtype):
    """(loss, gradients of the 160 trainable tensors, moving statistics after the pass) of the statement in `dtype`"""
    ts = [torch.tensor(w, dtype=dtype) for w in ws]
    pos = _trainable_positions()
    for i in pos:
        ts[i].requires_grad_(True)
    stats = []
    logits = TR.classifier_forward_train(ts, torch.tensor(x, dtype=dtype), torch.tensor(mask, dtype=dtype), relu_masks, stats)
    loss = TR.bce_on_logits(logits, torch.tensor(t, dtype=dtype))
    grads = torch.autograd.grad(loss, [ts[i] for i in pos])
    moving = TR.moving_stats_after([w.detach() for w in ts], stats)
    return loss.detach(), grads, moving


def _rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).norm()) / max(float(ref.norm()), 1e-300)


def _rel_max(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def test_whole_network_gradient_against_float64():
    from confignet_amd import ops
    from confignet_amd.metrics.celeba_attribute_prediction import bce_on_logits
    net, ws = _net()
    x, t, mask = _batch()
    params = net.trainable_weights
    assert len(params) == 160 and len(net.base.trainable_weights) == 156
    with ops.branch_log() as log:
        logits = net.forward_train(x, mask)
        loss = bce_on_logits(logits, net.head_net.to_device(t))
        grads = torch.autograd.grad(loss, params)
    assert all(kind == "relu6" for kind, _ in log) and len(log) == 35
    relu_masks = [m for _, m in log][::-1]                      # logged by the backward pass: last layer first
    loss64, g64, mov64 = _cpu_gradients(ws, x, t, mask, relu_masks, torch.float64)
    loss32, g32, mov32 = _cpu_gradients(ws, x, t, mask, relu_masks, torch.float32)
    rows, failed = [], []

    def note(name, err, yard):
        rows.append((name, yard, err, err / yard if yard else (float("inf") if err else 0.0)))
        print("%s: yardstick %.3e observed %.3e" % (name, yard, err))
        if not err <= MULT * yard:
            failed.append("%s: error %.3e, yardstick %.3e" % (name, err, yard))

    note("loss", abs(float(loss.detach()) - float(loss64)) / abs(float(loss64)), abs(float(loss32) - float(loss64)) / abs(float(loss64)))
    names = ["w%03d" % i for i in _trainable_positions()]
    for name, p, g, a, b in zip(names, params, grads, g64, g32):
        assert tuple(g.shape) == tuple(p.shape) and bool(torch.isfinite(g).all()), name
        note("grad " + name + " " + "x".join(map(str, p.shape)), _rel_l2(g, a), _rel_l2(b, a))
    after = net.get_weights()
    for j, ((mm64, mv64), (mm32, mv32)) in enumerate(zip(mov64, mov32)):
        i = 5 * j + 3 if j < 52 else 262
        note("moving mean %d" % j, _rel_max(torch.tensor(after[i]), mm64), _rel_max(mm32, mm64))
        note("moving var %d" % j, _rel_max(torch.tensor(after[i + 1]), mv64), _rel_max(mv32, mv64))
    path = os.environ.get("ATTRIBUTE_CLASSIFIER_TRAINING_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%-44s %10s %10s %8s\n" % ("whole network (4, 64, 64, 3), 3 attributes", "yardstick", "observed", "ratio"))
            for r in rows:
                f.write("%-44s %10.2e %10.2e %8.2f\n" % r)
    assert not failed, "; ".join(failed)


def test_adam_step_on_the_products_own_gradient():
    from confignet_amd.optim import Adam
    net, ws = _net()
    x, t, mask = _batch()
    opt = Adam(lr=1e-3)
    net.train_on_batch(x, t, opt, dropout_mask=mask)
    torch.cuda.synchronize()
    params = net.trainable_weights
    after = net.get_weights()
    assert opt.iterations == 1
    visible = 0
    for i, p in zip(_trainable_positions(), params):
        g = p.grad.detach().double().cpu()
        theta0 = torch.tensor(ws[i], dtype=torch.float64)
        want, _, _ = TR.adam_step(theta0, g, torch.zeros_like(g), torch.zeros_like(g), 1, lr=1e-3)
        assert float(g.abs().max()) > 0, i
        tol = 4.0 * float(np.spacing(np.float32(want.abs().max())))
        err = float((torch.tensor(after[i], dtype=torch.float64) - want).abs().max())
        assert err <= tol, "weight %d: %.3e off after the step, 4 ulp = %.3e" % (i, err, tol)
        visible += float((want - theta0).abs().max()) > 50 * tol
    # the step is visible at this tolerance on all but the tensors whose gradient is rounding noise around an exact zero: the beta
    # of a linear projection feeds only 1 x 1 convolutions with batch normalisation behind them, which remove a per-channel shift
    assert visible >= 160 - 17 - 1, visible
    for i in (3, 4, 258, 259, 262, 263):                                                                # moving statistics moved, too
        assert not np.array_equal(after[i], ws[i])


class _Faces:
    """64 pictures at 64 x 64 whose two attributes are functions of the picture"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (64, 1, 1, 3))
        tilt = rng.integers(-60, 61, (64, 1, 1, 1)) * np.where(np.arange(64) < 32, 1, -1)[None, None, :, None]
        self.imgs = np.clip(base + tilt + rng.integers(-10, 11, (64, 64, 64, 3)), 0, 255).astype(np.uint8)
        red = self.imgs[..., 0].mean((1, 2)) > 128
        left = self.imgs[:, :, :32].mean((1, 2, 3)) > self.imgs[:, :, 32:].mean((1, 2, 3))
        self.attributes = [{"Red": float(r), "Left": float(l)} for r, l in zip(red, left)]

    def get_attribute_values(self, sample_idxs, attribute_names):
        return np.array([[self.attributes[i][a] for a in attribute_names] for i in sample_idxs])


def _train_run(out, deterministic=False):
    from confignet_amd import ops
    from confignet_amd.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier
    cfg = json.loads(json.dumps(DEFAULT_CONFIG))
    cfg.update(input_shape=[64, 64, 3], predicted_attributes=["Left", "Red"], batch_size=8)
    ops.set_deterministic(deterministic)
    try:
        np.random.seed(0)
        clf = CelebaAttributeClassifier(cfg, seed=3)
        clf.train(_Faces(1), _Faces(2), str(out), n_epochs=2, steps_per_epoch=10)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    return clf


def test_training_links_to_inference(tmp_path):
    from confignet_amd.metrics.celeba_attribute_prediction import CelebaAttributeClassifier
    data = _Faces(1)
    assert 8 < sum(a["Red"] for a in data.attributes) < 56 and 8 < sum(a["Left"] for a in data.attributes) < 56
    clf = _train_run(tmp_path / "a", deterministic=True)
    for name in ("checkpoints/0000.json", "checkpoints/0000.npy", "checkpoints/0001.json", "checkpoints/0001.npy", "logs.txt"):
        assert os.path.exists(tmp_path / "a" / name), name
    assert os.listdir(tmp_path / "a" / "best_model")
    assert not os.path.exists(tmp_path / "a" / "losses.png")
    header = open(tmp_path / "a" / "logs.txt").readline()
    assert header.strip("# \n").split("\t") == ["loss", "binary_accuracy", "val_loss", "val_binary_accuracy"]
    table = np.loadtxt(tmp_path / "a" / "logs.txt")
    assert table.shape == (2, 4) and np.isfinite(table).all()
    assert list(clf.logs) == ["loss", "binary_accuracy", "val_loss", "val_binary_accuracy"]
    assert clf.logs["loss"][1] < clf.logs["loss"][0]
    # the last checkpoint predicts exactly what the trained model in memory predicts.  Compared in deterministic mode: in the
    # default mode the inference convolutions split their reductions over atomics, and the SAME model predicting the same
    # pictures twice differs in the last bit (measured: 2.4e-7), so "exactly" has a meaning only there.
    from confignet_amd import ops
    imgs = _Faces(2).imgs[:40]
    loaded = CelebaAttributeClassifier.load(str(tmp_path / "a" / "checkpoints" / "0001.json"))
    fresh = CelebaAttributeClassifier(clf.config, seed=3)
    ops.set_deterministic(True)
    try:
        mem = clf.predict_attributes(imgs)
        assert np.array_equal(loaded.predict_attributes(imgs), mem)
        assert not np.allclose(fresh.predict_attributes(imgs), mem, atol=1e-3)
    finally:
        ops.set_deterministic(False)
    w = clf.classifier.get_weights()
    w0 = fresh.classifier.get_weights()
    assert not np.array_equal(w[3], w0[3]) and not np.array_equal(w[262], w0[262])      # trained moving statistics are in the file
    assert all(np.array_equal(a, b) for a, b in zip(w, list(np.load(tmp_path / "a" / "checkpoints" / "0001.npy", allow_pickle=True))))
    # deterministic mode: a second run writes the same bits
    clf2 = _train_run(tmp_path / "b", deterministic=True)
    assert all(np.array_equal(a, b) for a, b in zip(w, clf2.classifier.get_weights()))
    assert clf2.logs == clf.logs


def test_training_command_line(tmp_path):
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    faces = _Faces(4)
    for name in ("train", "val"):
        ds = NeuralRendererDataset(img_shape=(64, 64, 3))
        faces.imgs.tofile(str(tmp_path / (name + "_imgs.dat")))
        ds.imgs_memmap_filename, ds.imgs_memmap_shape, ds.imgs_memmap_dtype = name + "_imgs.dat", faces.imgs.shape, "uint8"
        ds.attributes = [dict(a, Wearing_Necktie=0.0) for a in faces.attributes]
        ds.save(str(tmp_path / (name + ".pck")))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "train_attribute_classifier.py"), "--training_set_path", str(tmp_path / "train.pck"),
           "--validation_set_path", str(tmp_path / "val.pck"), "--output_dir", str(out), "--n_epochs", "1", "--steps_per_epoch", "2",
           "--batch_size", "8"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out / "checkpoints" / "0000.json") as fp:
        meta = json.load(fp)
    assert meta["config"]["predicted_attributes"] == ["Left", "Red"] and meta["config"]["batch_size"] == 8
    assert meta["logs"] == {}                                  # (the reference saves the checkpoint before it appends the epoch's logs)
    with open(out / "best_model" / "0000.json") as fp:
        assert len(json.load(fp)["logs"]["loss"]) == 1
    assert np.loadtxt(out / "logs.txt").shape == (4,)
