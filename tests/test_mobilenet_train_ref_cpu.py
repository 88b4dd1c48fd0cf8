"""Pins tests/mobilenet_train_ref.py (the float64 statement the GPU training tests compare against) without a GPU: its gradient
against central finite differences on a three-triple stack, the Adam step and the moving-statistic rule against values worked
out by hand; and the CPU-visible surface of the training feature (argument names, command line)."""
import inspect
import os
import subprocess
import sys

import torch

from tests import mobilenet_train_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stack(ws, x, stats=None):
    """conv 1x1 -> BN -> ReLU6, depthwise 3x3 stride 2 -> BN -> ReLU6, conv 1x1 -> BN (the inverted residual block)"""
    y = TR.triple(x.permute(0, 3, 1, 2), ws[0], ws[1], ws[2], "conv", 1, True, stats=stats)
    y = TR.triple(y, ws[3], ws[4], ws[5], "dw", 2, True, stats=stats)
    y = TR.triple(y, ws[6], ws[7], ws[8], "conv", 1, False, stats=stats)
    return y


def test_gradient_of_a_three_triple_stack_against_finite_differences():
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ws = [rnd(1, 1, 3, 8), 1 + 0.3 * rnd(8), 1.5 + rnd(8), rnd(3, 3, 8, 1), 1 + 0.3 * rnd(8), 1.5 + rnd(8), rnd(1, 1, 8, 4),
          1 + 0.3 * rnd(4), rnd(4)]
    x, t = rnd(3, 6, 6, 3), rnd(3, 4, 3, 3)
    loss = lambda ws_: (_stack(ws_, x) * t).sum()
    ps = [w.clone().requires_grad_(True) for w in ws]
    grads = torch.autograd.grad(loss(ps), ps)
    h = 1e-6
    for i, (w, gr) in enumerate(zip(ws, grads)):
        flat = w.reshape(-1)
        for j in range(0, flat.numel(), max(1, flat.numel() // 7)):          # a spread of elements of every tensor
            d = torch.zeros_like(flat)
            d[j] = h
            up = [v if k != i else (flat + d).reshape(w.shape) for k, v in enumerate(ws)]
            dn = [v if k != i else (flat - d).reshape(w.shape) for k, v in enumerate(ws)]
            fd = float(loss(up) - loss(dn)) / (2 * h)
            an = float(gr.reshape(-1)[j])
            # central differences in float64: truncation h^2 f''' and rounding eps |f| / h, both ~1e-6 of the gradient scale
            assert abs(fd - an) <= 1e-5 * max(1.0, float(gr.abs().max())), (i, j, fd, an)


def test_forced_masks_keep_the_value_and_set_the_derivative():
    x = torch.tensor([-1.0, 0.5, 3.0, 7.0], dtype=torch.float64, requires_grad=True)
    mask = torch.tensor([True, False, True, False])
    y = TR.relu6(x, mask)
    assert torch.equal(y.detach(), torch.tensor([0.0, 0.5, 3.0, 6.0], dtype=torch.float64))
    (gx,) = torch.autograd.grad(y.sum(), x)
    assert torch.equal(gx, mask.double())


def test_adam_step_and_moving_statistics_by_hand():
    # first Keras Adam step from zero moments: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1, so the update is
    # lr g / (|g| + eps sqrt(1000)) -- for g = 2, lr = 1e-3: theta - 1e-3 * 2 / (2 + 1e-7 * 31.6227766...)
    th, m, v = TR.adam_step(torch.tensor([1.0], dtype=torch.float64), torch.tensor([2.0], dtype=torch.float64),
                            torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), 1)
    assert abs(float(m) - 0.2) < 1e-15 and abs(float(v) - 0.004) < 1e-15
    assert abs(float(th) - (1.0 - 1e-3 * 2.0 / (2.0 + 1e-7 * 1000 ** 0.5))) < 1e-15
    # second step with g = -1: m = 0.18 - 0.1 = 0.08, v = 0.003996 + 0.001 = 0.004996, lr_t = 1e-3 sqrt(1 - 0.998001) / 0.19
    th2, m2, v2 = TR.adam_step(th, torch.tensor([-1.0], dtype=torch.float64), m, v, 2)
    assert abs(float(m2) - 0.08) < 1e-15 and abs(float(v2) - 0.004996) < 1e-15
    lr_t = 1e-3 * (1 - 0.999 ** 2) ** 0.5 / (1 - 0.81)
    assert abs(float(th2) - (float(th) - lr_t * 0.08 / (0.004996 ** 0.5 + 1e-7))) < 1e-15
    # moving statistics: x = (1, 2, 3, 6) has mean 3, biased variance 3.5, Bessel-corrected 14 / 3; from (0, 1) with momentum 0.99
    x = torch.tensor([1.0, 2.0, 3.0, 6.0], dtype=torch.float64).reshape(4, 1, 1, 1)
    stats = []
    TR.triple(x, torch.ones(1, 1, 1, 1, dtype=torch.float64), torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
              "conv", 1, False, stats=stats)
    mean, var, rows = stats[0]
    assert rows == 4 and abs(float(mean) - 3.0) < 1e-15 and abs(float(var) - 3.5) < 1e-15
    assert abs(float(TR.bessel(var, rows)) - 14.0 / 3.0) < 1e-14
    assert abs(float(TR.moving_update(torch.zeros(1, dtype=torch.float64), mean)) - 0.03) < 1e-15
    assert abs(float(TR.moving_update(torch.ones(1, dtype=torch.float64), TR.bessel(var, rows))) - (0.99 + 0.14 / 3.0)) < 1e-14


def test_the_training_surface_has_the_references_argument_names():
    from confignet_amd.metrics.celeba_attribute_prediction import CelebaAttributeClassifier
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(CelebaAttributeClassifier.train) == ["self", "training_set", "validation_set", "output_dir", "n_epochs", "steps_per_epoch"]
    assert sig(CelebaAttributeClassifier.sample_batch_from_dataset) == ["self", "dataset", "batch_size", "add_noise"]
    assert sig(CelebaAttributeClassifier.batch_generator) == ["self", "training_set"]
    assert sig(CelebaAttributeClassifier.callback) == ["self", "epoch", "logs", "output_dir"]
    import confignet.metrics.celeba_attribute_prediction as alias
    assert alias.CelebaAttributeClassifier is CelebaAttributeClassifier


def test_command_line_lists_the_six_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_attribute_classifier.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--training_set_path", "--validation_set_path", "--output_dir", "--n_epochs", "--steps_per_epoch", "--batch_size",
                "--ignored_attributes"):
        assert opt in r.stdout, opt
    sys.path.insert(0, ROOT)
    import train_attribute_classifier as cli
    args = cli.parse_args(["--training_set_path", "a", "--validation_set_path", "b", "--output_dir", "c"])
    assert (args.n_epochs, args.steps_per_epoch, args.batch_size) == (1000, 100, 32)
    assert args.ignored_attributes == ["Wearing_Necklace", "Wearing_Necktie"]
