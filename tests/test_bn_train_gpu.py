"""Training-mode BatchNormalization (ops.bn_train_fwd / ops.bn_train_bwd: cn_nc_reduce + csrc/bn_train.hip) with ReLU6 and with
no activation behind it, against float64 autograd of the statement in tests/mobilenet_train_ref.py.

Compared: y, the batch mean and (biased) variance, both moving-statistic updates (Bessel-corrected and not), gx, dgamma, dbeta.
Yardstick (as tests/test_norm_tails_gpu.py, without its caps): each quantity's error is taken relative to its own maximum and
may be at most MULT = 32 times the error of the SAME statement evaluated in float32 on the CPU.  Inputs are drawn in float32, and
the ReLU6 decisions of both CPU evaluations are taken from the product's y.  Channel 1 of every case has mean 1000 and sigma 1:
a one-pass fp32 variance s2 / m - mean^2 is rounding noise there (mean^2 = 1e6 against var = 1), so the case fails without the
second walk of cn_bn_train_coef.  Shapes: (4, 3, 5, 8) (60 rows: one slice, dead lanes), (2, 16, 16, 96) (512 rows: several
slices of the backward reduce), (32, 1, 1, 1280) (the head's extent, should a later change send it through these kernels).
Set ATTRIBUTE_CLASSIFIER_TRAINING_ERRORS to a path to get the table of measured ratios (profiles/attribute_classifier_training_errors.txt)."""
import os

import numpy as np
import pytest
import torch

from tests import mobilenet_train_ref as TR

pytestmark = pytest.mark.gpu

MULT = 32.0
SHAPES = [(4, 3, 5, 8), (2, 16, 16, 96), (32, 1, 1, 1280)]
ACT_NONE, ACT_RELU6 = 0, 4
_ROWS = []


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("ATTRIBUTE_CLASSIFIER_TRAINING_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%-44s %-12s %10s %10s %8s\n" % ("case", "quantity", "yardstick", "observed", "ratio"))
            for r in _ROWS:
                f.write("%-44s %-12s %10.2e %10.2e %8.2f\n" % r)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _statement(x, gamma, beta, gy, mm, mv, mask, dtype):
    """every compared quantity of the layer in `dtype` on the CPU; x (N, H, W, C)"""
    x, gamma, beta, gy, mm, mv = (t.to(dtype) for t in (x, gamma, beta, gy, mm, mv))
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    yl, mean, var = TR.bn_train(x.permute(0, 3, 1, 2), gamma, beta)
    y = yl if mask is None else TR.relu6(yl, mask.permute(0, 3, 1, 2))
    gx, dgamma, dbeta = torch.autograd.grad((y * gy.permute(0, 3, 1, 2)).sum(), (x, gamma, beta))
    rows = x.numel() // x.shape[-1]
    return {"y": y.permute(0, 2, 3, 1), "mean": mean, "var": var, "mov_mean": TR.moving_update(mm, mean),
            "mov_var_bessel": TR.moving_update(mv, TR.bessel(var, rows)), "mov_var_biased": TR.moving_update(mv, var),
            "gx": gx, "dgamma": dgamma, "dbeta": dbeta}


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU6], ids=["linear", "relu6"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_training_forward_and_backward(shape, act):
    from confignet_amd import ops
    c = shape[-1]
    g = torch.Generator().manual_seed(sum(shape) + act)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(*shape) * (0.5 + torch.rand(c, generator=g)) + rnd(c)
    x[..., 1] = 1000.0 + rnd(*shape[:-1])
    gamma, beta, gy = 2.0 + 0.5 * rnd(c), 2.0 + rnd(c), rnd(*shape)                   # y = 2 xh + 2: both sides of ReLU6 are hit
    mm, mv = rnd(c), 1.0 + torch.rand(c, generator=g)

    mov = [(mm.clone().cuda(), mv.clone().cuda()) for _ in range(2)]
    y, saved = ops.bn_train_fwd(x.cuda(), gamma.cuda(), beta.cuda(), mov[0][0], mov[0][1], act, bessel=True)
    ops.bn_train_fwd(x.cuda(), gamma.cuda(), beta.cuda(), mov[1][0], mov[1][1], act, bessel=False)
    gx, dgamma, dbeta = ops.bn_train_bwd(gy.cuda(), y if act == ACT_RELU6 else None, x.cuda(), saved, act)
    got = {"y": y, "mean": saved[0], "var": saved[1], "mov_mean": mov[0][0], "mov_var_bessel": mov[0][1], "mov_var_biased": mov[1][1],
           "gx": gx, "dgamma": dgamma, "dbeta": dbeta}
    mask = None
    if act == ACT_RELU6:
        mask = ((y > 0) & (y < 6)).cpu()
        assert 0.02 < float(mask.float().mean()) < 0.98 and bool((y == 6).any()) and bool((y == 0).any())
    ref = _statement(x, gamma, beta, gy, mm, mv, mask, torch.float64)
    yard = _statement(x, gamma, beta, gy, mm, mv, mask, torch.float32)
    case = "bn_train %s %s" % (shape, "relu6" if act else "linear")
    failed = []
    for k in got:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        ys, err = rel_err(yard[k], ref[k]), rel_err(got[k], ref[k])
        _ROWS.append((case, k, ys, err, err / ys if ys else float("inf") if err else 0.0))
        print("%s %s: yardstick %.3e observed %.3e" % (case, k, ys, err))
        if not err <= MULT * ys:
            failed.append("%s: error %.3e of its maximum, yardstick %.3e" % (k, err, ys))
    assert not failed, "%s: %s" % (case, "; ".join(failed))
    # a naive one-pass variance of channel 1 would be off by far more than the bound: the case is not vacuous
    s1, s2 = x[..., 1].float().sum(), (x[..., 1].float() ** 2).sum()
    m = x.numel() // c
    naive = float(s2 / m - (s1 / m) ** 2)
    assert abs(naive - float(ref["var"][1].detach())) > 1e-3 * float(ref["var"][1].detach())
