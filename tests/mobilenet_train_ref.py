"""torch-CPU statement of TRAINING the CelebA attribute classifier (tests/mobilenet_ref.py states inference): MobileNetV2 with
batch statistics, the head (pool, BatchNormalization on (N, 1280), inverted dropout with a GIVEN mask, Dense), the
binary cross-entropy taken back to the logits, the moving-statistic updates and one Keras Adam step.  Written for any float
type: float64 is the reference, float32 the yardstick of what the arithmetic costs.  ReLU6 decisions can be FORCED (a list of
boolean masks, one per ReLU6 in forward order): the value stays clamp(x, 0, 6), the derivative is the mask."""
import torch
import torch.nn.functional as F

from tests.mobilenet_ref import BLOCKS, EPS, _conv, _pad_s2

MOMENTUM = 0.99


def relu6(x, mask=None):
    y = torch.clamp(x, 0, 6)
    if mask is None:
        return y
    lin = x * mask.to(x.dtype).reshape(x.shape)
    return lin + (y - lin).detach()


def bn_train(x, gamma, beta, eps=EPS):
    """x (N, C, ...) -> (y, batch mean, biased batch variance) over every axis but 1"""
    dims = [d for d in range(x.dim()) if d != 1]
    sh = [1, -1] + [1] * (x.dim() - 2)
    mean = x.mean(dim=dims)
    var = ((x - mean.view(sh)) ** 2).mean(dim=dims)
    y = (x - mean.view(sh)) * torch.rsqrt(var.view(sh) + eps) * gamma.view(sh) + beta.view(sh)
    return y, mean, var


def triple(x, k, gamma, beta, kind, stride, act, mask=None, stats=None):
    """Conv2D / DepthwiseConv2D (bias-free, TF "same") -> BatchNormalization (training) [-> ReLU6] on NCHW x.
    mask: NHWC-flattened forced ReLU6 decisions.  stats: a list that receives (mean, var, rows)."""
    kh = k.shape[0]
    if kh == 3:
        ph, pw = (_pad_s2(x.shape[2]), _pad_s2(x.shape[3])) if stride == 2 else ((1, 1), (1, 1))
        x = F.pad(x, (pw[0], pw[1], ph[0], ph[1]))
    z = _conv(x, k, stride, groups=x.shape[1] if kind == "dw" else 1)
    y, mean, var = bn_train(z, gamma, beta)
    if stats is not None:
        stats.append((mean.detach(), var.detach(), z.numel() // z.shape[1]))
    if act:
        if mask is not None:
            n, c, h, w = y.shape
            mask = mask.reshape(n, h, w, c).permute(0, 3, 1, 2)
        y = relu6(y, mask)
    return y


def base_forward_train(ws, x, masks=None, stats=None):
    """ws: the base's 260 tensors (moving statistics are not read); x (N, H, W, 3) -> (N, 1280, h, w)"""
    it = iter(ws)
    mk = iter(masks) if masks is not None else None

    def run(x, kind, stride, act):
        k, gamma, beta, _, _ = [next(it) for _ in range(5)]
        return triple(x, k, gamma, beta, kind, stride, act, next(mk) if (mk is not None and act) else None, stats)

    x = run(x.permute(0, 3, 1, 2), "conv", 2, True)
    cin = 32
    for t, c, n, s in BLOCKS:
        for i in range(n):
            stride = s if i == 0 else 1
            inp = x
            if t != 1:
                x = run(x, "conv", 1, True)
            x = run(x, "dw", stride, True)
            x = run(x, "conv", 1, False)
            if stride == 1 and cin == c:
                x = x + inp
            cin = c
    x = run(x, "conv", 1, True)
    assert next(it, None) is None and (mk is None or next(mk, None) is None)
    return x


def classifier_forward_train(ws, x, dropout_mask, masks=None, stats=None):
    """ws: the 266 tensors; -> logits (N, A).  stats receives the base's 52 entries and the head's (biased variance)."""
    f = base_forward_train(ws[:-6], x, masks, stats).mean(dim=(2, 3))
    gamma, beta, _, _, kernel, bias = ws[-6:]
    z, mean, var = bn_train(f, gamma, beta)
    if stats is not None:
        stats.append((mean.detach(), var.detach(), f.shape[0]))
    return (z * dropout_mask.to(z.dtype)) @ kernel + bias


def bce_on_logits(z, t):
    return (torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean()


def moving_update(moving, value, momentum=MOMENTUM):
    """Keras _assign_moving_average: variable -= (variable - value) (1 - momentum)"""
    return moving - (moving - value) * (1.0 - momentum)


def bessel(var, rows):
    """the fused path's variance for the moving average: M / (M - 1) times the biased one"""
    return var * (rows / (rows - 1.0))


def moving_stats_after(ws, stats):
    """[(moving mean, moving variance)] of the 52 base layers (Bessel-corrected variance) and the head (biased) after one pass"""
    olds = [(ws[i + 3], ws[i + 4]) for i in range(0, 260, 5)] + [(ws[262], ws[263])]
    out = []
    for j, ((mm, mv), (mean, var, rows)) in enumerate(zip(olds, stats)):
        v = bessel(var, rows) if j < 52 else var
        out.append((moving_update(mm, mean), moving_update(mv, v)))
    return out


def adam_step(theta, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """Keras Adam: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); theta -= lr_t m / (sqrt(v) + eps)"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    return theta - lr_t * m / (v.sqrt() + eps), m, v
