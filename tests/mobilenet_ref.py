"""float64 torch-CPU statement of the CelebA attribute classifier: keras MobileNetV2(alpha 1.0, include_top=False) ->
GlobalAveragePooling2D -> BatchNormalization -> Dropout (inference: identity) -> Dense(sigmoid), written out layer by layer
from the published architecture with every padding explicit.  Weights: the Keras get_weights() list (per layer: kernel |
gamma, beta, moving_mean, moving_variance)."""
import torch
import torch.nn.functional as F

BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
EPS = 1e-3


def weight_shapes(n_attributes=None):
    shapes = [(3, 3, 3, 32)] + [(32,)] * 4
    cin = 32
    for t, c, n, s in BLOCKS:
        for i in range(n):
            if t != 1:
                shapes += [(1, 1, cin, cin * t)] + [(cin * t,)] * 4
            shapes += [(3, 3, cin * t, 1)] + [(cin * t,)] * 4
            shapes += [(1, 1, cin * t, c)] + [(c,)] * 4
            cin = c
    shapes += [(1, 1, 320, 1280)] + [(1280,)] * 4
    if n_attributes is not None:
        shapes += [(1280,)] * 4 + [(1280, n_attributes), (n_attributes,)]
    return shapes


def _pad_s2(e):
    """ZeroPadding2D(correct_pad(x, 3)) in front of a stride-2 3x3 layer: (0, 1) for an even extent, (1, 1) for an odd one"""
    return (0, 1) if e % 2 == 0 else (1, 1)


def _bn(x, gamma, beta, mean, var):                   # x NCHW
    sh = (1, -1, 1, 1)
    return (x - mean.view(sh)) / torch.sqrt(var.view(sh) + EPS) * gamma.view(sh) + beta.view(sh)


def _conv(x, k, stride=1, groups=1):
    """x NCHW, k Keras (kh, kw, cin / groups or c, cout or 1); padding applied by the caller"""
    if groups > 1:
        w = k.permute(2, 3, 0, 1)                       # (c, 1, 3, 3)
    else:
        w = k.permute(3, 2, 0, 1)
    return F.conv2d(x, w, stride=stride, groups=groups)


def base_forward(ws, x):
    """ws: float64 tensors of the base (260); x (N, H, W, 3) preprocessed -> (N, 1280, h, w) after out_relu (NCHW)"""
    it = iter(ws)

    def take(n):
        return [next(it) for _ in range(n)]

    x = x.permute(0, 3, 1, 2)
    k, = take(1)
    ph, pw = _pad_s2(x.shape[2]), _pad_s2(x.shape[3])
    x = torch.clamp(_bn(_conv(F.pad(x, (pw[0], pw[1], ph[0], ph[1])), k, 2), *take(4)), 0, 6)          # Conv1
    cin = 32
    for t, c, n, s in BLOCKS:
        for i in range(n):
            stride = s if i == 0 else 1
            inp = x
            if t != 1:
                k, = take(1)
                x = torch.clamp(_bn(_conv(x, k), *take(4)), 0, 6)                                         # expand
            k, = take(1)
            if stride == 2:
                ph, pw = _pad_s2(x.shape[2]), _pad_s2(x.shape[3])
            else:
                ph = pw = (1, 1)                                                                          # "same", k 3, s 1
            x = torch.clamp(_bn(_conv(F.pad(x, (pw[0], pw[1], ph[0], ph[1])), k, stride, groups=x.shape[1]), *take(4)), 0, 6)
            k, = take(1)
            x = _bn(_conv(x, k), *take(4))                                                                # project (linear)
            if stride == 1 and cin == c:
                x = x + inp
            cin = c
    k, = take(1)
    x = torch.clamp(_bn(_conv(x, k), *take(4)), 0, 6)                                                     # Conv_1, out_relu
    assert next(it, None) is None
    return x


def classifier_forward(ws, x):
    """ws: the 266 float64 tensors; x (N, H, W, 3) preprocessed -> (probabilities, logits), (N, n_attributes) each"""
    f = base_forward(ws[:-6], x).mean(dim=(2, 3))
    gamma, beta, mean, var, kernel, bias = ws[-6:]
    z = (f - mean) / torch.sqrt(var + EPS) * gamma + beta
    logits = z @ kernel + bias
    return torch.sigmoid(logits), logits


def bilinear_half_pixel(x, oh, ow):
    """cv2.resize INTER_LINEAR statement on (N, H, W, C) float64: source coordinate (o + 0.5) in / out - 0.5 clamped to
    [0, in - 1], linear in y and x"""
    n, h, w, c = x.shape

    def axis(o, i):
        src = torch.clamp((torch.arange(o, dtype=torch.float64) + 0.5) * (i / o) - 0.5, 0, i - 1)
        lo = torch.floor(src).long()
        hi = torch.clamp(lo + 1, max=i - 1)
        return lo, hi, src - lo
    y0, y1, fy = axis(oh, h)
    x0, x1, fx = axis(ow, w)
    top = x[:, y0][:, :, x0] * (1 - fx)[None, None, :, None] + x[:, y0][:, :, x1] * fx[None, None, :, None]
    bot = x[:, y1][:, :, x0] * (1 - fx)[None, None, :, None] + x[:, y1][:, :, x1] * fx[None, None, :, None]
    return top * (1 - fy)[None, :, None, None] + bot * fy[None, :, None, None]
