"""MobileNetV2 feature network (keras.applications.MobileNetV2(alpha=1.0, include_top=False) [TF-2.1; keras_applications
mobilenet_v2.py, restated from the published architecture, Sandler et al. 2018]) on the HIP kernels: the base of the CelebA
attribute classifier (celeba_attribute_prediction.py).

Every Conv2D / DepthwiseConv2D (bias-free) -> BatchNormalization(eps 1e-3) [-> ReLU(6.)] triple is ONE launch: the
inference-mode normalisation folded into the filter and a bias, ReLU6 in the epilogue.  The full convolutions (Conv1, the 1x1
expand / project convolutions, Conv_1) run on `ops.conv_fwd`, the depthwise 3x3 layers on `ops.dwconv3x3_fwd`, and the residual
`Add` of a block sits in the epilogue of its projection (`ops.conv_fwd_res`).  Weights are held in the Keras `get_weights()`
order (per layer in `model.layers` order: kernel | gamma, beta, moving_mean, moving_variance): 260 arrays, 2 257 984 parameters.
Without a weights file the network is He-initialised (seeded).

Training (`forward_train`, for CelebaAttributeClassifier.train): the same graph with batch statistics, nothing folded.  Each
triple is one `ConvBnActFn` with a hand-written backward: `ops.conv_fwd` / `ops.dwconv3x3_fwd`, then training-mode
BatchNormalization as one reduce and one apply pass each way (`ops.bn_train_fwd` / `ops.bn_train_bwd`), then
`ops.conv_dgrad` / `ops.conv_wgrad` or `ops.dwconv3x3_dgrad` / `ops.dwconv3x3_wgrad`.  The residual `Add` is autograd's add.
Kernels, gamma and beta are the trainable weights (156 tensors); moving mean and variance are not, and every training forward
updates them in place.  The moving statistics restate TF-2.1 Keras from its published source
(tensorflow/python/keras/layers/normalization.py; parity against executed TF is not pinned):
  - `BatchNormalizationBase.__init__`: the layer default momentum 0.99, used for every BatchNormalization here (BN_MOMENTUM).
    keras_applications/mobilenet_v2.py is remembered to pass momentum=0.999 to the base's layers; that could not be checked
    against its source here, so the layer default stands until a pin against executed TF says otherwise.
  - `_assign_moving_average`: variable -= (variable - value) * (1 - momentum), the factor taken in double, then cast.
  - `_fused_batch_norm` (4-D inputs, axis 3, the default fused=None resolves to the fused path): the variance handed to the
    moving average is the op's batch variance output, which carries Bessel's correction M / (M - 1); the normalisation itself
    uses the biased variance.
  - 2-D inputs (the classifier head's BatchNormalization on (N, 1280)) take the non-fused path (`_moments`, `nn.moments`):
    biased variance for both."""
import numpy as np
import torch
from torch.autograd import Function

from .. import ops
from ..nn import Net
from ..ops import ACT_NONE, ACT_RELU6, ConvSpec
from .inception_distance import _Graph, keras_layer_order

# inverted residual blocks: (expansion t, output channels c, repeats n, first stride s)
BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
BN_EPS = 1e-3
# momentum of every BatchNormalization's moving statistics (see the module docstring); one constant, one place to change it
BN_MOMENTUM = 0.99


def mobilenet_v2_graph():
    """Layer graph in the creation order of keras_applications/mobilenet_v2.py (alpha 1.0: every width is already a multiple
    of 8).  Pads are folded into the convolutions (TF "same" gives the ZeroPadding2D(correct_pad) pads of the stride-2 layers)
    and carry no weights, so they are left out."""
    g = _Graph()
    x = g.add("input", [], channels=3)
    x = g.add("conv", [x], filters=32, kernel=3, stride=2)                                            # Conv1
    x = g.add("relu6", [g.add("bn", [x])])
    cin = 32
    for t, c, n, s in BLOCKS:
        for i in range(n):
            stride = s if i == 0 else 1
            inp = x
            if t != 1:
                x = g.add("relu6", [g.add("bn", [g.add("conv", [x], filters=cin * t, kernel=1, stride=1)])])   # block_k_expand
            x = g.add("relu6", [g.add("bn", [g.add("dw", [x], stride=stride)])])                          # depthwise
            x = g.add("bn", [g.add("conv", [x], filters=c, kernel=1, stride=1)])                           # project (linear)
            if stride == 1 and cin == c:
                x = g.add("add", [inp, x])
            cin = c
    x = g.add("relu6", [g.add("bn", [g.add("conv", [x], filters=1280, kernel=1, stride=1)])])          # Conv_1, out_relu
    return g.layers


def mobilenet_v2_weights(rng=None, graph=None):
    """The Keras get_weights() list of the network as (name, host array) pairs, He-initialised kernels (seeded), BatchNormalization
    gamma 1, beta 0, moving mean 0, moving variance 1.  Host only: shapes and order without a device."""
    rng = rng or np.random.default_rng(0)
    graph = graph or mobilenet_v2_graph()
    chans, shapes = {}, {}
    for name, kind, ins, p in graph:                           # channel bookkeeping in creation order
        if kind == "input":
            chans[name] = p["channels"]
        elif kind == "conv":
            k = p["kernel"]
            shapes[name] = (k, k, chans[ins[0]], p["filters"])
            chans[name] = p["filters"]
        elif kind == "dw":
            shapes[name] = (3, 3, chans[ins[0]], 1)
            chans[name] = chans[ins[0]]
        else:
            chans[name] = chans[ins[0]]
    out = []
    for name, kind, ins, p in keras_layer_order(graph):
        if kind in ("conv", "dw"):
            kh, kw, ci, co = shapes[name]
            fan_in = kh * kw * (ci if kind == "conv" else 1)
            out.append((name + "_kernel", (rng.standard_normal(shapes[name]) * np.sqrt(2.0 / fan_in)).astype(np.float32)))
        elif kind == "bn":
            co = chans[name]
            out += [(name + "_gamma", np.ones(co, np.float32)), (name + "_beta", np.zeros(co, np.float32)),
                    (name + "_mean", np.zeros(co, np.float32)), (name + "_var", np.ones(co, np.float32))]
    return out


class ConvBnActFn(Function):
    """One Conv2D / DepthwiseConv2D (bias-free) -> BatchNormalization (training mode) [-> ReLU6] triple.  The moving statistics
    are updated in place by the forward pass."""

    @staticmethod
    def forward(ctx, x, k, gamma, beta, mov_mean, mov_var, kind, ksize, stride, act):
        x, k = x.contiguous(), k.contiguous()
        if kind == "dw":
            g = None
            z = ops.dwconv3x3_fwd(x, k, None, stride)
        else:
            g = ConvSpec((ksize, ksize), stride=stride).geom(tuple(x.shape), k.shape[-1])
            z = ops.conv_fwd(x, k, None, g, ACT_NONE, 0.0)
        y, saved = ops.bn_train_fwd(z, gamma, beta, mov_mean, mov_var, act, eps=BN_EPS, momentum=BN_MOMENTUM, bessel=True)
        ctx.save_for_backward(x, k, z, y if act == ACT_RELU6 else None, *saved)
        ctx.kind, ctx.g, ctx.stride, ctx.act = kind, g, stride, act
        return y

    @staticmethod
    def backward(ctx, gy):
        x, k, z, y, mean, var, r, a = ctx.saved_tensors
        gz, dgamma, dbeta = ops.bn_train_bwd(gy.contiguous(), y, z, (mean, var, r, a), ctx.act)
        gx = gk = None
        slot = ops.sink_for(k) if ctx.needs_input_grad[1] else None
        if ctx.kind == "dw":
            if ctx.needs_input_grad[0]:
                gx = ops.dwconv3x3_dgrad(gz, k, tuple(x.shape), ctx.stride)
            if ctx.needs_input_grad[1]:
                if slot is not None:
                    ops.sink_dwconv3x3_wgrad(x, gz, ctx.stride, slot)
                else:
                    gk = ops.dwconv3x3_wgrad(x, gz, ctx.stride)
        else:
            if ctx.needs_input_grad[0]:
                gx = ops.conv_dgrad(gz, k, ctx.g)
            if ctx.needs_input_grad[1]:
                if slot is not None:
                    ops.sink_conv_wgrad(x, gz, ctx.g, tuple(k.shape), slot)
                else:
                    gk = ops.conv_wgrad(x, gz, ctx.g, tuple(k.shape))
        return gx, gk, dgamma, dbeta, None, None, None, None, None, None


class MobileNetV2(Net):
    """(N, H, W, 3) preprocessed to [-1, 1], H, W >= 32 -> (N, ceil(H/32), ceil(W/32), 1280) after out_relu."""

    def __init__(self, rng=None):
        super().__init__()
        self.graph = mobilenet_v2_graph()
        self._slots = {}
        for name, a in mobilenet_v2_weights(rng, self.graph):
            i = self.add_weight(name, a, trainable=not name.endswith(("_mean", "_var")))
            layer = name.rsplit("_", 1)[0]
            if name.endswith(("_kernel", "_gamma")):
                self._slots[layer] = i
        self.finalize()
        self._folded = {}
        consumers = {}
        for name, kind, ins, p in self.graph:
            for i in ins:
                consumers.setdefault(i, []).append(name)
        self._consumers = consumers
        self._layer = {l[0]: l for l in self.graph}

    def count_params(self):
        return int(sum(w.numel() for w in self.weights))

    def _fold(self, conv_name, bn_name):
        """inference BatchNormalization(eps 1e-3) folded into the preceding bias-free (depthwise) convolution: per output
        channel a = gamma / sqrt(var + eps), w' = w a, b = beta - mean a; cached per weight epoch"""
        hit = self._folded.get(conv_name)
        if hit is not None and hit[0] == self.epoch:
            return hit[1], hit[2]
        k = self.weights[self._slots[conv_name]]
        gamma, beta, mean, var = self.weights[self._slots[bn_name]:self._slots[bn_name] + 4]
        a = gamma * torch.rsqrt(var + BN_EPS)
        w = (k * (a[:, None] if self._layer[conv_name][1] == "dw" else a)).contiguous()
        b = (beta - mean * a).contiguous()
        self._folded[conv_name] = (self.epoch, w, b)
        return w, b

    def _conv_bn(self, bn_name, vals, act, res=None):
        conv = self._layer[bn_name][2][0]
        _, kind, ins, p = self._layer[conv]
        w, b = self._fold(conv, bn_name)
        x = vals[ins[0]]
        if kind == "dw":
            return ops.dwconv3x3_fwd(x, w, b, p["stride"], act)
        g = ConvSpec((p["kernel"], p["kernel"]), stride=p["stride"]).geom(tuple(x.shape), w.shape[-1])
        if res is not None:
            return ops.conv_fwd_res(x, w, b, res, g, act)
        return ops.conv_fwd(x, w, b, g, act, 0.0)

    def __call__(self, x):
        x = self.to_device(x)
        assert x.dim() == 4 and x.shape[1] >= 32 and x.shape[2] >= 32 and x.shape[3] == 3, tuple(x.shape)
        vals = {}
        with torch.no_grad():
            for name, kind, ins, p in self.graph:
                if kind == "input":
                    vals[name] = x
                elif kind == "bn":
                    cons = [self._layer[c][1] for c in self._consumers.get(name, [])]
                    if cons == ["add"]:
                        continue                                   # evaluated at the add: residual in the projection's epilogue
                    vals[name] = self._conv_bn(name, vals, ACT_RELU6 if cons == ["relu6"] else ACT_NONE)
                elif kind == "relu6":
                    vals[name] = vals[ins[0]]                      # (in the epilogue of the launch that produced its input)
                elif kind == "add":
                    vals[name] = self._conv_bn(ins[1], vals, ACT_NONE, res=vals[ins[0]])
            return vals[self.graph[-1][0]]

    def forward_train(self, x):
        """The graph of __call__ in training mode: batch statistics, differentiable w.r.t. every kernel, gamma and beta; the
        moving statistics are updated in place (and the folded inference weights invalidated)."""
        x = self.to_device(x)
        assert x.dim() == 4 and x.shape[1] >= 32 and x.shape[2] >= 32 and x.shape[3] == 3, tuple(x.shape)
        vals = {}
        for name, kind, ins, p in self.graph:
            if kind == "input":
                vals[name] = x
            elif kind == "bn":
                cons = [self._layer[c][1] for c in self._consumers.get(name, [])]
                conv, ckind, cins, cp = self._layer[ins[0]]
                k = self.weights[self._slots[conv]]
                gamma, beta, mean, var = self.weights[self._slots[name]:self._slots[name] + 4]
                vals[name] = ConvBnActFn.apply(vals[cins[0]], k, gamma, beta, mean, var, ckind, cp.get("kernel", 3), cp["stride"],
                                               ACT_RELU6 if cons == ["relu6"] else ACT_NONE)
            elif kind == "relu6":
                vals[name] = vals[ins[0]]                          # (in the triple that produced its input)
            elif kind == "add":
                vals[name] = vals[ins[0]] + vals[ins[1]]
        self.mark_updated()                                        # moving statistics changed: the folded weights are stale
        return vals[self.graph[-1][0]]
