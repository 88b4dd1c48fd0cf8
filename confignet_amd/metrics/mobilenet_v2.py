"""MobileNetV2 feature network (keras.applications.MobileNetV2(alpha=1.0, include_top=False) [TF-2.1; keras_applications
mobilenet_v2.py, restated from the published architecture, Sandler et al. 2018]) on the HIP kernels: the base of the CelebA
attribute classifier (celeba_attribute_prediction.py).

Every Conv2D / DepthwiseConv2D (bias-free) -> BatchNormalization(eps 1e-3) [-> ReLU(6.)] triple is ONE launch: the
inference-mode normalisation folded into the filter and a bias, ReLU6 in the epilogue.  The full convolutions (Conv1, the 1x1
expand / project convolutions, Conv_1) run on `ops.conv_fwd`, the depthwise 3x3 layers on `ops.dwconv3x3_fwd`, and the residual
`Add` of a block sits in the epilogue of its projection (`ops.conv_fwd_res`).  Weights are held in the Keras `get_weights()`
order (per layer in `model.layers` order: kernel | gamma, beta, moving_mean, moving_variance): 260 arrays, 2 257 984 parameters.
Without a weights file the network is He-initialised (seeded)."""
import numpy as np
import torch

from .. import ops
from ..nn import Net
from ..ops import ACT_NONE, ACT_RELU6, ConvSpec
from .inception_distance import _Graph, keras_layer_order

# inverted residual blocks: (expansion t, output channels c, repeats n, first stride s)
BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
BN_EPS = 1e-3


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


class MobileNetV2(Net):
    """(N, H, W, 3) preprocessed to [-1, 1], H, W >= 32 -> (N, ceil(H/32), ceil(W/32), 1280) after out_relu."""

    def __init__(self, rng=None):
        super().__init__()
        self.graph = mobilenet_v2_graph()
        self._slots = {}
        for name, a in mobilenet_v2_weights(rng, self.graph):
            i = self.add_weight(name, a, trainable=False)
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
