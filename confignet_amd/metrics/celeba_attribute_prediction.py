"""CelebaAttributeClassifier (reference: confignet/metrics/celeba_attribute_prediction.py): the attribute classifier the
controllability metrics score images with, inference only, on the HIP kernels.

The network is keras Sequential([MobileNetV2(include_top=False), GlobalAveragePooling2D, BatchNormalization, Dropout(0.5),
Dense(n_attributes, sigmoid)]): the base is `mobilenet_v2.MobileNetV2`, the pooling one `ops.nc_reduce`, and the head's
inference-mode BatchNormalization is folded into the Dense layer, which runs as ONE `ops.gemm` with the sigmoid in its epilogue
(Dropout is the identity at inference).  Weights are the Keras `get_weights()` list of the Sequential model (the base's 260
arrays, then gamma, beta, moving_mean, moving_variance of the head's normalisation, then the Dense kernel and bias), held on
the host and uploaded when the classifier first runs; `save` / `load` read and write the reference's files.

Training the classifier (`train`, the reference's train_attribute_classifier.py) is not provided: it needs the depthwise
convolution's backward pass, training-mode BatchNormalization and dropout, none of which this package has."""
import json
import os

import numpy as np

from .mobilenet_v2 import BN_EPS, mobilenet_v2_weights

DEFAULT_CONFIG = {
    "input_shape": None,
    "predicted_attributes": None,
    "optimizer": {
        "lr": 0.001
    },
    "batch_size": 32
}

PREDICT_BATCH_SIZE = 32           # keras Model.predict's default batch


def head_weights(n_attributes, rng=None):
    """BatchNormalization (1280) defaults and a glorot-uniform Dense (1280, n_attributes) with a zero bias, Keras order."""
    rng = rng or np.random.default_rng(0)
    lim = np.sqrt(6.0 / (1280 + n_attributes))
    return [np.ones(1280, np.float32), np.zeros(1280, np.float32), np.zeros(1280, np.float32), np.ones(1280, np.float32),
            rng.uniform(-lim, lim, size=(1280, n_attributes)).astype(np.float32), np.zeros(n_attributes, np.float32)]


class AttributeClassifierNet:
    """The Sequential model: Keras-like get_weights / set_weights / count_params on a host copy of the weights, and the
    forward pass on the device (built on first use, refreshed after set_weights)."""

    def __init__(self, input_shape, n_attributes, seed=0):
        self.input_shape = tuple(int(v) for v in input_shape)
        assert len(self.input_shape) == 3 and self.input_shape[2] == 3 and min(self.input_shape[:2]) >= 32, self.input_shape
        rng = np.random.default_rng(seed)
        self._weights = [a for _, a in mobilenet_v2_weights(rng)] + head_weights(n_attributes, rng)
        self._base = None
        self._head = None               # (epoch of the base, folded Dense kernel, folded bias) on the device

    def get_weights(self):
        return [np.array(w, copy=True) for w in self._weights]

    def set_weights(self, weights):
        weights = list(weights)
        assert len(weights) == len(self._weights), "expected %d arrays, got %d" % (len(self._weights), len(weights))
        new = []
        for w, a in zip(self._weights, weights):
            a = np.asarray(a, dtype=np.float32)
            assert a.shape == w.shape, "shape mismatch %s vs %s" % (a.shape, w.shape)
            new.append(np.ascontiguousarray(a))
        self._weights = new
        if self._base is not None:
            self._base.set_weights(new[:-6])
        self._head = None

    def count_params(self):
        return int(sum(w.size for w in self._weights))

    @property
    def base(self):
        if self._base is None:
            from .mobilenet_v2 import MobileNetV2
            self._base = MobileNetV2()
            self._base.set_weights(self._weights[:-6])
        return self._base

    def _folded_head(self):
        """BatchNormalization(eps 1e-3) folded into the Dense layer: z = f a + (beta - mean a), a = gamma / sqrt(var + eps), so
        z K + c = f (a K) + ((beta - mean a) K + c)"""
        if self._head is None:
            import torch
            from .. import ops
            dev = self.base.device
            gamma, beta, mean, var, kernel, bias = (torch.as_tensor(w, device=dev) for w in self._weights[-6:])
            a = gamma * torch.rsqrt(var + BN_EPS)
            k = (kernel * a[:, None]).contiguous()
            c = ops.gemm((beta - mean * a)[None].contiguous(), kernel.contiguous(), bias=bias.contiguous())[0].contiguous()
            self._head = (k, c)
        return self._head

    def features(self, x):
        """(N, H, W, 3) preprocessed -> (N, 1280): the base and GlobalAveragePooling2D"""
        from .. import ops
        v = self.base(x)
        s1 = ops.nc_reduce(v, None, want_dot=False)[0]
        return s1.reshape(v.shape[0], v.shape[-1]) / float(v.shape[1] * v.shape[2])

    def __call__(self, x, logits=False):
        """(N, H, W, 3) preprocessed -> (N, n_attributes) probabilities (logits=True: the pre-sigmoid values)"""
        import torch
        from .. import ops
        with torch.no_grad():
            f = self.features(x)
            k, c = self._folded_head()
            return ops.gemm(f, k, bias=c, act=ops.ACT_NONE if logits else ops.ACT_SIGMOID)


class CelebaAttributeClassifier:
    def __init__(self, config, seed=0):
        self.config = config
        self.logs = {}
        self.classifier = None
        self._seed = seed
        self.initialize_dnn()

    def initialize_dnn(self):
        self.classifier = AttributeClassifierNet(self.config["input_shape"], len(self.config["predicted_attributes"]), seed=self._seed)

    def save(self, output_dir, output_filename):
        """<output_filename>.json = {"logs", "config"}; <output_filename>.npy = a dtype=object array of the Keras weight list
        (what the reference's np.save(path, model.get_weights()) writes)."""
        weights = self.classifier.get_weights()
        metadata = {"logs": self.logs, "config": self.config}
        with open(os.path.join(output_dir, output_filename + ".json"), "w") as fp:
            json.dump(metadata, fp, indent=4)
        arr = np.empty(len(weights), dtype=object)                # (numpy >= 2 refuses to build a ragged array from the list)
        for i, w in enumerate(weights):
            arr[i] = w
        np.save(os.path.join(output_dir, output_filename + ".npy"), arr)

    @classmethod
    def load(cls, file_path):
        with open(file_path, "r") as fp:
            metadata = json.load(fp)
        weights = np.load(os.path.splitext(file_path)[0] + ".npy", allow_pickle=True)
        classifier = cls(metadata["config"])
        classifier.logs = metadata["logs"]
        classifier.classifier.set_weights(list(weights))
        return classifier

    def predict_attributes(self, input_images):
        """celeba_attribute_prediction.py:129-141: float32 images are taken as [-1, 1] ((x + 1) * 127.5), other types as pixel
        values; resampled to config["input_shape"] (bilinear, half-pixel centres, as cv2.resize INTER_LINEAR -- computed in
        float for uint8 images too: cv2's 11-bit fixed-point uint8 arithmetic is not reproduced, and cv2 is not a dependency)
        when the size differs; mobilenet_v2.preprocess_input; the classifier in batches of 32.  All of that after the upload is
        one cn_image_preprocess launch per batch.  Returns (N, n_attributes) float32 probabilities."""
        import torch
        from .. import ops
        input_images = np.asarray(input_images)
        from_signed = input_images.dtype == np.float32
        if input_images.dtype not in (np.uint8, np.float32):
            input_images = input_images.astype(np.float32)
        shape = tuple(int(v) for v in self.config["input_shape"])
        net = self.classifier
        out = np.zeros((input_images.shape[0], len(self.config["predicted_attributes"])), np.float32)
        for s in range(0, input_images.shape[0], PREDICT_BATCH_SIZE):
            batch = torch.as_tensor(np.ascontiguousarray(input_images[s:s + PREDICT_BATCH_SIZE])).to(net.base.device)
            x = ops.image_preprocess(batch, shape[:2], from_signed=from_signed)
            out[s:s + PREDICT_BATCH_SIZE] = net(x).cpu().numpy()
        return out
