"""CelebaAttributeClassifier (reference: confignet/metrics/celeba_attribute_prediction.py): the attribute classifier the
controllability metrics score images with, inference and training, on the HIP kernels.

The network is keras Sequential([MobileNetV2(include_top=False), GlobalAveragePooling2D, BatchNormalization, Dropout(0.5),
Dense(n_attributes, sigmoid)]): the base is `mobilenet_v2.MobileNetV2`, the pooling one `ops.nc_reduce`, and the head's
inference-mode BatchNormalization is folded into the Dense layer, which runs as ONE `ops.gemm` with the sigmoid in its epilogue
(Dropout is the identity at inference).  Weights are the Keras `get_weights()` list of the Sequential model (the base's 260
arrays, then gamma, beta, moving_mean, moving_variance of the head's normalisation, then the Dense kernel and bias), held on
the host and uploaded when the classifier first runs; `save` / `load` read and write the reference's files.

Training (`train`, the reference's l.65-127 and train_attribute_classifier.py).  `AttributeClassifierNet.forward_train` runs
`MobileNetV2.forward_train` (batch statistics; depthwise gradients and training-mode BatchNormalization on HIP kernels), the
pooling, the head's training-mode BatchNormalization on (N, 1280) (torch: the non-fused Keras path, biased variance also for the
moving statistic, momentum 0.99), inverted Dropout(0.5) (kept units x 2; the mask from a seeded torch generator, applied with
`ops.mul`) and the Dense layer, and returns LOGITS.  The loss is what keras.losses.BinaryCrossentropy computes on a sigmoid output
in graph mode -- TF 2.1's backend.binary_crossentropy goes back to the logits when the output's op is Sigmoid --:
mean over batch and attributes of max(z, 0) - z t + log1p(exp(-|z|)), gradient (sigmoid(z) - t) / (N A); the metric is binary
accuracy at threshold 0.5.  The optimiser is Keras Adam(lr) (beta 0.9 / 0.999, eps 1e-7, bias correction in lr_t) on
`optim.Adam` / `ops.adam_step` without an EMA copy, one step counter for the base's and the head's arena.  `train` samples with
np.random as the reference does (np.random.seed governs it), draws 200 validation samples once, reports per epoch the running
means `loss` / `binary_accuracy` and `val_loss` / `val_binary_accuracy` (inference mode, batches of 32), writes
checkpoints/<epoch:04d>.json|.npy every epoch, best_model/ when val_binary_accuracy improves, and logs.txt.  The reference's
matplotlib plots (losses.png, metrics.png) are not written, as everywhere else in this package."""
import json
import os

import numpy as np
import torch

from .. import ops
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
        self._host = [a for _, a in mobilenet_v2_weights(rng)] + head_weights(n_attributes, rng)
        self._stale = False             # a training step has changed the device weights since the host copy was taken
        self._base = None
        self._head = None               # (epoch of the base, folded Dense kernel, folded bias) on the device
        self._head_net = None           # the head's six arrays as a Net (training only)
        self._dropout_rng = None
        self._seed = seed

    @property
    def _weights(self):
        """The host copy of the Keras weight list, refreshed from the device after training steps."""
        if self._stale:
            self._stale = False
            self._host = self._base.get_weights() + self._head_net.get_weights()
        return self._host

    @_weights.setter
    def _weights(self, new):
        self._host, self._stale = new, False
        if self._head_net is not None:
            self._head_net.set_weights(new[-6:])

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


    # ---- training ------------------------------------------------------------------------------------------------------
    @property
    def head_net(self):
        if self._head_net is None:
            from ..nn import Net
            base = self.base
            w = self._weights[-6:]
            net = Net()
            for name, a, tr in zip(("bn_gamma", "bn_beta", "bn_mean", "bn_var", "dense_kernel", "dense_bias"), w,
                                   (True, True, False, False, True, True)):
                net.add_weight(name, a, trainable=tr)
            net.finalize()
            assert net.device == base.device
            self._head_net = net
        return self._head_net

    @property
    def trainable_weights(self):
        """kernels, gamma and beta of the base (156 tensors), then gamma, beta, Dense kernel and bias of the head"""
        return self.base.trainable_weights + self.head_net.trainable_weights

    def draw_dropout_mask(self, n):
        """(n, 1280) inverted-dropout mask of rate 0.5: 2 where a unit is kept, else 0; from this network's seeded generator"""
        if self._dropout_rng is None:
            self._dropout_rng = torch.Generator().manual_seed(self._seed)
        return (torch.rand((n, 1280), generator=self._dropout_rng) >= 0.5).to(torch.float32) * 2.0

    def forward_train(self, x, dropout_mask=None):
        """(N, H, W, 3) preprocessed -> (N, n_attributes) LOGITS in training mode (batch statistics, dropout), differentiable
        w.r.t. `trainable_weights`; updates every moving statistic in place.  dropout_mask: (N, 1280) multipliers (0 / 2)
        instead of a drawn one."""
        from .. import functional as F
        from .mobilenet_v2 import BN_MOMENTUM
        head = self.head_net
        v = self.base.forward_train(x)
        f = F.global_avg_pool(v).reshape(v.shape[0], v.shape[-1])
        gamma, beta, mov_mean, mov_var, kernel, bias = head.weights
        mean = f.mean(0)
        var = ((f - mean) ** 2).mean(0)                              # biased: the non-fused Keras path of a 2-D input
        z = (f - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta
        with torch.no_grad():
            mov_mean.sub_((mov_mean - mean) * (1.0 - BN_MOMENTUM))
            mov_var.sub_((mov_var - var) * (1.0 - BN_MOMENTUM))
        if dropout_mask is None:
            dropout_mask = self.draw_dropout_mask(f.shape[0])
        mask = head.to_device(dropout_mask)
        assert tuple(mask.shape) == tuple(z.shape), (tuple(mask.shape), tuple(z.shape))
        d = _MaskMulFn.apply(z, mask)
        self._stale, self._head = True, None
        return F.linear(d, kernel, bias)

    def train_on_batch(self, x, targets, optimizer, dropout_mask=None):
        """One optimiser step on a batch; returns (loss, binary accuracy) as 0-d device tensors (no host synchronisation)."""
        from ..nn import backward_into_arenas
        logits = self.forward_train(x, dropout_mask)
        t = self.head_net.to_device(targets)
        loss = bce_on_logits(logits, t)
        backward_into_arenas(loss, [self.base, self.head_net])
        optimizer.apply_gradients([self.base, self.head_net])
        self._stale, self._head = True, None
        with torch.no_grad():
            return loss.detach(), binary_accuracy(logits.detach(), t)


def bce_on_logits(z, t):
    """keras.losses.BinaryCrossentropy on a sigmoid output, taken back to the logits z: mean over batch and attributes of
    max(z, 0) - z t + log1p(exp(-|z|)); gradient (sigmoid(z) - t) / (N A)."""
    return _BceLogitsFn.apply(z, t)


def binary_accuracy(z, t):
    """keras.metrics.BinaryAccuracy(threshold 0.5) from logits: sigmoid(z) > 0.5 is z > 0"""
    return ((z > 0).to(t.dtype) == t).to(z.dtype).mean()


class _MaskMulFn(torch.autograd.Function):
    """x * mask (ops.mul) with a constant mask: inverted dropout"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return ops.mul(x.contiguous(), mask)

    @staticmethod
    def backward(ctx, gy):
        (mask,) = ctx.saved_tensors
        return ops.mul(gy.contiguous(), mask), None


class _BceLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, t):
        ctx.save_for_backward(z, t)
        return (z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean()

    @staticmethod
    def backward(ctx, gout):
        z, t = ctx.saved_tensors
        return gout * (torch.sigmoid(z) - t) / z.numel(), None


N_VALIDATION_SAMPLES = 200        # celeba_attribute_prediction.py:119


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

    # ---- training (celeba_attribute_prediction.py:65-127) ---------------------------------------------------------------
    def callback(self, epoch, logs, output_dir):
        """End of an epoch: checkpoints/<epoch:04d> (saved BEFORE this epoch's logs are appended, as the reference does), the
        logs, best_model/<epoch:04d> when val_binary_accuracy is the first or beats every earlier one, logs.txt (no plots)."""
        def save_into(sub):
            os.makedirs(os.path.join(output_dir, sub), exist_ok=True)
            self.save(os.path.join(output_dir, sub), "%04d" % epoch)

        save_into("checkpoints")
        for key, value in logs.items():
            self.logs.setdefault(key, []).append(float(value))
        acc = self.logs["val_binary_accuracy"]
        if len(acc) == 1 or acc[-1] > max(acc[:-1]):
            save_into("best_model")
        table = np.stack([np.asarray(v, dtype=np.float64) for v in self.logs.values()], axis=1)
        np.savetxt(os.path.join(output_dir, "logs.txt"), table, header="\t".join(self.logs.keys()))

    def sample_batch_from_dataset(self, dataset, batch_size=None, add_noise=False):
        """(imgs, attributes): `batch_size` images drawn with replacement (np.random.randint), preprocessed as
        mobilenet_v2.preprocess_input does (x / 127.5 - 1, float32); add_noise: N(0, 0.05) on the first half of the batch."""
        batch_size = self.config["batch_size"] if batch_size is None else batch_size
        sample_idxs = np.random.randint(0, dataset.imgs.shape[0], batch_size)
        imgs = np.asarray(dataset.imgs[sample_idxs]).astype(np.float32)
        imgs /= 127.5
        imgs -= 1.0
        if add_noise:
            half = batch_size // 2
            imgs[:half] += np.random.normal(0, 0.05, imgs[:half].shape)
        return imgs, dataset.get_attribute_values(sample_idxs, self.config["predicted_attributes"])

    def batch_generator(self, training_set):
        while True:
            yield self.sample_batch_from_dataset(training_set)

    def evaluate(self, imgs, labels):
        """(loss, binary accuracy) of preprocessed images in inference mode, batches of 32, as Keras validates"""
        net = self.classifier
        loss = acc = 0.0
        for s in range(0, imgs.shape[0], PREDICT_BATCH_SIZE):
            z = net(imgs[s:s + PREDICT_BATCH_SIZE], logits=True)
            t = torch.as_tensor(np.asarray(labels[s:s + PREDICT_BATCH_SIZE], dtype=np.float32)).to(z.device)
            with torch.no_grad():
                loss += float(bce_on_logits(z, t)) * z.shape[0]
                acc += float(binary_accuracy(z, t)) * z.shape[0]
        return loss / imgs.shape[0], acc / imgs.shape[0]

    def train(self, training_set, validation_set, output_dir, n_epochs, steps_per_epoch):
        from ..optim import Adam
        optimizer = Adam(**self.config["optimizer"])
        validation_imgs, validation_labels = self.sample_batch_from_dataset(validation_set, N_VALIDATION_SAMPLES)
        batches = self.batch_generator(training_set)
        for epoch in range(n_epochs):
            loss_sum = acc_sum = None
            for _ in range(steps_per_epoch):
                imgs, attributes = next(batches)
                loss, acc = self.classifier.train_on_batch(imgs, np.asarray(attributes, dtype=np.float32), optimizer)
                loss_sum = loss if loss_sum is None else loss_sum + loss
                acc_sum = acc if acc_sum is None else acc_sum + acc
            val_loss, val_acc = self.evaluate(validation_imgs, validation_labels)
            logs = {"loss": float(loss_sum) / steps_per_epoch, "binary_accuracy": float(acc_sum) / steps_per_epoch,
                    "val_loss": val_loss, "val_binary_accuracy": val_acc}
            self.callback(epoch, logs, output_dir)
