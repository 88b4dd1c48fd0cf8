#!/usr/bin/env python
"""Training of the CelebA attribute classifier on MI355X with the reference's command line (reference:
train_attribute_classifier.py:11-34).

    python train_attribute_classifier.py --training_set_path train.pck --validation_set_path val.pck --output_dir OUT \
        [--n_epochs 1000] [--steps_per_epoch 100] [--batch_size 32] [--ignored_attributes Wearing_Necklace Wearing_Necktie]

Dataset files are the reference's (`NeuralRendererDataset.save`: <name>.pck + the image memmap next to it) with per-image
CelebA attributes.  The output directory receives checkpoints/, best_model/ and logs.txt; a checkpoint's .json is what
train_confignet.py --attribute_classifier_path takes."""
import argparse
import copy
import sys

import numpy as np
import torch  # noqa: F401  (before the package loads its HIP library: kernels and tensors must share torch's HIP runtime)

import confignet
from confignet.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier

FLAGS = [
    ("--training_set_path", dict(required=True, help="training set (.pck)")),
    ("--validation_set_path", dict(required=True, help="validation set (.pck)")),
    ("--output_dir", dict(required=True, help="receives checkpoints/, best_model/ and logs.txt")),
    ("--n_epochs", dict(type=int, default=1000)),
    ("--steps_per_epoch", dict(type=int, default=100)),
    ("--batch_size", dict(type=int, default=DEFAULT_CONFIG["batch_size"])),
    ("--ignored_attributes", dict(nargs="+", default=["Wearing_Necklace", "Wearing_Necktie"], help="attributes left out of the classifier")),
]


def parse_args(argv):
    ap = argparse.ArgumentParser(description="CelebA attribute classifier training (MI355X)")
    for flag, kw in FLAGS:
        ap.add_argument(flag, **kw)
    return ap.parse_args(argv)


def main(argv):
    args = parse_args(argv)
    training_set = confignet.NeuralRendererDataset.load(args.training_set_path)
    validation_set = confignet.NeuralRendererDataset.load(args.validation_set_path)
    config = copy.deepcopy(DEFAULT_CONFIG)
    config["input_shape"] = tuple(int(v) for v in training_set.imgs.shape[1:])
    config["batch_size"] = args.batch_size
    # every attribute of the data set but the ignored ones, sorted (the order of the classifier's outputs)
    config["predicted_attributes"] = sorted(a for a in training_set.attributes[0] if a not in args.ignored_attributes)
    np.random.seed(0)
    classifier = CelebaAttributeClassifier(config)
    classifier.train(training_set, validation_set, args.output_dir, n_epochs=args.n_epochs, steps_per_epoch=args.steps_per_epoch)


if __name__ == "__main__":
    main(sys.argv[1:])
