#!/usr/bin/env python
"""Controllability metrics of a ConfigNet checkpoint on a test set (reference: evaluation/evaluate_confignet_controllability.py;
ConfigNet paper, Table 2).

    python evaluation/evaluate_confignet_controllability.py --model_path models/confignet_256/model.json \
        --attribute_classifier_path models/attribute_classifier/model.json --test_set_path test.pck --output_dir OUT \
        --synth_data_path synth.pck [--beard_style_map_path beard_style_to_pca_map.json] [--n_fine_tuning_iters N] \
        [--n_samples 1000] [--write_images]

Writes <name>.json (the metrics dict), <name>.csv (rows: attribute value for I+, for I-, mean difference of the other
attributes, corr coef; one column per configuration) and, when matplotlib is importable, <name>.png, with
<name> = contr_metrics_tuning_iters_<N>_<model file stem>.  --synth_data_path names the synthetic dataset whose metadata
labels give the blendshape names; without --beard_style_map_path the mustache configuration is skipped."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the package loads its HIP library: kernels and tensors must share torch's HIP runtime)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_path", help="Path to the confignet model", required=True)
    parser.add_argument("--test_set_path", help="Path to the test set", required=True)
    parser.add_argument("--output_dir", help="Directory where results will be written", required=True)
    parser.add_argument("--attribute_classifier_path", help="Path to the celeba attribute classifier that will be used for testing",
                        required=True)
    parser.add_argument("--synth_data_path", help="Synthetic dataset whose metadata labels give the blendshape names", required=True)
    parser.add_argument("--beard_style_map_path", help="beard_style_to_pca_map.json of the synthetic data (mustache configuration)",
                        default=None)
    parser.add_argument("--n_fine_tuning_iters", type=int, help="Number of fine tuning iterations that will be performed on each image",
                        default=0)
    parser.add_argument("--n_samples", type=int, help="Number of samples used for testing", default=1000)
    parser.add_argument("--write_images", help="Write the generated images next to the results", action="store_true", default=False)
    return parser


def parse_args(args):
    args = build_parser().parse_args(args)
    import confignet
    confignet_model = confignet.load_confignet(args.model_path)
    test_set = confignet.NeuralRendererDataset.load(args.test_set_path)
    test_imgs = np.asarray(test_set.imgs[:args.n_samples])
    synth_set = confignet.NeuralRendererDataset.load(args.synth_data_path)
    if not synth_set.metadata_input_labels:
        synth_set.process_metadata(confignet_model.config)
    blendshape_names = synth_set.metadata_input_labels["blendshape_values"]

    metrics_extractor = confignet.ControllabilityMetrics(confignet_model, args.attribute_classifier_path,
                                                         per_image_tuning_iters=args.n_fine_tuning_iters,
                                                         blendshape_names=blendshape_names, beard_style_map=args.beard_style_map_path)
    metrics_filename = "contr_metrics_tuning_iters_%d_" % args.n_fine_tuning_iters
    metrics_filename += os.path.splitext(os.path.basename(args.model_path))[0]
    img_output_dir = os.path.join(args.output_dir, metrics_filename) if args.write_images else None
    os.makedirs(args.output_dir, exist_ok=True)
    metrics = metrics_extractor.get_metrics(test_imgs, img_output_dir=img_output_dir)

    per_config = [(key, value) for key, value in metrics.items() if isinstance(value, tuple)]
    set_attribute_values = [v[0] for _, v in per_config]
    not_set_attribute_values = [v[1] for _, v in per_config]
    other_attr_deltas = [v[2] for _, v in per_config]
    correlation_coefficient = [v[3] for _, v in per_config]
    tick_labels = [k for k, _ in per_config]

    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
    except ImportError:
        plt = None
    if plt is not None:
        plt.figure(figsize=(12, 9))
        plt.plot(set_attribute_values)
        plt.plot(not_set_attribute_values)
        plt.plot(other_attr_deltas)
        plt.plot(correlation_coefficient)
        plt.legend(["Attribute value for I_+", "Attribute value for I_-", "Mean difference of other attributes", "Corr coef"])
        plt.xticks(range(len(set_attribute_values)), rotation=45)
        plt.gca().set_xticklabels(tick_labels)
        plt.ylim(0, 1)
        plt.tight_layout()
        plt.savefig(os.path.join(args.output_dir, metrics_filename + ".png"))
        plt.close()

    with open(os.path.join(args.output_dir, metrics_filename + ".json"), "w") as fp:
        json.dump(metrics, fp, indent=4)
    csv_content = np.vstack((set_attribute_values, not_set_attribute_values, other_attr_deltas, correlation_coefficient))
    np.savetxt(os.path.join(args.output_dir, metrics_filename + ".csv"), csv_content, delimiter=",")
    return metrics


if __name__ == "__main__":
    parse_args(sys.argv[1:])
