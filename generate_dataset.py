#!/usr/bin/env python
"""Builds a NeuralRendererDataset (`<name>_res_<size>.pck` + `<name>_res_<size>_imgs.dat`) from a directory of pictures; the
command line of the reference's generate_dataset.py (same flag names and defaults), plus --openface_path and --device.

    python generate_dataset.py --dataset_dir renders/ --dataset_name synth --output_dir datasets/ --synthetic_data --pre_normalize 0

Landmarks come from the user's own OpenFace build (--openface_path, or OPENFACE_PATH), or from `processed/*.csv` files and the
`landmarks_detected` marker placed next to the pictures; nothing is downloaded."""
import argparse
import os
import sys

import confignet
from confignet_amd.face_image_normalizer import pick_device


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset_dir", required=True, help="directory with the pictures (and, for renders, their meta*.json / uv*.exr)")
    ap.add_argument("--dataset_name", required=True, help="stem of the two output files; _res_<img_size> is appended")
    ap.add_argument("--output_dir", required=True, help="where the two files go (created if missing)")
    ap.add_argument("--img_size", type=int, default=256, help="side of the square normalised pictures")
    ap.add_argument("--pre_normalize", type=int, default=1, help="0 skips the 2-D pre-normalisation (use for renders)")
    ap.add_argument("--img_output_dir", default=None, help="also write the normalised pictures here as JPEGs")
    ap.add_argument("--load_attributes", action="store_true", help="read dataset_dir/list_attr_celeba.txt")
    ap.add_argument("--synthetic_data", action="store_true", help="renders: per-picture metadata, pose filter and eye masks")
    ap.add_argument("--openface_path", default=None, help="FaceLandmarkImg of an OpenFace build")
    ap.add_argument("--device", default=None, help="torch device of the warps, or none for numpy; default: the GPU if there is one")
    args = ap.parse_args(argv)

    size = args.img_size
    dataset = confignet.NeuralRendererDataset((size, size, 3), args.synthetic_data, device=pick_device(args.device))
    os.makedirs(args.output_dir, exist_ok=True)
    output_path = os.path.join(args.output_dir, "%s_res_%d.pck" % (args.dataset_name, size))
    attributes = os.path.join(args.dataset_dir, "list_attr_celeba.txt") if args.load_attributes else None
    dataset.generate_face_dataset(args.dataset_dir, output_path, attribute_label_file_path=attributes,
                                  pre_normalize=args.pre_normalize == 1, openface_path=args.openface_path)
    if args.img_output_dir is not None:
        print("normalised pictures -> %s" % args.img_output_dir)
        dataset.write_images(args.img_output_dir)
        if args.load_attributes:
            dataset.write_images_by_attribute(args.img_output_dir)
    return dataset


if __name__ == "__main__":
    parse_args(sys.argv[1:])
