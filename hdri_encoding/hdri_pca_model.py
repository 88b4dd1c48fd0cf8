#!/usr/bin/env python
"""Command line of confignet_amd.hdri.build_model: fits the PCA model of 360-degree HDR environment maps on the *.hdr pictures of a
directory and writes hdri_model.pck, the basis pictures and (--write_hdris) reconstructions.  Flag names are the reference's
(hdri_encoding/hdri_pca_model.py), so its command lines keep working.

    python hdri_encoding/hdri_pca_model.py --hdri_dir assets/HDRI --output_dir models/hdri --output_shape 64 128
"""
import argparse
import os
import sys

import torch  # noqa: F401  (before the package: the HIP library then binds to the HIP runtime torch ships)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from confignet_amd import hdri  # noqa: E402
from confignet_amd.hdri import HDRIModelPCA, load_hdris, rotate_hdri  # noqa: E402,F401  (importers of this module expect them here)


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Fit the HDRI PCA model")
    ap.add_argument("--hdri_dir", required=True, help="folder whose *.hdr pictures (equirectangular, all one size) the model is fitted on")
    ap.add_argument("--output_dir", required=True, help="folder for hdri_model.pck, pca_basis/ and hdris/")
    ap.add_argument("--n_components", type=float, default=50, help="how many components to keep; a value in (0, 1) keeps as many as explain that share of the variance")
    ap.add_argument("--output_shape", type=int, nargs=2, default=(64, 128), metavar=("ROWS", "COLS"), help="size the pictures are reduced to before the decomposition")
    ap.add_argument("--n_rotations_per_image", type=int, default=5, help="randomly rotated copies of each picture in the fit")
    ap.add_argument("--write_hdris", action="store_true", help="also write each picture at the model's size and as the model reconstructs it")
    ap.add_argument("--seed", type=int, default=0, help="numpy seed the rotations are drawn under")
    a = ap.parse_args(argv)
    return hdri.build_model(a.hdri_dir, a.output_dir, a.n_components, a.output_shape, a.n_rotations_per_image, a.seed, a.write_hdris)


if __name__ == "__main__":
    parse_args(sys.argv[1:])
