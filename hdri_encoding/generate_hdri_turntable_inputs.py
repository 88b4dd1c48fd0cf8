#!/usr/bin/env python
"""Command line of confignet_amd.hdri.write_turntable: the embeddings of one environment map turned once around the vertical axis,
saved as .npy for the demo's light sweep (evaluation/confignet_demo.py --hdri_turntable_path).  Flag names are the reference's
(hdri_encoding/generate_hdri_turntable_inputs.py).

    python hdri_encoding/generate_hdri_turntable_inputs.py --hdri_file_path sky.hdr --hdri_model_path models/hdri/hdri_model.pck \
        --output_file_path assets/hdri_turntable_embeddings.npy
"""
import argparse
import os
import sys

import torch  # noqa: F401  (before the package: the HIP library then binds to the HIP runtime torch ships)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from confignet_amd import hdri  # noqa: E402

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "assets")


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Embed one environment map under a full turn of rotations")
    ap.add_argument("--hdri_file_path", required=True, help="the .hdr picture to turn")
    ap.add_argument("--output_file_path", default=os.path.join(ASSETS, "hdri_turntable_embeddings.npy"), help=".npy file the (rotations, components) array is written to")
    ap.add_argument("--hdri_model_path", default=os.path.join(ASSETS, "hdri_model_20190919.pck"), help="model file, ours or one the reference wrote")
    ap.add_argument("--n_hdri_rotations", type=int, default=90, help="steps from -180 to 180 degrees, both ends included")
    ap.add_argument("--hdri_output_dir", default=None, help="if given: folder for the pictures decoded back from the embeddings (.hdr)")
    a = ap.parse_args(argv)
    return hdri.write_turntable(a.hdri_file_path, a.hdri_model_path, a.output_file_path, a.n_hdri_rotations, a.hdri_output_dir)


if __name__ == "__main__":
    parse_args(sys.argv[1:])
