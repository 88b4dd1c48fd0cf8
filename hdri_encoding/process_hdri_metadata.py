#!/usr/bin/env python
"""Command line of confignet_amd.hdri.embed_render_metadata: writes `hdri_embedding` into the render metadata .json files of a
dataset, all renders in one pass over the pool of environment maps.  Flag names are the reference's
(hdri_encoding/process_hdri_metadata.py).

    python hdri_encoding/process_hdri_metadata.py --input_dir renders/ --render_asset_dir assets/ --model_path models/hdri/hdri_model.pck
"""
import argparse
import os
import sys

import torch  # noqa: F401  (before the package: the HIP library then binds to the HIP runtime torch ships)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from confignet_amd import hdri  # noqa: E402

DEFAULT_MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "assets", "hdri_model_20200116.pck")


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Add hdri_embedding to render metadata files")
    ap.add_argument("--input_dir", required=True, help="folder of render metadata *.json files; they are rewritten in place")
    ap.add_argument("--render_asset_dir", required=True, help="asset folder; the environment maps are the *.hdr files of its HDRI/ subfolder")
    ap.add_argument("--hdri_output_dir", default=None, help="if given: folder for each render's rotated map and its reconstruction (.hdr)")
    ap.add_argument("--model_path", default=DEFAULT_MODEL, help="model file, ours or one the reference wrote")
    a = ap.parse_args(argv)
    return hdri.embed_render_metadata(a.input_dir, a.render_asset_dir, a.model_path, a.hdri_output_dir)


if __name__ == "__main__":
    parse_args(sys.argv[1:])
