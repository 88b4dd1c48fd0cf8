#!/usr/bin/env python
"""Headless ConfigNet demo on MI355X (reference: evaluation/confignet_demo.py; no window -- frames go to --output_dir as
.npy canvases, keys come from --keys).  Models are loaded with the reference's layout (model.json + model.npz).

    python evaluation/confignet_demo.py --confignet_model_path models/confignet_256/model.json \
        --latent_gan_model_path models/latentgan_256/model.json --keys "ddwwx  b" [--image_path face.npy | photo.jpg | photos/] [--test_mode]

--image_path takes a photo or a directory of photos as the reference's demo does (they are normalised first: OpenFace landmarks,
confignet_amd/face_image_normalizer.py), or an .npy of faces that are aligned already.
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from confignet import ConfigNet, FaceImageNormalizer, LatentGAN   # noqa: E402
from confignet_amd.demo import DemoSession   # noqa: E402
from confignet_amd.face_image_normalizer import DEFAULT_OPENFACE_PATH, imread, pick_device   # noqa: E402


MAX_INPUT_IMAGES = 200          # of a directory, as the reference's demo


def process_images(image_path, resolution, openface_path=None, device=None):
    """The demo's input faces as a list of (R, R, 3) uint8 B, G, R arrays: an .npy of faces that are aligned already, one photo,
    or a directory of photos (normalised into <directory>/normalized, without done markers, so a later call sees new photos)."""
    openface_path = openface_path or DEFAULT_OPENFACE_PATH
    shape = (resolution, resolution)
    if os.path.isdir(image_path):
        FaceImageNormalizer.normalize_dataset_dir(image_path, True, shape, openface_path=openface_path, write_done_file=False,
                                                  device=device)
        found = glob.glob(os.path.join(image_path, "normalized", "*.png"))[:MAX_INPUT_IMAGES]
        if not found:
            raise ValueError("%s: no picture with a detected face" % image_path)
        return [imread(path) for path in found]
    if not os.path.isfile(image_path):
        raise ValueError("%s is neither a file nor a directory" % image_path)
    if image_path.endswith(".npy"):
        arr = np.load(image_path)
        return [arr] if arr.ndim == 3 else list(arr)
    return [FaceImageNormalizer.normalize_individual_image(imread(image_path), shape, openface_path=openface_path, device=device)]


def run(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--image_path", default=None, help="an image, a directory of images, or an .npy with one (R,R,3) or several "
                    "(M,R,R,3) aligned uint8 face images")
    ap.add_argument("--openface_path", default=None, help="FaceLandmarkImg of an OpenFace build, for images that are not aligned yet")
    ap.add_argument("--device", default=None, help="where photos are warped, as in generate_dataset.py: a torch device, or none for numpy")
    ap.add_argument("--confignet_model_path", required=True)
    ap.add_argument("--latent_gan_model_path", default=None)
    ap.add_argument("--n_rows", type=int, default=2)
    ap.add_argument("--n_cols", type=int, default=3)
    ap.add_argument("--keys", default="", help="key presses, one per frame (space, wsad, ikjl, n, x, z, c, v, b)")
    ap.add_argument("--output_dir", default=None)
    ap.add_argument("--hdri_turntable_path", default=None, help="assets/hdri_turntable_embeddings.npy of the reference")
    ap.add_argument("--test_mode", action="store_true", help="one frame, every key handler fired once")
    args = ap.parse_args(argv)
    images = None
    aligned = args.image_path is not None and args.image_path.endswith(".npy")
    if aligned:
        images = process_images(args.image_path, None)
    latentgan = LatentGAN.load(args.latent_gan_model_path) if args.image_path is None else None
    model = ConfigNet.load(args.confignet_model_path)
    if args.image_path is not None and not aligned:             # photos are normalised to the model's resolution
        images = process_images(args.image_path, int(model.config["output_shape"][0]), args.openface_path, device=pick_device(args.device))
    hdri = np.load(args.hdri_turntable_path) if args.hdri_turntable_path else None
    session = DemoSession(model, latentgan, images, args.n_rows, args.n_cols, hdri)
    count = [0]

    def save(canvas):
        if args.output_dir is not None:
            os.makedirs(args.output_dir, exist_ok=True)
            np.save(os.path.join(args.output_dir, "frame_%04d.npy" % count[0]), canvas)
        count[0] += 1
    session.run(test_mode=args.test_mode, keys=args.keys, on_frame=save)
    return session


if __name__ == "__main__":
    run(sys.argv[1:])
