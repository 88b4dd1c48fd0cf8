"""confignet_amd -- MI355X-native implementation of the ConfigNet GAN hot path behind the reference's
own Python surface (reference: confignet/__init__.py:3-14 for the names callers import)."""
import torch  # noqa: F401  (before the HIP library loads: kernels and tensors must share torch's HIP runtime, whatever the caller imports first)

from ._lib import LIB_PATH  # noqa: F401  (raises ImportError if the HIP library is not built)
from .confignet_first_stage import ConfigNetFirstStage
from .confignet_second_stage import ConfigNet
from .latent_gan import LatentGAN
from .confignet_utils import load_confignet
from .synthetic_data import SyntheticFaceDataset
from .face_image_normalizer import FaceImageNormalizer

__all__ = ["ConfigNetFirstStage", "ConfigNet", "LatentGAN", "load_confignet", "SyntheticFaceDataset", "FaceImageNormalizer"]
