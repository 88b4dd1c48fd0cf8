"""Alias of confignet_amd.face_image_normalizer under the reference's module path."""
from confignet_amd.face_image_normalizer import *   # noqa: F401,F403
from confignet_amd import face_image_normalizer as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
