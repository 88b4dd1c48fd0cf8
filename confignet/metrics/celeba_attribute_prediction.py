"""Alias of confignet_amd.metrics.celeba_attribute_prediction under the reference's module path."""
from confignet_amd.metrics.celeba_attribute_prediction import *                           # noqa: F401,F403
from confignet_amd.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier   # noqa: F401
