"""Alias of the controllability configurations (confignet_amd.metrics.controllability) under the reference's module path."""
from confignet_amd.metrics.controllability import CONFIGS, ControllabilityMetricConfigs, ControllableAttributeConfig   # noqa: F401
