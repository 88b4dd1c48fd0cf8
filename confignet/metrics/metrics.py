from confignet_amd.metrics.metrics import InceptionMetrics                                # noqa: F401
from confignet_amd.metrics.controllability import ControllabilityMetrics                    # noqa: F401
from confignet_amd.metrics.celeba_attribute_prediction import CelebaAttributeClassifier   # noqa: F401
