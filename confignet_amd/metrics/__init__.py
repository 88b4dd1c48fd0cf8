"""Training-time metrics of the reference (confignet/metrics/): FID / KID on InceptionV3 features and the controllability
metrics on the CelebA attribute classifier (MobileNetV2), on the HIP path."""
from .inception_distance import InceptionFeatureExtractor, compute_FID, compute_KID      # noqa: F401
from .metrics import InceptionMetrics                                                    # noqa: F401
from .celeba_attribute_prediction import CelebaAttributeClassifier                       # noqa: F401
from .controllability import ControllabilityMetrics                                      # noqa: F401
