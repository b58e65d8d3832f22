from .device_dataset import DeviceAugmentLoader, DeviceJointsDB, synthetic_aug  # noqa: F401
from .device_pipeline import DevicePipeline  # noqa: F401
from .synthetic import SyntheticPose  # noqa: F401
