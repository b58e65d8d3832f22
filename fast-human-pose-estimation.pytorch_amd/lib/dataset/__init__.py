from .coco import COCODataset, coco  # noqa: F401
from .device_dataset import DeviceAugmentLoader, DeviceJointsDB, epoch_order, synthetic_aug  # noqa: F401
from .device_pipeline import DevicePipeline  # noqa: F401
from .mpii import MPIIDataset, mpii  # noqa: F401
from .synthetic import SyntheticPose  # noqa: F401
