"""Synthetic datasets, sharded sampling and (on-device) augmentation."""
from .synthetic import (SyntheticCIFAR10, SyntheticCIFAR100, SyntheticImageNet,  # noqa: F401
                        SyntheticImageDataset)
from .loader import (CPULoader, DeviceLoader, make_loader, shard_indices, augment_cpu,  # noqa: F401
                     lam_table, CIFAR_MEAN, CIFAR_STD)
