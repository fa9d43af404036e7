"""Import-path shim for reference ``tf_raft/datasets/augmentor.py`` (dataset.py:11: ``from .augmentor import FlowAugmentor,
SparseFlowAugmentor``): both augmentors on the device (DESIGN.md sections 10 and 11)."""
from tf_raft_amd.augment import FlowAugmentor, SparseFlowAugmentor  # noqa: F401
