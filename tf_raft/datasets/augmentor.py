"""Import-path shim for reference ``tf_raft/datasets/augmentor.py`` (dataset.py:11: ``from .augmentor import FlowAugmentor,
SparseFlowAugmentor``): the dense augmentor on the device; the sparse one is out of scope."""
from tf_raft_amd.augment import FlowAugmentor  # noqa: F401
