"""Import-path shim for reference ``tf_raft/datasets/__init__.py`` (train_sintel.py:9: ``from tf_raft.datasets import MpiSintel,
ShapeSetter, CropOrPadder``): the batch-shaping stages and the training augmentations; the data-set readers are out of scope."""
from tf_raft_amd.augment import FlowAugmentor, SparseFlowAugmentor  # noqa: F401
from tf_raft_amd.datasets import CropOrPadder, ShapeSetter  # noqa: F401
