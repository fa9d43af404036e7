"""Import-path shim for reference ``tf_raft/datasets/flow_viz.py`` (tf_raft/training.py:7: ``from .datasets.flow_viz import
flow_to_image``): the Middlebury colour coding of ``tf_raft_amd.io``."""
from tf_raft_amd.io import flow_to_image, flow_uv_to_colors, make_colorwheel  # noqa: F401
