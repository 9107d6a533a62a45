from .api import add_depth, add_location, swap_dims_channel_frequency  # noqa: F401
from .splitbeam import add_splitbeam_angle  # noqa: F401

__all__ = ["add_depth", "add_location", "add_splitbeam_angle", "swap_dims_channel_frequency"]
