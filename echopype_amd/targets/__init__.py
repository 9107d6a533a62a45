from .api import METHODS_SINGLE_TARGET, detect_single_targets  # noqa: F401
from .track import METHODS_TRACK, track_targets  # noqa: F401

__all__ = ["detect_single_targets", "METHODS_SINGLE_TARGET", "track_targets", "METHODS_TRACK"]
