from .api import METHODS_SINGLE_TARGET, detect_single_targets  # noqa: F401

__all__ = ["detect_single_targets", "METHODS_SINGLE_TARGET"]
