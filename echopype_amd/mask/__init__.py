from .api import METHODS_BOTTOM, apply_mask, detect_seafloor  # noqa: F401

__all__ = ["apply_mask", "detect_seafloor", "METHODS_BOTTOM"]
