from .api import METHODS_BOTTOM, METHODS_SHOAL, apply_mask, detect_seafloor, detect_shoal  # noqa: F401

__all__ = ["apply_mask", "detect_seafloor", "detect_shoal", "METHODS_BOTTOM", "METHODS_SHOAL"]
