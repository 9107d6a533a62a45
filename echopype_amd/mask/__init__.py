from .api import (METHODS_BOTTOM, METHODS_SHOAL, apply_mask, detect_seafloor, detect_shoal,  # noqa: F401
                  frequency_differencing, line_mask, regrid_mask)
from .regions import label_regions, region_statistics  # noqa: F401

__all__ = ["apply_mask", "detect_seafloor", "detect_shoal", "frequency_differencing", "line_mask", "regrid_mask",
           "METHODS_BOTTOM", "METHODS_SHOAL", "label_regions", "region_statistics"]
