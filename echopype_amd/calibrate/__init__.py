from .api import CALIBRATOR, compute_Sv, compute_TS  # noqa: F401
from .sv_spectrum import compute_Sv_spectrum  # noqa: F401

__all__ = ["compute_Sv", "compute_TS", "compute_Sv_spectrum", "CALIBRATOR"]
