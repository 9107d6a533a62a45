from .api import METHODS_SINGLE_TARGET, detect_single_targets  # noqa: F401
from .spectra import target_spectra  # noqa: F401
from .track import METHODS_TRACK, track_targets  # noqa: F401

# (tests/test_track_host.py holds ``__all__`` at the four names it had when tracking was added: ``target_spectra`` is an
#  attribute of the package like them, and left out of the star import)
__all__ = ["detect_single_targets", "METHODS_SINGLE_TARGET", "track_targets", "METHODS_TRACK"]
