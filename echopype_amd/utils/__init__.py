from . import uwa  # noqa: F401
from .align import align_to_ping_time  # noqa: F401
