from .shoal_echoview import shoal_echoview  # noqa: F401
from .shoal_weill import shoal_weill  # noqa: F401

__all__ = ["shoal_echoview", "shoal_weill"]
