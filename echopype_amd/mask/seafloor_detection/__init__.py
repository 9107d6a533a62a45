from .bottom_basic import bottom_basic  # noqa: F401
from .bottom_blackwell import bottom_blackwell  # noqa: F401

__all__ = ["bottom_basic", "bottom_blackwell"]
