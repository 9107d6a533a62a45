from .transient_fielding import transient_noise_fielding  # noqa: F401
from .transient_matecho import transient_noise_matecho  # noqa: F401

__all__ = ["transient_noise_fielding", "transient_noise_matecho"]
