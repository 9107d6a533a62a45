"""``convert``: raw instrument files -> EchoData (echopype convert/).  EK60 ``.raw`` only: see :mod:`.api`."""
from .api import open_raw  # noqa: F401

__all__ = ["open_raw"]
