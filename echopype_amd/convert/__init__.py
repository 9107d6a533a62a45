"""``convert``: raw instrument files -> EchoData (echopype convert/).  EK60 ``.raw`` through ``open_raw`` (:mod:`.api`),
EK80 ``.raw`` through ``open_raw_ek80`` (:mod:`.api_ek80`)."""
from .api import open_raw  # noqa: F401
from .api_ek80 import open_raw_ek80  # noqa: F401

__all__ = ["open_raw", "open_raw_ek80"]
