from .summary_statistics import (abundance, aggregation, center_of_mass, convert_to_linear, delta_z,  # noqa: F401
                                 dispersion, evenness, summary)

__all__ = ["abundance", "aggregation", "center_of_mass", "convert_to_linear", "delta_z", "dispersion", "evenness",
           "summary"]
