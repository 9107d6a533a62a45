from .api import (check_and_correct_reversed_time, coerce_increasing_time, create_old_time_array,  # noqa: F401
                  exist_reversed_time, orchestrate_reverse_time_check)

__all__ = ["exist_reversed_time", "coerce_increasing_time", "check_and_correct_reversed_time"]
