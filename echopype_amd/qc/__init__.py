from .api import check_and_correct_reversed_time, coerce_increasing_time, exist_reversed_time  # noqa: F401

__all__ = ["exist_reversed_time", "coerce_increasing_time", "check_and_correct_reversed_time"]
