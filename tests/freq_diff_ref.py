"""NumPy judge of mask.frequency_differencing: the operator applied to ``sv[a] - sv[b]`` in the array's own type (what
the reference computes for an ndarray and a Python scalar), and, to tell the two rules apart, the same in float64."""
import operator

import numpy as np

OPS = {">": operator.gt, "<": operator.lt, "<=": operator.le, ">=": operator.ge, "==": operator.eq}


def freq_diff(sv, a, b, op, diff):
    """bool array like ``sv[0]``: (sv[a] - sv[b]) op diff, NumPy's own arithmetic (difference and scalar in sv.dtype)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(OPS[op](sv[a] - sv[b], diff))


def freq_diff_typed(sv, a, b, op, diff):
    """The same with the scalar converted to the array's type by hand."""
    with np.errstate(invalid="ignore"):
        return np.asarray(OPS[op](sv[a] - sv[b], sv.dtype.type(diff)))


def freq_diff_in_double(sv, a, b, op, diff):
    """The other rule: the rounded difference compared with the unrounded ``diff`` in float64."""
    with np.errstate(invalid="ignore"):
        return np.asarray(OPS[op]((sv[a] - sv[b]).astype(np.float64), float(diff)))


def half_steps(rng, shape, dtype, lo=-8, hi=8):
    """Values that are multiples of 0.5: differences hit a threshold that is one exactly and often."""
    return (rng.integers(2 * lo, 2 * hi + 1, size=shape) * 0.5).astype(dtype)
