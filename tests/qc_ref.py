"""Restatement of the reference's reversed-time repair (qc/api.py:12-85) as a loop over int64 ticks (Python integers, wrapped):
the formula as the issue states it, not the reference's text.  tests/test_qc_host.py holds it bit for bit to the results
the reference's own ``_clean_reversed`` gave (tests/golden/qc_reversed_time.npz); the GPU tests hold the kernels to it.

With ``d[i] = t[i+1] - t[i]``: the reversals are the ``ni`` with ``d[ni] < 0``; each is replaced by the median of the
ORIGINAL ``d[max(0, ni - win_len) : ni]`` (an even count: the wrapping sum of the two middle values divided by 2, truncated
toward zero); with ``f`` the first reversal, ``new[: f+1] = t[: f+1]`` and ``new[f+1+k] = t[f] + sum(d'[f : f+k+1])``."""
import numpy as np

NAT = -(1 << 63)


def wrap(x):
    """A Python integer as the int64 it wraps to."""
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def ticks(t):
    """A datetime64 array (any unit) or an integer array -> list of Python integers."""
    a = np.asarray(t)
    return [int(x) for x in (a.view(np.int64) if a.dtype.kind == "M" else a)]


def median(vals):
    """np.median of timedelta64 values, on their ticks."""
    s = sorted(vals)
    n = len(s)
    if n == 0:
        raise IndexError("the window before the reversal is empty")
    if n % 2:
        return s[n // 2]
    tot = wrap(s[n // 2 - 1] + s[n // 2])
    return -((-tot) // 2) if tot < 0 else tot // 2


def reversals(t):
    """Indices ni with a negative difference that touches no NaT."""
    t = ticks(t)
    return [i for i in range(len(t) - 1) if t[i] != NAT and t[i + 1] != NAT and wrap(t[i + 1] - t[i]) < 0]


def exist_reversed(t):
    return bool(reversals(t))


def is_sorted_and_valid(t):
    t = ticks(t)
    return bool(t) and NAT not in t and not reversals(t)


def clean_reversed(t, win_len):
    """The repaired ticks as an int64 array.  No reversal, and a reversal in the first difference: IndexError, like the
    reference.  NaT is not restated (the package refuses it)."""
    t = ticks(t)
    assert NAT not in t
    d = [wrap(t[i + 1] - t[i]) for i in range(len(t) - 1)]
    neg = [i for i, x in enumerate(d) if x < 0]
    if not neg:
        raise IndexError("no reversal")
    sub = {ni: median(d[max(0, ni - win_len):ni]) for ni in neg}  # all medians before any substitution
    f = neg[0]
    new = t[:f + 1]
    for i in range(f, len(d)):
        new.append(wrap(new[-1] + sub.get(i, d[i])))
    return np.array(new, dtype=np.int64)
