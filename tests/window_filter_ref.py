"""The rule of clean.window_filter restated in NumPy: the judge of the kernel (csrc/window_filter.hip).

``x[..., p, s]`` float32 or float64, a window of ``ping_num x range_sample_num`` samples (both odd), half widths ``hp``
and ``hs``.  The window of ``(p, s)`` is pings ``p-hp .. p+hp`` and samples ``s-hs .. s+hs`` clipped to the array --
written here as a NaN pad of the half widths, since NaN is what the rule ignores -- and never crosses the leading axes.
Valid values are the non-NaN ones; ``-inf`` and ``+inf`` are values.  All arithmetic is float64, rounded once to the
type of ``x``:

``min`` / ``max``  ``nanmin`` / ``nanmax`` of the window;
``mean``           ``10 log10(nanmean(10^(v/10)))``;
``median``         ``10 log10(nanmedian(10^(v/10)))``, evaluated as a selection: with ``a <= b`` the two middle valid values
                   (the same one for an odd count) the result is ``a`` itself where ``a == b`` and ``10 log10((10^(a/10)
                   + 10^(b/10)) / 2)`` otherwise.  (``test_window_filter_host.py`` holds this form to the expression on
                   the linear values.)

A window with fewer than ``min_valid`` valid values gives NaN; with ``keep_nan`` a sample that is NaN stays NaN."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

METHODS = ("median", "mean", "min", "max")


def windows(x, ping_num, range_sample_num):
    """(..., P, S, ping_num * range_sample_num) float64: the window of every sample, NaN outside the array."""
    x = np.asarray(x)
    hp, hs = ping_num // 2, range_sample_num // 2
    pad = [(0, 0)] * (x.ndim - 2) + [(hp, hp), (hs, hs)]
    xp = np.pad(x.astype(np.float64), pad, constant_values=np.nan)
    w = sliding_window_view(xp, (ping_num, range_sample_num), axis=(-2, -1))
    return w.reshape(*x.shape, ping_num * range_sample_num)


def _lin(v):
    with np.errstate(over="ignore"):
        return np.power(10.0, v / 10.0)


def window_results(x, ping_num, range_sample_num):
    """({method: the float64 result of every window before ``min_valid`` and ``keep_nan`` act, NaN where the window has
    no valid value}, the number of valid values per window): one pass over the windows for all four methods."""
    x = np.asarray(x)
    assert x.ndim >= 2 and x.dtype in (np.float32, np.float64)
    assert ping_num % 2 == 1 and range_sample_num % 2 == 1
    if x.size == 0:
        return {m: np.full(x.shape, np.nan) for m in METHODS}, np.zeros(x.shape, np.int64)
    w = windows(x, ping_num, range_sample_num)
    valid = ~np.isnan(w)
    n = valid.sum(axis=-1)
    nn = np.maximum(n, 1)
    res = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        res["min"] = np.where(valid, w, np.inf).min(axis=-1)
        res["max"] = np.where(valid, w, -np.inf).max(axis=-1)
        res["mean"] = 10.0 * np.log10(np.where(valid, _lin(w), 0.0).sum(axis=-1) / nn)
        srt = np.sort(w, axis=-1)  # NaN last
        a = np.take_along_axis(srt, ((nn - 1) // 2)[..., None], axis=-1)[..., 0]
        b = np.take_along_axis(srt, (nn // 2)[..., None], axis=-1)[..., 0]
        res["median"] = np.where(a == b, a, 10.0 * np.log10((_lin(a) + _lin(b)) / 2.0))
    return {m: np.where(n > 0, r, np.nan) for m, r in res.items()}, n


def finish(res, n, x, min_valid=1, keep_nan=True):
    """``min_valid`` and ``keep_nan`` applied to one result of ``window_results``, rounded once to the type of ``x``."""
    x = np.asarray(x)
    assert 1 <= min_valid
    res = np.where(n >= min_valid, res, np.nan)
    if keep_nan:
        res = np.where(np.isnan(x), np.nan, res)
    return res.astype(x.dtype)


def window_filter_ref(x, method, ping_num, range_sample_num, min_valid=1, keep_nan=True, with_count=False):
    """The filtered array, of the type and shape of ``x``; ``with_count``: and the number of valid values per window."""
    assert method in METHODS and 1 <= min_valid <= ping_num * range_sample_num
    res, n = window_results(x, ping_num, range_sample_num)
    out = finish(res[method], n, x, min_valid, keep_nan)
    return (out, n) if with_count else out
