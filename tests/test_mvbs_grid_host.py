"""The conservative range grid of the compute_MVBS routes that do not wait for the GPU (commongrid/deferred.py): the bin
count, and what happens to bins launched on ``n_cap`` range bins once the range statistics are known -- CPU only."""
import logging

import numpy as np
import pytest

from echopype_amd.commongrid import deferred
from echopype_amd.xr_lite import Dataset

BINS = [0.5, 1.0, 2.0, 20.0]


@pytest.mark.parametrize("b", BINS)
def test_n_range_bins_is_the_length_of_the_reference_arange(b):
    maxima = [0.0, 1e-8, np.nextafter(b, 0.0), b, b + 1e-8, 7 * b, 7 * b + 1e-8, 149.99999999, 150 + 1e-8]
    for r in maxima:
        edges = np.arange(0, r + b, b)
        assert deferred.n_range_bins(r, b) == len(edges) - 1, (r, b)
        np.testing.assert_array_equal(deferred.range_edges(r, b), edges)
    for r in (float("nan"), float("inf"), float("-inf")):
        assert deferred.n_range_bins(r, b) == 0
        assert len(deferred.range_edges(r, b)) == 1


def _rmax_for(n_r, b=1.0):
    """A maximum whose reference grid has ``n_r`` bins (checked with NumPy)."""
    r = (n_r - 0.5) * b if n_r else 0.0
    assert len(np.arange(0, r + b, b)) - 1 == n_r
    return r


def test_trim_decision_keeps_slices_or_falls_back(caplog):
    caplog.set_level(logging.WARNING)
    decide = lambda stats, **kw: deferred.trim_decision(stats, 10, 1.0, "echo_range", **kw)  # noqa: E731
    for n_r in (10, 7, 1):
        np.testing.assert_array_equal(decide((_rmax_for(n_r), 0)), np.arange(0, n_r + 1.0))
    for stats in ((_rmax_for(0), 0), (_rmax_for(11), 0), (float("nan"), 0), (float("-inf"), 0), None):
        assert decide(stats) is None
    assert not caplog.records
    # range_var_max: the maximum is r_cap whatever the statistics say
    for hi in (3.2, 1e9, float("nan")):
        np.testing.assert_array_equal(decide((hi, 0), range_var_max="7m", r_cap=7 + 1e-8), np.arange(0, 7 + 1e-8 + 1, 1.0))
    assert len(decide((3.2, 0), range_var_max="7m", r_cap=7 + 1e-8)) - 1 == 8
    assert decide(None, range_var_max="7m", r_cap=7 + 1e-8) is None  # (no statistics: the fallback, as before)


def test_trim_decision_without_a_fallback_raises_the_two_errors():
    decide = lambda stats: deferred.trim_decision(stats, 10, 1.0, "depth", has_fallback=False)  # noqa: E731
    with pytest.raises(ValueError, match="range bins are empty"):
        decide((float("nan"), 0))
    with pytest.raises(RuntimeError, match=r"nanmax\(depth\) = 10.5 lies beyond the range grid the shards agreed on"):
        decide((_rmax_for(11), 0))
    assert len(decide((_rmax_for(0), 0))) == 1       # an empty grid is the reference's answer: returned as it is
    assert len(decide((_rmax_for(7), 3))) - 1 == 7


def test_nan_coordinate_warning_exactly_when_the_trim_succeeds(caplog):
    caplog.set_level(logging.WARNING)
    assert deferred.trim_decision((_rmax_for(11), 5), 10, 1.0, "depth") is None
    assert deferred.trim_decision((float("nan"), 5), 10, 1.0, "depth") is None
    assert deferred.trim_decision((_rmax_for(7), 0), 10, 1.0, "depth") is not None
    assert not caplog.records
    assert deferred.trim_decision((_rmax_for(7), 2), 10, 1.0, "depth") is not None
    assert len(caplog.records) == 1
    msg = caplog.records[0].getMessage()
    assert msg.startswith("The ```depth``` coordinate array contain NaNs. Aggregation may be negatively impacted")


def test_deferred_mvbs_calls_the_fallback_once_with_the_snapshot():
    """The fallback branches of the shared assembly need no device: the fallback gets the snapshot taken at call time
    and its answer is the result -- once, at first use when deferred, inside the call otherwise."""
    ds = Dataset(coords={"channel": np.array(["a"])})
    ds.attrs["tag"] = "at call time"
    grid, bins = (np.zeros(1, "datetime64[ns]"), 0, 1), np.zeros((1, 1, 10))
    for stats in ((_rmax_for(0), 0), (_rmax_for(11), 0), (float("nan"), 0), None):
        calls = []

        def fallback(snap):
            calls.append(snap.attrs["tag"])
            return Dataset(coords={"x": np.arange(3)})

        out = deferred.deferred_mvbs(ds, bins, 10, lambda: stats, None, 10.5, grid, "echo_range", 1.0, "20s",
                                     fallback=fallback)
        ds.attrs["tag"] = "edited after the call"
        assert calls == []
        assert out.sizes["x"] == 3 and out.sizes["x"] == 3 and calls == ["at call time"]
        ds.attrs["tag"] = "at call time"
        now = deferred.deferred_mvbs(ds, bins, 10, lambda: stats, None, 10.5, grid, "echo_range", 1.0, "20s",
                                     fallback=fallback, defer=False)
        assert calls == ["at call time"] * 2 and now.sizes["x"] == 3
    # ... and without one the error surfaces at first use, and again at every later access
    out = deferred.deferred_mvbs(ds, bins, 10, lambda: (float("nan"), 0), None, 10.5, grid, "echo_range", 1.0, "20s")
    for _ in range(2):
        with pytest.raises(ValueError, match="range bins are empty"):
            out.attrs


def test_range_cap_precedence():
    assert deferred.range_cap("150m", 99.0) == 150 + 1e-8
    assert deferred.range_cap(None, 99.0) == 99.0
    assert deferred.range_cap(None, None) is None  # (no rows to reduce: the caller has no cap)
