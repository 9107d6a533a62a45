"""mask.regrid_mask without a GPU: the validation errors that need no device, and the NumPy judge of the GPU tests
(tests/regrid_mask_ref.py) against pandas -- ``pd.cut`` on ``IntervalIndex.from_breaks`` for the membership on both
axes, ``Series.resample(...).first().index`` for the time edges."""
import numpy as np
import pandas as pd
import pytest

import regrid_mask_ref as R

T0 = np.datetime64("2021-03-04T10:00:00", "ns").astype(np.int64)
S = 10**9


def _da(data, dims, coords=None, name="mask"):
    from echopype_amd.xr_lite import DataArray

    return DataArray(np.asarray(data), dims, coords=coords, name=name)


def _inputs(P=4, D=4, T=None, dtype=np.int64):
    pt = (T0 + S * np.arange(P)).view("datetime64[ns]")
    shape, dims = ((P, D), ("ping_time", "depth")) if T is None else ((T, P, D), ("beam", "ping_time", "depth"))
    return (_da(np.ones(shape, dtype), dims, {"ping_time": pt, "depth": np.arange(D)}),
            _da(np.arange(D, dtype=np.float64), ("depth",), {"depth": np.arange(D)}, name="depth"))


@pytest.mark.parametrize("change, kw, typ, msg", [
    (None, {"method": "blockwise"}, ValueError, "Passing in reindex=False is only allowed when method='map_reduce'."),
    (None, {"method": "cohorts", "reindex": True}, ValueError,
     "Passing in reindex=True is only allowed when method='map_reduce'."),
    (None, {"ping_time_bin": 20}, TypeError, "ping_time_bin must be a string"),
    ("3d", {}, ValueError, "Mask must have only 2 dimensions unless 'third_dim' is specified."),
    (None, {"third_dim": "beam"}, ValueError, "Mask must contain the specified 'beam' as a dimension."),
    ("4d", {"third_dim": "beam"}, ValueError, "Mask must have 3 dimensions when 'third_dim' is specified."),
    ("two", {}, ValueError, "Mask must be binary True/False or 1/0."),
    ("nan", {}, ValueError, "Mask must be binary True/False or 1/0."),
    ("two", {"func": "logical-XOR"}, ValueError, "Mask must be binary True/False or 1/0."),
    ("two-u8", {"func": "logical-XOR"}, ValueError, "Mask must be binary True/False or 1/0."),
    (None, {"func": "logical-XOR"}, ValueError, "'func' must be 'logical-AND' or 'logical-OR'."),
    ("u8", {"func": "mean"}, ValueError, "'func' must be 'logical-AND' or 'logical-OR'."),
    ("bool", {"func": "mean"}, ValueError, "'func' must be 'logical-AND' or 'logical-OR'."),
])
def test_validation_errors_in_the_reference_order(change, kw, typ, msg):
    import echopype_amd as ep

    mask, rng = _inputs()
    if change == "3d":
        mask, _ = _inputs(T=2)
    elif change == "4d":
        m3, _ = _inputs(T=2)
        mask = _da(m3.values[None], ("x",) + m3.dims, m3.coords)
    elif change in ("two", "two-u8"):
        v = mask.values.astype(np.uint8 if change == "two-u8" else np.int64)
        v[1, 2] = 2
        mask = _da(v, mask.dims, mask.coords)
    elif change == "nan":
        v = mask.values.astype(np.float64)
        v[0, 0] = np.nan
        mask = _da(v, mask.dims, mask.coords)
    elif change in ("u8", "bool"):
        mask = _da(mask.values.astype(np.uint8 if change == "u8" else bool), mask.dims, mask.coords)
    with pytest.raises(Exception) as ei:
        ep.mask.regrid_mask(mask, rng, **kw)
    assert type(ei.value) is typ and str(ei.value) == msg


def test_method_comes_before_everything_else():
    import echopype_amd as ep

    with pytest.raises(ValueError, match="only allowed when method='map_reduce'"):
        ep.mask.regrid_mask(None, None, ping_time_bin=3, method="blockwise")


# ---- the judge against pandas ------------------------------------------------------------------------------------------
def _cut(x, edges, closed):
    """pandas' membership: codes of pd.cut on the IntervalIndex of the edges (-1: none)."""
    return np.asarray(pd.cut(x, pd.IntervalIndex.from_breaks(edges, closed=closed)).codes)


def _pandas_time_edges(ping_ns, bin_str):
    idx = pd.Series(0, index=pd.DatetimeIndex(np.asarray(ping_ns).view("datetime64[ns]"))).resample(bin_str).first().index
    return idx.union([idx[-1] + pd.Timedelta(bin_str)]).values.astype("datetime64[ns]").view(np.int64)


def _pandas_regrid(mask, ping_ns, rng, range_bin, bin_str, func, closed, third):
    """The reference's computation with pandas in place of flox: group-by mean over the cut codes, then the test."""
    T, P, D = mask.shape
    tedges = _pandas_time_edges(ping_ns, bin_str)
    redges = R.range_edges(rng, range_bin)
    ti = _cut(pd.DatetimeIndex(np.asarray(ping_ns).view("datetime64[ns]")), pd.DatetimeIndex(tedges.view("datetime64[ns]")),
              closed)
    ri = _cut(np.broadcast_to(np.asarray(rng, dtype=np.float64), (P, D)).reshape(-1), redges, closed).reshape(P, D)
    uniq = np.unique(third)
    df = pd.DataFrame({"g": np.repeat(np.searchsorted(uniq, third), P * D), "t": np.tile(np.repeat(ti, D), T),
                       "r": np.tile(ri.reshape(-1), T), "v": mask.reshape(-1).astype(np.float64)})
    df = df[(df.t >= 0) & (df.r >= 0)]
    mean = np.zeros((len(uniq), len(tedges) - 1, len(redges) - 1))  # fill_value = 0.0
    for (g, t, r), m in df.groupby(["g", "t", "r"]).v.mean().items():
        mean[g, t, r] = m
    return tedges, redges, (mean == 1.0) if func == "logical-AND" else (mean != 0.0)


def _random_case(seed):
    rng = np.random.default_rng(seed)
    T, P, D = int(rng.integers(1, 4)), int(rng.integers(1, 40)), int(rng.integers(1, 25))
    bin_s = int(rng.choice([5, 20, 60]))
    # pings: whole and fractional seconds, some exactly on a time edge, now and then a gap of several bins
    steps = rng.choice([0, S // 2, S, 3 * S, bin_s * S], size=P, p=[0.1, 0.2, 0.4, 0.2, 0.1])
    if seed % 3 == 0:
        steps[P // 2] += 3 * bin_s * S
    start = T0 + (0 if seed % 2 else 7 * S)  # (T0 is on an edge of every bin size used)
    ping_ns = start + np.cumsum(steps) - steps[0]
    range_bin = float(rng.choice([0.5, 1.0, 2.5, 10.0]))
    depth = np.sort(rng.choice(np.arange(0, 60) * range_bin / 4, size=D, replace=False))  # many exactly on an edge
    rng2d = seed % 4 == 1
    if rng2d:
        depth = depth[None, :] + rng.choice([0.0, range_bin / 4], size=(P, 1))
        depth = np.where(rng.random((P, D)) < 0.1, np.nan, depth)
        if np.isnan(depth).all():
            depth[0, 0] = 0.0
    mask = (rng.random((T, P, D)) < rng.choice([0.5, 0.9, 1.0])).astype(np.int64)
    third = rng.integers(0, 3, size=T)
    return mask, ping_ns, depth, range_bin, bin_s, third


@pytest.mark.parametrize("seed", range(30))
def test_judge_against_pandas(seed):
    mask, ping_ns, depth, range_bin, bin_s, third = _random_case(seed)
    for closed in ("left", "right"):
        for func in ("logical-AND", "logical-OR"):
            uniq, tedges, redges, got = R.regrid(mask, ping_ns, depth, range_bin, bin_s * S, func, closed, third=third)
            ptedges, predges, want = _pandas_regrid(mask, ping_ns, depth, range_bin, f"{bin_s}s", func, closed, third)
            np.testing.assert_array_equal(tedges, ptedges)
            np.testing.assert_array_equal(redges, predges)
            np.testing.assert_array_equal(uniq, np.unique(third))
            np.testing.assert_array_equal(got.astype(bool), want, err_msg=f"{seed} {closed} {func}")
            np.testing.assert_array_equal(
                R.regrid_by_counts(mask, ping_ns, depth, range_bin, bin_s * S, func, closed, third=third)[3], got)


@pytest.mark.parametrize("closed", ["left", "right"])
def test_membership_on_tenth_of_a_metre_edges(closed):
    """range_bin = 0.1: the edges are i*0.1 as np.arange computes them (3*0.1 = 0.30000000000000004), a depth given as
    the decimal literal next to one (0.3) lies on the other side of it."""
    edges = R.range_edges([2.0], 0.1)
    np.testing.assert_array_equal(edges[:21], np.arange(21) * 0.1)
    x = np.concatenate([np.arange(1, 20) * 0.1, np.array([0.3, 0.6, 0.7, 1.2, 1.4, 1.7, 1.9])])
    assert (x[2] != x[19]) and x[2] == edges[3]
    got = R.member(x, edges, closed)
    np.testing.assert_array_equal(got, _cut(x, edges, closed))
    assert got[2] == (3 if closed == "left" else 2) and got[19] == 2  # on the edge 3*0.1 | just below it


def test_ping_on_an_edge_and_an_empty_bin():
    ping_ns = T0 + S * np.array([0, 5, 20, 39, 80, 81])  # 0, 20 and 80 are edges of the 20 s bins; [40, 60), [60, 80) empty
    for closed in ("left", "right"):
        tedges = R.time_edges(ping_ns, 20 * S)
        np.testing.assert_array_equal(tedges, _pandas_time_edges(ping_ns, "20s"))
        assert len(tedges) == 6
        got = R.member(ping_ns, tedges, closed)
        np.testing.assert_array_equal(got, _cut(pd.DatetimeIndex(ping_ns.view("datetime64[ns]")),
                                                pd.DatetimeIndex(tedges.view("datetime64[ns]")), closed))
        np.testing.assert_array_equal(got, [0, 0, 1, 1, 4, 4] if closed == "left" else [-1, 0, 0, 1, 3, 4])
    mask = np.ones((1, 6, 2), dtype=bool)
    out = R.regrid(mask, ping_ns, [1.0, 2.0], 5.0, 20 * S)[3]
    np.testing.assert_array_equal(out[0, :, 0], [True, True, False, False, True])
