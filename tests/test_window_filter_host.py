"""clean.window_filter without a GPU: the export and its signature, the properties of the NumPy restatement of its rule
(tests/window_filter_ref.py, the oracle of the kernel), an independent cross-check of that oracle against scipy.ndimage,
and every refusal of the public function, of the tensor-level wrapper and of the C entry (they all come before any
device access)."""
import inspect
import os

import numpy as np
import pytest

from window_filter_ref import METHODS, window_filter_ref, windows

NAN, INF = np.nan, np.inf
SIZES = [(1, 1), (3, 3), (1, 15), (15, 1), (7, 5), (15, 15)]


def _field(seed, shape, dtype=np.float64, nan_share=0.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(-70.0, 4.0, shape)
    if nan_share:
        x[rng.random(shape) < nan_share] = NAN
    return x.astype(dtype)


def _lin(v):
    return np.power(10.0, np.asarray(v, dtype=np.float64) / 10.0)


def test_export_signature_and_constants():
    import echopype_amd as ep
    from echopype_amd import _lib, ops

    assert "window_filter" in ep.clean.__all__ and callable(ops.window_filter)
    P = inspect.Parameter
    kw = P.POSITIONAL_OR_KEYWORD
    assert inspect.signature(ep.clean.window_filter) == inspect.Signature([
        P("ds_Sv", kw), P("method", kw, default="median"), P("ping_num", kw, default=3), P("range_sample_num", kw, default=3),
        P("var_name", kw, default="Sv"), P("min_valid", kw, default=1), P("keep_nan", kw, default=True)])
    assert inspect.signature(ops.window_filter) == inspect.Signature([
        P("x", kw), P("method", kw), P("ping_num", kw), P("range_sample_num", kw), P("min_valid", P.KEYWORD_ONLY, default=1),
        P("keep_nan", P.KEYWORD_ONLY, default=True), P("out", P.KEYWORD_ONLY, default=None),
        P("_max_grid", P.KEYWORD_ONLY, default=0)])
    assert len(_lib.SIGNATURES["epa_window_filter"]) == 13 and hasattr(_lib.lib, "epa_window_filter")
    header = open(os.path.join(__import__("conftest").ROOT, "include", "echopype_amd.h")).read()
    assert f"#define EPA_WINDOW_FILTER_MAX {_lib.WINDOW_FILTER_MAX} " in header and _lib.WINDOW_FILTER_MAX == 15
    assert f"#define EPA_WINDOW_FILTER_TP {_lib.WINDOW_FILTER_TP} " in header
    assert f"#define EPA_WINDOW_FILTER_TS {_lib.WINDOW_FILTER_TS} " in header
    assert ("enum epa_window_method { EPA_WINDOW_MEDIAN = 0, EPA_WINDOW_MEAN = 1, EPA_WINDOW_MIN = 2, EPA_WINDOW_MAX = 3 }"
            in header)
    assert _lib.WINDOW_METHODS == METHODS == ("median", "mean", "min", "max")
    assert (_lib.WINDOW_MEDIAN, _lib.WINDOW_MEAN, _lib.WINDOW_MIN, _lib.WINDOW_MAX) == (0, 1, 2, 3)
    for word in ("metres", "Boolean masks".lower(), "weighted", "sharded"):
        assert word in ep.clean.window_filter.__doc__  # what is out of scope is said


# ---- the oracle's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_window_of_one_sample_is_the_identity(dtype):
    x = _field(1, (2, 9, 11), dtype, nan_share=0.2)
    x[0, 2, 3], x[1, 4, 5] = -INF, INF
    for method in METHODS:
        y = window_filter_ref(x, method, 1, 1)
        assert y.dtype == x.dtype
        if method == "mean" and dtype == np.float64:  # (the one method with a round trip through the exponential)
            np.testing.assert_allclose(y, x, rtol=0, atol=1e-12)
        else:
            np.testing.assert_array_equal(y, x)


@pytest.mark.parametrize("size", SIZES[1:])
def test_median_and_mean_lie_between_min_and_max(size):
    x = _field(2, (2, 19, 23), nan_share=0.3)
    x[0, 5, 5], x[1, 7, 9] = -INF, INF
    lo, hi = (window_filter_ref(x, m, *size, keep_nan=False) for m in ("min", "max"))
    for m in ("median", "mean"):
        y = window_filter_ref(x, m, *size, keep_nan=False)
        np.testing.assert_array_equal(np.isnan(y), np.isnan(lo))
        ok = ~np.isnan(y)
        assert (lo[ok] <= y[ok] + 1e-12).all() and (y[ok] <= hi[ok] + 1e-12).all()
    assert (lo[ok] <= hi[ok]).all()


def test_the_median_is_the_linear_nanmedian_and_the_mean_the_linear_nanmean():
    """The selection form of the oracle's median against the expression the rule names, 10 log10(nanmedian(10^(v/10)));
    odd counts and equal middle values come back as the inputs themselves."""
    x = np.round(_field(3, (17, 21), nan_share=0.25) * 2) / 2  # (quantised: ties)
    for size in SIZES:
        w = windows(x, *size)
        some = ~np.isnan(w).all(axis=-1)
        y, n = window_filter_ref(x, "median", *size, keep_nan=False, with_count=True)
        np.testing.assert_array_equal(n, (~np.isnan(w)).sum(axis=-1))
        want = np.full(x.shape, NAN)
        want[some] = 10.0 * np.log10(np.nanmedian(_lin(w[some]), axis=-1))
        np.testing.assert_allclose(y, want, rtol=0, atol=1e-12, equal_nan=True)
        odd = some & (n % 2 == 1)
        np.testing.assert_array_equal(y[odd], np.nanmedian(w[odd], axis=-1))  # an input, bit for bit
        assert np.isin(y[odd], x[~np.isnan(x)]).all()
        m = window_filter_ref(x, "mean", *size, keep_nan=False)
        want[some] = 10.0 * np.log10(np.nanmean(_lin(w[some]), axis=-1))
        np.testing.assert_allclose(m, want, rtol=0, atol=1e-12, equal_nan=True)
    # two different middle values: the linear mean of the two, not the mean of the decibels
    pair = np.array([[-80.0, -60.0]])
    np.testing.assert_allclose(window_filter_ref(pair, "median", 1, 3), 10 * np.log10((1e-8 + 1e-6) / 2), rtol=0, atol=1e-12)


def test_infinities_are_values():
    x = np.array([[-INF, -INF, -INF, -70.0, INF, -60.0, NAN, NAN]])
    mean = window_filter_ref(x, "mean", 1, 3)
    assert mean[0, 0] == -INF and mean[0, 1] == -INF and np.isfinite(mean[0, 2]) and mean[0, 3] == INF and mean[0, 5] == INF
    assert np.isnan(mean[0, 6]) and np.isnan(mean[0, 7])
    np.testing.assert_array_equal(window_filter_ref(x, "min", 1, 3, keep_nan=False), [[-INF, -INF, -INF, -INF, -70, -60, -60, NAN]])
    np.testing.assert_array_equal(window_filter_ref(x, "max", 1, 3, keep_nan=False), [[-INF, -INF, -70, INF, INF, INF, -60, NAN]])
    med = window_filter_ref(x, "median", 1, 3, keep_nan=False)
    np.testing.assert_array_equal(med[0, [0, 1, 2, 3, 7]], [-INF, -INF, -INF, -70.0, NAN])
    assert med[0, 4] == -60.0 and med[0, 5] == INF and med[0, 6] == -60.0  # (-70, inf, -60); (inf, -60): linear mean; (-60)


def test_keep_nan_and_min_valid_act_as_stated():
    x = _field(4, (13, 17), nan_share=0.4)
    for method in METHODS:
        kept = window_filter_ref(x, method, 3, 5)
        filled = window_filter_ref(x, method, 3, 5, keep_nan=False)
        assert np.isnan(kept[np.isnan(x)]).all()
        np.testing.assert_array_equal(kept[~np.isnan(x)], filled[~np.isnan(x)])
        assert (~np.isnan(filled[np.isnan(x)])).any()  # samples are filled in
        _, n = window_filter_ref(x, method, 3, 5, keep_nan=False, with_count=True)
        for mv in (1, 6, 15):
            y = window_filter_ref(x, method, 3, 5, min_valid=mv, keep_nan=False)
            np.testing.assert_array_equal(np.isnan(y), n < max(mv, 1))
            np.testing.assert_array_equal(y[n >= mv], filled[n >= mv])
    # min_valid at the window size: only whole windows without a NaN survive, so every edge sample is NaN
    y = window_filter_ref(_field(5, (9, 9)), "median", 3, 3, min_valid=9)
    assert np.isnan(y[0]).all() and np.isnan(y[:, -1]).all() and not np.isnan(y[1:-1, 1:-1]).any()


def test_a_window_larger_than_the_array_is_the_statistic_of_the_whole_plane():
    x = _field(6, (2, 3, 5), nan_share=0.2)
    x[0, 1, 1] = -INF
    for method, whole in (("min", np.nanmin), ("max", np.nanmax), ("median", lambda a: 10 * np.log10(np.nanmedian(_lin(a)))),
                          ("mean", lambda a: 10 * np.log10(np.nanmean(_lin(a))))):
        y = window_filter_ref(x, method, 15, 15, keep_nan=False)
        for c in range(2):
            np.testing.assert_allclose(y[c], np.full((3, 5), whole(x[c])), rtol=0, atol=1e-12)


def test_channels_are_filtered_on_their_own_and_planes_need_no_channel():
    x = _field(7, (3, 8, 9), nan_share=0.1)
    for method in METHODS:
        y = window_filter_ref(x, method, 5, 3)
        for c in range(3):
            np.testing.assert_array_equal(y[c], window_filter_ref(x[c], method, 5, 3))
    assert window_filter_ref(x[:, :0], "median", 3, 3).shape == (3, 0, 9)


# ---- an independent cross-check ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 3), (5, 5), (7, 5), (1, 15), (15, 1)])
def test_against_scipy_ndimage_away_from_the_edges(size):
    ndi = pytest.importorskip("scipy.ndimage")
    x = _field(8, (40, 37))
    hp, hs = size[0] // 2, size[1] // 2
    inner = (slice(hp, x.shape[0] - hp), slice(hs, x.shape[1] - hs))
    np.testing.assert_array_equal(window_filter_ref(x, "median", *size)[inner], ndi.median_filter(x, size=size)[inner])
    np.testing.assert_array_equal(window_filter_ref(x, "min", *size)[inner], ndi.minimum_filter(x, size=size)[inner])
    np.testing.assert_array_equal(window_filter_ref(x, "max", *size)[inner], ndi.maximum_filter(x, size=size)[inner])
    got = _lin(window_filter_ref(x, "mean", *size)[inner])
    want = ndi.uniform_filter(_lin(x), size=size)[inner]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
DIMS = ("channel", "ping_time", "range_sample")


def _ds(dims=DIMS, dtype=np.float64):
    from echopype_amd.xr_lite import Dataset

    sizes = {"channel": 2, "ping_time": 4, "range_sample": 5, "beam": 3}
    ds = Dataset(coords={"channel": np.array(["a", "b"]), "range_sample": np.arange(5),
                         "ping_time": np.datetime64("2026-01-01", "ns") + np.arange(4) * np.timedelta64(1, "s")})
    ds["Sv"] = (dims, np.zeros(tuple(sizes[d] for d in dims), dtype=dtype))
    return ds


BAD_ARGS = [
    (dict(method="mode"), "method must be one of"),
    (dict(method=0), "method must be one of"),
    (dict(ping_num=2), "ping_num must be an odd integer within 1 .. 15"),
    (dict(ping_num=17), "ping_num must be an odd integer within 1 .. 15"),
    (dict(ping_num=-1), "ping_num must be an odd integer within 1 .. 15"),
    (dict(ping_num=3.0), "ping_num must be an odd integer within 1 .. 15"),
    (dict(range_sample_num=0), "range_sample_num must be an odd integer within 1 .. 15"),
    (dict(range_sample_num=4), "range_sample_num must be an odd integer within 1 .. 15"),
    (dict(range_sample_num=True), "range_sample_num must be an odd integer within 1 .. 15"),
    (dict(min_valid=0), r"min_valid must be an integer within 1 \.\. 9"),
    (dict(min_valid=10), r"min_valid must be an integer within 1 \.\. 9"),
    (dict(min_valid=1.5), r"min_valid must be an integer within 1 \.\. 9"),
    (dict(ping_num=5, range_sample_num=1, min_valid=6), r"min_valid must be an integer within 1 \.\. 5"),
]


def test_refusals_of_the_public_function(monkeypatch):
    import torch

    import echopype_amd as ep
    from echopype_amd import ops

    def no_device(*a, **k):
        raise AssertionError("a refusal must come before any device access")

    monkeypatch.setattr(ops, "window_filter", no_device)
    monkeypatch.setattr(ops, "to_device", no_device)
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    wf = ep.clean.window_filter
    for kw, match in BAD_ARGS:
        with pytest.raises(ValueError, match="clean.window_filter: " + match):
            wf(_ds(), **kw)
    with pytest.raises(ValueError, match="has no variable 'Sv_corrected'"):
        wf(_ds(), var_name="Sv_corrected")
    with pytest.raises(ValueError, match="has no variable"):
        wf(_ds(), var_name="channel")  # (a coordinate is not a variable to filter)
    for dtype in (np.int32, bool, np.complex128):
        with pytest.raises(ValueError, match="Sv must be floating"):
            wf(_ds(dtype=dtype))
    for dims in (("channel", "range_sample", "ping_time"), ("ping_time", "channel", "range_sample"), ("range_sample",),
                 ("beam", "channel", "ping_time", "range_sample"), ("ping_time", "beam")):
        with pytest.raises(ValueError, match=r"must lie over \(\.\.\., 'ping_time', 'range_sample'\)"):
            wf(_ds(dims))


def test_the_wrapper_refuses_before_it_calls(monkeypatch):
    import torch

    from echopype_amd import _lib, ops

    def no_call(*a, **k):
        raise AssertionError("a refusal must come before the library is called")

    monkeypatch.setattr(ops, "call", no_call)
    x = torch.zeros(2, 4, 5)
    for kw, match in BAD_ARGS:
        args = dict(method="median", ping_num=3, range_sample_num=3, min_valid=1)
        args.update(kw)
        with pytest.raises(ValueError, match="window_filter: " + match):
            ops.window_filter(x, args["method"], args["ping_num"], args["range_sample_num"], min_valid=args["min_valid"])
    for bad in (torch.zeros(5), torch.zeros(1, 2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.float16),
                np.zeros((2, 3))):
        with pytest.raises(ValueError, match=r"x must be a float32 / float64 tensor of shape \(C, P, S\) or \(P, S\)"):
            ops.window_filter(bad, "median", 3, 3)
    with pytest.raises(ValueError, match="x must be on the device"):
        ops.window_filter(x, "mean", 3, 3)
    assert ops.window_filter_args("max", np.int64(15), 1, np.int32(15)) == (_lib.WINDOW_MAX, 15, 1, 15)


def _call(x=4096, dtype=0, shape=(1, 4, 5), method=0, ping_num=3, range_sample_num=3, min_valid=1, keep_nan=1, out=8192,
          max_grid=0):
    from echopype_amd import _lib

    _lib.call("epa_window_filter", x, dtype, *shape, method, ping_num, range_sample_num, min_valid, keep_nan, out, max_grid, None)


def test_the_library_refuses_bad_arguments_before_any_hip_call():
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match=f"epa_window_filter: bad dtype {bad}"):
            _call(dtype=bad)
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=f"epa_window_filter: bad method {bad}"):
            _call(method=bad)
    for shape in ((-1, 4, 5), (1, -4, 5), (1, 4, -5)):
        with pytest.raises(ValueError, match="bad shape"):
            _call(shape=shape)
    for pn, rn in ((2, 3), (3, 0), (17, 3), (3, 16), (-3, 3), (3, -1)):
        with pytest.raises(ValueError, match="the window sizes must be odd and within 1 .. 15"):
            _call(ping_num=pn, range_sample_num=rn)
    for mv in (0, -1, 10):
        with pytest.raises(ValueError, match=r"min_valid must be within 1 \.\. 9"):
            _call(min_valid=mv)
    with pytest.raises(ValueError, match="max_grid must not be negative"):
        _call(max_grid=-1)
    for kw in (dict(x=None), dict(out=None)):
        with pytest.raises(ValueError, match="NULL array argument"):
            _call(**kw)
    # 1 x 4 x 5 float32 = 80 bytes: the same array, a shifted one on either side; the first byte behind the other is allowed
    for out in (4096, 4096 + 4, 4096 - 76, 4096 + 79):
        with pytest.raises(ValueError, match="out overlaps x"):
            _call(out=out)
    with pytest.raises(ValueError, match="out overlaps x"):
        _call(dtype=1, out=4096 + 159)
    with pytest.raises(ValueError, match="tiles do not fit one launch"):
        _call(shape=(1 << 20, 1 << 20, 1 << 20))
    # nothing to do: no launch and no complaint, whatever the pointers
    for shape in ((0, 4, 5), (1, 0, 5), (1, 4, 0)):
        _call(x=None, out=None, shape=shape)
