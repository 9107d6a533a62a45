"""clean.window_filter on the GPU (csrc/window_filter.hip through ops.window_filter and clean.window_filter) against
its NumPy restatement (tests/window_filter_ref.py).

The judge: the NaN pattern and the infinities are the oracle's; ``min``, ``max`` and the medians of an odd count of
valid values are selections and equal the oracle's as values (``==``); the mean and the medians of an even count are
within 1e-9 in float64 and within one float32 ulp of the oracle's rounded value in float32 -- kernel and oracle both
compute in float64 and round once (the rule of test_gpu_regrid.py).  The oracle works on the float64 copy of a float32
input, which holds the same numbers, so one evaluation serves both types.  Outputs are pre-filled with a value no
result can take, so an element the kernel left out shows; the launch trace names the kernel that ran.  The seam shapes
come from the tile the library exports."""
import numpy as np
import pytest

from window_filter_ref import METHODS, finish, window_filter_ref, window_results

pytestmark = pytest.mark.gpu

SENTINEL = 777.0  # (Sv here is at most -30 dB or infinite)
NAN, INF = np.nan, np.inf
WINDOWS = [(1, 1), (3, 3), (1, 15), (15, 1), (7, 5), (15, 15)]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd as ep

    return torch, ep


def _tile():
    from echopype_amd import _lib

    return _lib.WINDOW_FILTER_TP, _lib.WINDOW_FILTER_TS, _lib.WINDOW_FILTER_MAX


def _judge(got, want, n, method, what):
    """``got`` against the oracle's ``want`` (both of the input's type); ``n``: the oracle's count of valid values."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    inf = np.isinf(got) | np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf], err_msg=what)
    f = np.isfinite(want)
    exact = f if method in ("min", "max") else (f & (n % 2 == 1) if method == "median" else np.zeros_like(f))
    np.testing.assert_array_equal(got[exact], want[exact], err_msg=what + " (a selection)")
    f = f & ~exact
    err = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64))
    tol = 1e-9 if want.dtype == np.float64 else np.spacing(np.abs(want[f])).astype(np.float64)
    if err.size:
        print(f"{what}: largest error {err.max():.3e}, {int((err > 0).sum())} of {err.size} differ")
    assert (err <= tol).all(), what


def _run(torch, x, method, pn, rn, min_valid=1, keep_nan=True, max_grid=0):
    """ops.window_filter into a pre-filled output -> the result on the host."""
    from echopype_amd import _lib, ops

    x_t = torch.as_tensor(x).cuda()
    out = torch.full(x.shape, SENTINEL, dtype=x_t.dtype, device="cuda")
    with _lib.launch_trace() as tr:
        got = ops.window_filter(x_t, method, pn, rn, min_valid=min_valid, keep_nan=keep_nan, out=out, _max_grid=max_grid)
    assert tr.kernels == ([f"window_filter_kernel<{method}>"] if x.size else []), tr.kernels
    assert got is out
    host = out.cpu().numpy()
    assert not (host == SENTINEL).any(), "an element was not written"
    np.testing.assert_array_equal(x_t.cpu().numpy(), x)  # (the input is only read)
    return host


def _check_all(torch, x64, pn, rn, what, methods=METHODS, dtypes=DTYPES, min_valid=1, keep_nan=True, max_grid=0, results=None):
    """Every method and type on ``x64`` (float64 holding float32 numbers) against ONE evaluation of the oracle."""
    res, n = results if results is not None else window_results(x64, pn, rn)
    for dtype in dtypes:
        x = x64.astype(dtype)
        for method in methods:
            want = finish(res[method], n, x, min_valid, keep_nan)
            got = _run(torch, x, method, pn, rn, min_valid, keep_nan, max_grid)
            _judge(got, want, n, method, f"{what} {method} {pn}x{rn} {np.dtype(dtype).name} min_valid={min_valid} "
                                         f"keep_nan={keep_nan}")
    return res, n


def scene(seed, shape, nan_share=0.03, quantised=False):
    """dB noise around -70 with single-sample spikes, a NaN pad behind a ragged count per ping, a fully NaN ping and a
    fully NaN sample column, isolated NaN samples, and -inf / +inf alone and inside one window together -- as float64
    that holds float32 numbers."""
    rng = np.random.default_rng(seed)
    x = rng.normal(-70.0, 3.0, shape)
    C, P, S = shape
    if quantised:
        x = np.round(x)  # many equal values inside a window: ties for the median
    spikes = rng.random(shape) < 0.02
    x[spikes] = -35.0 + rng.normal(0, 1, int(spikes.sum()))
    x[rng.random(shape) < nan_share] = NAN  # isolated
    if S > 4:
        count = rng.integers(S // 2, S + 1, (C, P))  # ragged: samples behind it are the pad
        x[np.arange(S)[None, None, :] >= count[:, :, None]] = NAN
        x[:, :, S // 3] = NAN
    if P > 4:
        x[:, P // 2, :] = NAN
    if P > 8 and S > 6:
        x[0, 1, 1] = -INF
        x[0, 3, 5] = INF
        x[-1, 6, 2], x[-1, 7, 3] = -INF, INF  # together in every window of 3 x 3 and more around (6, 2) .. (7, 3)
    elif P * S > 2:
        x[0, 0, 0] = -INF
        x[-1, -1, -1] = INF
    return x.astype(np.float32).astype(np.float64)


def _seam_shapes():
    TP, TS, _ = _tile()
    return [(P, S) for P in (1, TP - 1, TP, TP + 1, 2 * TP + 1) for S in (1, 7, TS - 1, TS, TS + 1, 2 * TS + 3)]


@pytest.mark.parametrize("shape", _seam_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_seams(env, shape):
    """Three channels of every seam shape, every window and method, both types; min_valid and keep_nan vary with the
    window so that every setting meets every shape.  The first channel alone as (1, P, S) and as a plane (P, S) gives
    that channel's part of the three-channel result: a window never crosses channels."""
    torch, _ = env
    P, S = shape
    x = scene(1000 + 131 * P + S, (3, P, S))
    for k, (pn, rn) in enumerate(WINDOWS):
        min_valid = (1, pn * rn, (pn * rn + 1) // 2)[k % 3]
        res, n = _check_all(torch, x, pn, rn, f"{P}x{S}", min_valid=min_valid, keep_nan=bool(k % 2))
        if (pn, rn) == (3, 3):
            one = {m: r[:1] for m, r in res.items()}, n[:1]
            _check_all(torch, x[:1], pn, rn, f"C=1 {P}x{S}", results=one, dtypes=[DTYPES[(P + S) % 2]])
            plane = {m: r[0] for m, r in res.items()}, n[0]
            _check_all(torch, x[0], pn, rn, f"plane {P}x{S}", results=plane, dtypes=[DTYPES[(P + S + 1) % 2]], keep_nan=False)


def test_a_window_larger_than_the_array(env):
    """15 x 15 on 3 x 5: every window is the whole plane."""
    torch, _ = env
    x = scene(7, (2, 3, 5), nan_share=0.2)
    assert np.isneginf(x[0, 0, 0]) and np.isposinf(x[-1, -1, -1])
    res, n = _check_all(torch, x, 15, 15, "3x5", keep_nan=False)
    for c in range(2):
        assert (n[c] == n[c, 0, 0]).all() and 0 < n[c, 0, 0] < 15
    _check_all(torch, x, 15, 15, "3x5", results=(res, n), min_valid=int(n.max()))


@pytest.mark.parametrize("max_grid", [1, 2])
def test_the_tile_loop(env, max_grid):
    """Several tiles per workgroup: 2 x 3 x 3 tiles walked by one workgroup, and by two."""
    torch, _ = env
    TP, TS, _ = _tile()
    x = scene(11, (2, 2 * TP + 1, 2 * TS + 3))
    for pn, rn in ((3, 3), (7, 5), (15, 15)):
        _check_all(torch, x, pn, rn, f"max_grid={max_grid}", max_grid=max_grid, dtypes=[DTYPES[max_grid % 2]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_isolated_nan_and_min_valid(env, dtype):
    """A quantised field (many equal values in every window), a third of the samples NaN one by one: even counts of valid
    values everywhere, both keep_nan settings, min_valid at 1, in between and at the window size."""
    torch, _ = env
    TP, TS, _ = _tile()
    x = scene(13, (2, TP + 3, TS + 5), nan_share=0.3, quantised=True)
    for pn, rn in ((3, 3), (5, 7)):
        res, n = window_results(x, pn, rn)
        assert ((n % 2 == 0) & (n > 0)).sum() > x.size // 4
        for keep_nan in (True, False):
            for min_valid in (1, (pn * rn) // 2, pn * rn):
                _check_all(torch, x, pn, rn, "ties", dtypes=[dtype], min_valid=min_valid, keep_nan=keep_nan, results=(res, n))
    # a NaN-free quantised field: min_valid at the window size leaves exactly the samples half a window from the edges
    full = np.round(np.random.default_rng(17).normal(-70, 2, (1, TP + 3, TS + 5)))
    got = _run(torch, full.astype(dtype), "median", 3, 5, min_valid=15)
    assert np.isnan(got[0, 0]).all() and np.isnan(got[0, :, :2]).all() and not np.isnan(got[0, 1:-1, 2:-2]).any()
    np.testing.assert_array_equal(got, window_filter_ref(full.astype(dtype), "median", 3, 5, min_valid=15))


@pytest.mark.parametrize("dtype", DTYPES)
def test_infinities(env, dtype):
    """-inf and +inf alone and inside one window: values, in every method."""
    torch, _ = env
    x = np.full((1, 9, 12), -70.0)
    x[0, 1, 1] = -INF                      # alone
    x[0, 1, 9] = INF                       # alone
    x[0, 6, 4], x[0, 6, 5] = -INF, INF     # together
    x[0, 7, :] = NAN
    x[0, 8, :6], x[0, 8, 6:] = -INF, INF   # behind the NaN ping: windows that hold nothing but infinities
    res, n = _check_all(torch, x, 3, 3, "inf", dtypes=[dtype], keep_nan=False)
    assert np.isposinf(res["mean"][0, 6, 4]) and np.isposinf(res["max"][0, 5, 4]) and np.isneginf(res["min"][0, 5, 4])
    assert np.isneginf(res["mean"][0, 8, 0]) and np.isposinf(res["mean"][0, 8, 11]) and np.isposinf(res["mean"][0, 8, 5])
    assert np.isneginf(res["median"][0, 8, 1]) and np.isposinf(res["median"][0, 8, 10])
    _check_all(torch, x, 1, 5, "inf", dtypes=[dtype])


def test_fuzz(env):
    """Thirty seeded draws over shape, window, method, type, NaN share, min_valid and keep_nan."""
    torch, _ = env
    TP, TS, CAP = _tile()
    rng = np.random.default_rng(20261020)
    for k in range(30):
        shape = (int(rng.integers(1, 4)), int(rng.integers(1, 2 * TP + 4)), int(rng.integers(1, TS + 40)))
        pn, rn = (int(2 * rng.integers(0, CAP // 2 + 1) + 1) for _ in range(2))
        x = scene(int(rng.integers(1 << 30)), shape, nan_share=float(rng.choice([0.0, 0.05, 0.5, 0.95])),
                  quantised=bool(rng.integers(2)))
        _check_all(torch, x, pn, rn, f"draw {k} {shape}", methods=[METHODS[int(rng.integers(4))]],
                   dtypes=[DTYPES[int(rng.integers(2))]], min_valid=int(rng.integers(1, pn * rn + 1)),
                   keep_nan=bool(rng.integers(2)), max_grid=int(rng.choice([0, 0, 3])))


def test_channels_of_one_call_equal_the_planes_one_at_a_time(env):
    torch, _ = env
    from echopype_amd import ops

    TP, TS, _ = _tile()
    x = torch.as_tensor(scene(19, (3, TP + 2, TS + 9)).astype(np.float32)).cuda()
    for method in METHODS:
        whole = ops.window_filter(x, method, 5, 7, keep_nan=False)
        for c in range(3):
            plane = ops.window_filter(x[c], method, 5, 7, keep_nan=False)
            assert plane.shape == x[c].shape
            assert torch.equal(torch.nan_to_num(whole[c], nan=SENTINEL), torch.nan_to_num(plane, nan=SENTINEL)), (method, c)


def test_nothing_to_do_and_an_overlapping_out(env):
    torch, _ = env
    from echopype_amd import ops

    for shape in ((0, 4, 5), (2, 0, 5), (2, 4, 0), (0, 5)):
        for method in METHODS:
            assert _run(torch, np.zeros(shape, np.float32), method, 3, 3).shape == shape  # (no launch: _run checks the trace)
    buf = torch.zeros(2 * 4 * 5 + 5, device="cuda")
    x = buf[:40].view(2, 4, 5)
    for out in (x, buf[5:].view(2, 4, 5), buf[1:41].view(2, 4, 5)):
        with pytest.raises(ValueError, match="out overlaps x"):
            ops.window_filter(x, "median", 3, 3, out=out)
    with pytest.raises(ValueError, match="out must be a contiguous"):
        ops.window_filter(x, "median", 3, 3, out=torch.zeros(2, 4, 5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.window_filter(x.transpose(1, 2), "median", 3, 3)
    assert (buf == 0).all()


def test_no_host_synchronisation(env):
    """torch's synchronisation debug mode raises on any blocking call: ops.window_filter makes none."""
    torch, _ = env
    from echopype_amd import ops

    x = torch.as_tensor(scene(23, (2, 20, 70))).cuda()
    ops.window_filter(x, "mean", 3, 3)  # warm-up: the allocator's blocks
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [ops.window_filter(x, m, 3, 5) for m in METHODS]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for m, g in zip(METHODS, got):
        res, n = window_results(x.cpu().numpy(), 3, 5)
        _judge(g.cpu().numpy(), finish(res[m], n, x.cpu().numpy()), n, m, f"no synchronisation {m}")


# ---- through the API ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_clean_window_filter_after_compute_Sv_with_a_deferred_Sv(env, dtype):
    """compute_Sv leaves Sv deferred: window_filter is its first reader and writes it.  The result equals the ops-level
    call on the written Sv; the source dataset keeps its variable; attributes, dims and coordinates are as stated."""
    torch, ep = env
    from echopype_amd import echodata, ops, synth
    from echopype_amd.xr_lite import DeviceArray, LazyDeviceArray

    d = synth.ek60_numpy(2, 21, 150, seed=20261020)
    d["backscatter_r"][:, ::3, 120:] = np.nan
    ed = echodata.from_ek60_arrays(d).to_device()
    ds = ep.calibrate.compute_Sv(ed, dtype=dtype)
    lazy = ds["Sv"].data
    if dtype == "float64":  # (compute_Sv defers a float64 Sv; a float32 one is written at once)
        assert isinstance(lazy, LazyDeviceArray) and not lazy.materialized
    had_range = "actual_range" in ds["Sv"].attrs
    out = ep.clean.window_filter(ds, "median", 5, 3, min_valid=2)
    assert ds["Sv"].data is lazy and "window_filter" not in ds["Sv"].attrs
    assert not isinstance(lazy, LazyDeviceArray) or lazy.materialized
    assert ("actual_range" in ds["Sv"].attrs) == had_range
    sv = lazy.tensor
    want = ops.window_filter(sv, "median", 5, 3, min_valid=2)
    got = out["Sv"]
    assert isinstance(got.data, DeviceArray) and got.data.tensor.is_cuda and got.data.tensor.dtype == sv.dtype
    assert got.dims == ds["Sv"].dims == ("channel", "ping_time", "range_sample") and got.shape == ds["Sv"].shape
    assert torch.equal(torch.nan_to_num(got.data.tensor, nan=SENTINEL), torch.nan_to_num(want, nan=SENTINEL))
    sv_h = sv.cpu().numpy()
    assert sv_h.dtype == np.dtype(dtype) and np.isnan(sv_h).any() and np.isfinite(sv_h).any()
    res, n = window_results(sv_h, 5, 3)
    _judge(got.values, finish(res["median"], n, sv_h, 2, True), n, "median", "after compute_Sv")
    assert got.attrs["window_filter"] == "median 5x3" and "actual_range" not in got.attrs
    assert {k: v for k, v in got.attrs.items() if k != "window_filter"} == \
        {k: v for k, v in ds["Sv"].attrs.items() if k != "actual_range"}
    for c in ("channel", "ping_time", "range_sample"):
        np.testing.assert_array_equal(out[c].values, ds[c].values)
    assert set(out.data_vars) == set(ds.data_vars) and out.attrs == ds.attrs
    assert out["echo_range"].data is ds["echo_range"].data  # (a shallow copy: the other variables are shared)
    # a second filter on the result, another variable name, a plane without a channel
    ds2 = out.copy()
    ds2["Sv_plane"] = (("ping_time", "range_sample"), sv_h[0].copy(), {"actual_range": [0.0, 1.0], "units": "dB"})
    op = ep.clean.window_filter(ds2, "max", 1, 3, var_name="Sv_plane", keep_nan=False)
    assert op["Sv_plane"].attrs == {"units": "dB", "window_filter": "max 1x3"} and op["Sv"].data is out["Sv"].data
    np.testing.assert_array_equal(op["Sv_plane"].values, window_filter_ref(sv_h[0], "max", 1, 3, keep_nan=False))
    assert ds2["Sv_plane"].attrs["actual_range"] == [0.0, 1.0]


def _school_scene(dtype):
    """Background at -80 +- 1.5 dB, one school of 16 pings x 30 samples at -55 +- 1 dB, and twelve single-sample spikes
    of -40 dB, none next to another or to the school; nothing within 5 dB of the threshold of -65 dB."""
    rng = np.random.default_rng(5)
    P, S = 48, 90
    sv = np.clip(rng.normal(-80.0, 1.5, (P, S)), -86.0, -74.0)
    sv[20:36, 30:60] = np.clip(rng.normal(-55.0, 1.0, (16, 30)), -58.0, -52.0)
    spikes = [(3, 5), (3, 40), (7, 80), (10, 20), (14, 62), (25, 10), (25, 75), (33, 84), (40, 8), (41, 45), (44, 70), (46, 30)]
    for p, s in spikes:
        sv[p, s] = -40.0
    return sv.astype(dtype), spikes


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_median_in_front_of_detect_shoal_leaves_exactly_the_school(env, dtype):
    torch, ep = env
    from scipy import ndimage

    import shoal_ref
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    sv, spikes = _school_scene(dtype)
    P, S = sv.shape
    ds = Dataset(coords={"channel": np.array(["ch0"]), "range_sample": np.arange(S),
                         "ping_time": np.datetime64("2026-01-01", "ns") + np.arange(P) * np.timedelta64(1, "s")})
    ds["Sv"] = DataArray(DeviceArray(torch.as_tensor(sv[None]).cuda()), ("channel", "ping_time", "range_sample"))
    params = {"var_name": "Sv", "channel": "ch0", "thr": -65.0, "maxvgap": 0, "maxhgap": 0}
    # the oracle on the CPU, before and after
    want_raw = shoal_ref.weill(sv, thr=-65.0, maxvgap=0, maxhgap=0)
    filtered = window_filter_ref(sv, "median", 3, 3)
    assert not (np.abs(filtered + 65.0) < 5.0).any() and not (np.abs(sv + 65.0) < 5.0).any()
    want_med = shoal_ref.weill(filtered, thr=-65.0, maxvgap=0, maxhgap=0)
    assert ndimage.label(want_raw)[1] == 1 + len(spikes) and ndimage.label(want_med)[1] == 1
    school = np.zeros((P, S), bool)
    school[20:36, 30:60] = True
    corners = np.zeros((P, S), bool)
    corners[[20, 20, 35, 35], [30, 59, 30, 59]] = True  # four school samples of nine: the median there is background
    np.testing.assert_array_equal(want_med, school & ~corners)
    # the device, before and after
    raw = ep.mask.detect_shoal(ds, "weill", params).data.tensor.cpu().numpy()
    np.testing.assert_array_equal(raw, want_raw)
    assert ndimage.label(raw)[1] == 13
    ds_med = ep.clean.window_filter(ds, "median", 3, 3)
    n = window_results(sv, 3, 3)[1]  # (nine away from the edges: a median there is an input; six and four along them)
    _judge(ds_med["Sv"].values[0], filtered, n, "median", "the school scene")
    np.testing.assert_array_equal(ds_med["Sv"].values[0, 1:-1, 1:-1], filtered[1:-1, 1:-1])
    med = ep.mask.detect_shoal(ds_med, "weill", params).data.tensor.cpu().numpy()
    np.testing.assert_array_equal(med, want_med)
    assert ndimage.label(med)[1] == 1
