"""mask.regrid_mask on the GPU (csrc/mask_grid.hip through ops.regrid_mask and the public function) against
tests/regrid_mask_ref.py, which tests/test_regrid_mask_host.py holds against pandas.  Results are 0 / 1: equality, no
tolerance."""
import numpy as np
import pytest

import regrid_mask_ref as R

pytestmark = pytest.mark.gpu

T0 = np.datetime64("2021-03-04T10:00:00", "ns").astype(np.int64)
S = 10**9


def _arrays(mask, ping_ns, rng, third=None, third_dim="beam", device=False, range_name="depth", mask_dims=None):
    import torch

    from echopype_amd.xr_lite import DataArray, DeviceArray

    mask, rng = np.asarray(mask), np.asarray(rng, dtype=np.float64)
    dims = (("ping_time", "depth") if mask.ndim == 2 else (third_dim, "ping_time", "depth"))
    coords = {"ping_time": np.asarray(ping_ns, dtype=np.int64).view("datetime64[ns]"), "depth": np.arange(mask.shape[-1])}
    if mask.ndim == 3 and third is not None:
        coords[third_dim] = np.asarray(third)
    if mask_dims is not None:  # another order of the same dimensions
        mask = np.ascontiguousarray(mask.transpose([dims.index(d) for d in mask_dims]))
        dims = mask_dims
    up = (lambda a: DeviceArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())) if device else (lambda a: a)
    m = DataArray(up(mask), dims, coords=coords, name="shoal_mask")
    r = DataArray(up(rng), ("depth",) if rng.ndim == 1 else ("ping_time", "depth"), name=range_name)
    return m, r


def _check(mask, ping_ns, rng, range_bin, bin_s, func="logical-AND", closed="left", third=None, device=False,
           range_var_max=None, range_name="depth", judge=R.regrid, mask_dims=None, kernels=None):
    """Run the public function and the judge on the same input; everything the result carries is compared."""
    import torch

    import echopype_amd as ep
    from echopype_amd import _lib

    mask = np.asarray(mask)
    m, r = _arrays(mask, ping_ns, rng, third, device=device, range_name=range_name, mask_dims=mask_dims)
    kw = {} if range_var_max is None else {"range_var_max": f"{range_var_max}m"}
    with _lib.launch_trace() as tr:
        out = ep.mask.regrid_mask(m, r, range_bin=f"{range_bin}m", ping_time_bin=f"{bin_s}s", func=func, closed=closed,
                                  third_dim="beam" if mask.ndim == 3 else None, **kw)
    if kernels is not None:
        assert [k for k in tr.kernels if k.startswith("regrid_")] == ["regrid_clear_kernel", kernels,
                                                                      "regrid_final_kernel"], tr.kernels
    uniq, tedges, redges, want = judge(mask if mask.ndim == 3 else mask[None], ping_ns, rng, float(range_bin), bin_s * S,
                                       func, closed, third=third, range_var_max=range_var_max)
    got = out.data.tensor
    assert got.is_cuda and got.dtype == getattr(torch, mask.dtype.name)
    want = want if mask.ndim == 3 else want[0]
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), (func, closed, np.argwhere(got.cpu().numpy() != want)[:5])
    assert out.name == "shoal_mask"
    assert out.dims == (("beam",) if mask.ndim == 3 else ()) + ("ping_time", range_name)
    assert out.coords["ping_time"].dtype == np.dtype("datetime64[ns]")
    np.testing.assert_array_equal(out.coords["ping_time"].view(np.int64), tedges[:-1])
    assert out.coords[range_name].dtype == np.float64
    np.testing.assert_array_equal(out.coords[range_name], redges[:-1])
    if mask.ndim == 3:
        np.testing.assert_array_equal(out.coords["beam"], uniq)
    assert out[range_name].attrs == {"long_name": "Range distance", "units": "m"}
    return out, want


# ---- the situations of the reference's own tests ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [bool, np.int64])
@pytest.mark.parametrize("func", ["logical-AND", "logical-OR"])
def test_four_by_four_inside_the_cells(dtype, func):
    """Pings at :01, :19, :21, :39 and depths 1, 19, 21, 39 with 20 s / 20 m bins: 2 x 2 cells of 2 x 2 samples."""
    ping_ns = T0 + S * np.array([1, 19, 21, 39])
    depth = [1.0, 19.0, 21.0, 39.0]
    for rows in ([[1, 1, 1, 1]] * 4,
                 [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]],
                 [[1, 0, 1, 1], [1, 1, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]],
                 [[0, 0, 0, 0]] * 4):
        mask = np.array(rows).astype(dtype)
        for device in (False, True):
            out, want = _check(mask, ping_ns, depth, 20, 20, func, device=device, kernels="regrid_sweep_kernel_lds")
            cells = mask.astype(int).reshape(2, 2, 2, 2).transpose(0, 2, 1, 3).reshape(2, 2, 4)
            np.testing.assert_array_equal(want.astype(int), cells.min(-1) if func == "logical-AND" else cells.max(-1))
    assert out.attrs == {
        "cell_methods": "ping_time: mean (interval: 20 second comment: ping_time is the interval start) "
                        "depth: mean (interval: 20.0 meter comment: depth is the interval start)",
        "binning_mode": "physical units", "range_meter_interval": "20.0m", "ping_time_interval": "20s"}


@pytest.mark.parametrize("dtype", [bool, np.int64])
@pytest.mark.parametrize("func", ["logical-AND", "logical-OR"])
@pytest.mark.parametrize("closed", ["left", "right"])
def test_five_by_five_on_the_edges(dtype, func, closed):
    """Pings and depths on the edges 0, 10, .., 40 of 10 s / 10 m bins: the closed side decides every membership."""
    ping_ns = T0 + S * np.array([0, 10, 20, 30, 40])
    depth = [0.0, 10.0, 20.0, 30.0, 40.0]
    rng = np.random.default_rng(3)
    for k in range(3):
        mask = (rng.random((5, 5)) < 0.6).astype(dtype)
        out, want = _check(mask, ping_ns, depth, 10, 10, func, closed)
        # one sample per cell: the mask itself, shifted by one for the right-closed intervals (the first row and
        # column then fall before the first edge)
        assert want.shape == (5, 5)
        if closed == "left":
            np.testing.assert_array_equal(want, mask)
        else:
            np.testing.assert_array_equal(want[:4, :4], mask[1:, 1:])
            assert not want[4].any() and not want[:, 4].any()


# ---- shapes ---------------------------------------------------------------------------------------------------------------
def _pings_with_a_gap(P, bin_s):
    """P pings, one per second, over several bins, with one bin left empty in the middle."""
    t = np.arange(P, dtype=np.int64)
    t[P // 2:] += 2 * bin_s - (t[P // 2] % bin_s)  # the second half starts on an edge, two bins on
    return T0 + 3 * S + S * t


@pytest.mark.parametrize("D", [1, 15, 16, 17, 200])
@pytest.mark.parametrize("func", ["logical-AND", "logical-OR"])
def test_widths_around_the_sixteen_byte_load(D, func):
    P, bin_s = 45, 10
    ping_ns = _pings_with_a_gap(P, bin_s)
    depth = 0.25 + 0.5 * np.arange(D)
    rng = np.random.default_rng(D)
    fill = 1 if func == "logical-AND" else 0
    mask = np.full((P, D), fill, dtype=np.uint8)
    tedges = R.time_edges(ping_ns, bin_s * S)
    ti = R.member(ping_ns, tedges, "left")
    assert len(np.unique(ti)) < len(tedges) - 1  # an empty time bin
    # a cell that is uniform except for its last ping and last column
    last_ping = np.flatnonzero(ti == ti[0])[-1]
    cols = np.flatnonzero(R.member(depth, R.range_edges(depth, 2.0), "left") == 0)
    mask[last_ping, cols[-1]] = 1 - fill
    # and a few more exceptions anywhere
    mask[rng.integers(0, P, 3), rng.integers(0, D, 3)] = 1 - fill
    for device in (False, True):
        out, want = _check(mask, ping_ns, depth, 2, bin_s, func, device=device, kernels="regrid_sweep_kernel_lds")
    assert want[0, 0] == 1 - fill and (want == fill).any()
    empty = np.setdiff1d(np.arange(len(tedges) - 1), ti)
    assert not want[empty].any()


def test_range_var_max_below_the_deepest_sample():
    P, D = 12, 40
    ping_ns = T0 + S * np.arange(P)
    depth = np.arange(D) * 1.0
    mask = np.ones((P, D), dtype=bool)
    mask[:, 25:] = False  # beyond the last edge: dropped, so the last cell stays all True
    out, want = _check(mask, ping_ns, depth, 5, 20, range_var_max=22, kernels="regrid_sweep_kernel_lds")
    assert want.shape == (1, 5) and want.all()  # edges 0, 5, .., 25
    out, want = _check(mask, ping_ns, depth, 5, 20)
    assert want.shape == (1, 8) and want[0].tolist() == [True] * 5 + [False] * 3


@pytest.mark.parametrize("closed", ["left", "right"])
@pytest.mark.parametrize("D", [16, 37])
def test_two_dimensional_range_with_nans(D, closed):
    P, bin_s = 50, 20
    rng = np.random.default_rng(11 + D)
    ping_ns = _pings_with_a_gap(P, bin_s)
    depth = 0.5 * np.arange(D)[None, :] + rng.choice([0.0, 0.5, 3.0], size=(P, 1))
    depth[rng.random((P, D)) < 0.15] = np.nan
    mask = (rng.random((P, D)) < 0.85).astype(np.uint8)
    wants = {}
    for func in ("logical-AND", "logical-OR"):
        for device in (False, True):
            out, wants[func] = _check(mask, ping_ns, depth, 2.5, bin_s, func, closed, device=device,
                                      kernels="regrid_sweep_kernel_ping_lds")
    assert wants["logical-OR"].any() and not wants["logical-OR"].all()
    assert not np.array_equal(wants["logical-AND"], wants["logical-OR"])
    # a mask that is zero exactly where the range is known: the NaN samples must not reach any cell
    mask = np.isnan(depth).astype(np.uint8)
    out, want = _check(mask, ping_ns, depth, 2.5, bin_s, "logical-OR", closed)
    assert not want.any()


@pytest.mark.parametrize("func", ["logical-AND", "logical-OR"])
def test_third_dimension_merges_equal_coordinates(func):
    """The coordinate [7, 2, 7]: two output slices, 2 first; the two slices of 7 merge their samples."""
    P, D = 30, 20
    rng = np.random.default_rng(21)
    ping_ns = T0 + S * np.arange(P)
    depth = np.arange(D) * 1.0
    mask = (rng.random((3, P, D)) < 0.97).astype(np.int64)
    for device in (False, True):
        out, want = _check(mask, ping_ns, depth, 5, 10, func, third=[7, 2, 7], device=device)
    assert want.shape[0] == 2 and out.coords["beam"].tolist() == [2, 7]
    _, _, _, alone = R.regrid(mask[1:2], ping_ns, depth, 5.0, 10 * S, func)
    np.testing.assert_array_equal(want[0], alone[0])
    _, _, _, a = R.regrid(mask[0:1], ping_ns, depth, 5.0, 10 * S, func)
    _, _, _, b = R.regrid(mask[2:3], ping_ns, depth, 5.0, 10 * S, func)
    np.testing.assert_array_equal(want[1], (a[0] & b[0]) if func == "logical-AND" else (a[0] | b[0]))
    # an unsorted coordinate comes out sorted, no coordinate counts the slices, another order of the dimensions
    _check(mask, ping_ns, depth, 5, 10, func, third=[5, 9, 1])
    _check(mask, ping_ns, depth, 5, 10, func, third=None)
    _check(mask, ping_ns, depth, 5, 10, func, third=[7, 2, 7], mask_dims=("depth", "beam", "ping_time"), device=True)


def test_one_time_bin_with_very_many_pings():
    """5000 pings in one time bin: the bin is shared by several workgroups (a chunk of pings each), whose flags meet
    in the result."""
    P, D = 5000, 64
    ping_ns = T0 + (S // 100) * np.arange(P)  # 50 s in all, one bin of 60 s
    depth = 0.5 * np.arange(D)
    mask = np.ones((P, D), dtype=bool)
    mask[4999, 63] = False  # the last sample of the last chunk
    mask[2600, 17] = False
    out, want = _check(mask, ping_ns, depth, 4, 60, "logical-AND", device=True, kernels="regrid_sweep_kernel_lds")
    assert want.shape == (1, 8) and want[0].tolist() == [True, True, False, True, True, True, True, False]
    out, want = _check(~mask, ping_ns, depth, 4, 60, "logical-OR", device=True)
    assert want[0].tolist() == [False, False, True, False, False, False, False, True]


@pytest.mark.parametrize("two_d", [False, True])
def test_range_grid_too_large_for_lds(two_d):
    """range_bin = 0.001 m over 200 m: 200 000 range bins, whose flags go to the result directly."""
    from echopype_amd import ops

    P, D = (40, 4096) if not two_d else (12, 2048)
    rng = np.random.default_rng(31)
    ping_ns = _pings_with_a_gap(P, 10)
    depth = np.sort(rng.choice(np.arange(200000), size=D, replace=False)) * 0.001 + 0.0005
    depth[-1] = 199.9995
    if two_d:
        depth = depth[None, :] + rng.choice([0.0, 0.001], size=(P, 1))
    mask = (rng.random((P, D)) < 0.9).astype(np.uint8)
    n_rbins = len(R.range_edges(depth, 0.001)) - 1
    assert ops.regrid_needs_global_flags(n_rbins) and not ops.regrid_needs_global_flags(32768)
    for func in ("logical-AND", "logical-OR"):
        out, want = _check(mask, ping_ns, depth, 0.001, 10, func, device=True, judge=R.regrid_by_counts,
                           kernels="regrid_sweep_kernel_ping_global" if two_d else "regrid_sweep_kernel_global")
        assert want.any() and not want.all()


def test_range_grid_that_fills_most_of_lds():
    """20 000 range bins: 80 KB of flags, more than a workgroup gets without asking."""
    P, D = 24, 1000
    rng = np.random.default_rng(33)
    depth = np.sort(rng.choice(np.arange(20000), size=D, replace=False)) * 0.01 + 0.005
    depth[-1] = 199.995
    mask = (rng.random((P, D)) < 0.9).astype(np.uint8)
    for func in ("logical-AND", "logical-OR"):
        out, want = _check(mask, _pings_with_a_gap(P, 10), depth, 0.01, 10, func, device=True, judge=R.regrid_by_counts,
                           kernels="regrid_sweep_kernel_lds")
        assert want.shape[1] == 20000 and want.any() and not want.all()


@pytest.mark.parametrize("dtype", [np.uint8, np.float64, np.int32, bool])
def test_the_result_has_the_type_of_the_mask(dtype):
    P, D = 20, 33
    rng = np.random.default_rng(41)
    mask = (rng.random((P, D)) < 0.9).astype(dtype)
    for device in (False, True):
        _check(mask, T0 + S * np.arange(P), np.arange(D) * 0.7, 3, 5, device=device, range_name="echo_range")


def test_a_mask_holding_a_two_is_refused():
    import echopype_amd as ep

    P, D = 70, 50
    ping_ns = T0 + S * np.arange(P)
    for dtype, device in ((np.uint8, True), (np.int64, False), (np.uint8, False), (np.float32, True)):
        mask = np.ones((P, D), dtype=dtype)
        m, r = _arrays(mask, ping_ns, np.arange(D) * 1.0, device=device)
        ep.mask.regrid_mask(m, r, "5m", "20s")
        mask[P - 1, D - 1] = 2
        m, r = _arrays(mask, ping_ns, np.arange(D) * 1.0, device=device)
        with pytest.raises(ValueError) as ei:
            ep.mask.regrid_mask(m, r, "5m", "20s")
        assert str(ei.value) == "Mask must be binary True/False or 1/0."


def test_unsorted_ping_time_is_not_supported():
    import echopype_amd as ep

    ping_ns = T0 + S * np.array([0, 2, 1, 3])
    m, r = _arrays(np.ones((4, 3), dtype=bool), ping_ns, [0.0, 1.0, 2.0])
    with pytest.raises(NotImplementedError):
        ep.mask.regrid_mask(m, r)


def _random_case(seed):
    rng = np.random.default_rng(100 + seed)
    T = int(rng.integers(1, 4)) if seed % 2 else None
    P, D = int(rng.integers(1, 301)), int(rng.integers(1, 201))
    bin_s = int(rng.choice([5, 20, 60]))
    steps = rng.choice([0, S // 4, S, 2 * S, bin_s * S], size=P, p=[0.1, 0.3, 0.4, 0.15, 0.05])
    ping_ns = T0 + int(rng.integers(0, 30)) * S + np.cumsum(steps)
    range_bin = float(rng.choice([0.1, 0.5, 2.0, 10.0]))
    depth = np.sort(rng.choice(np.arange(0, 8 * D) * range_bin / 4, size=D, replace=False))  # many exactly on an edge
    if seed % 5 == 3:
        depth = depth[None, :] + rng.choice([0.0, range_bin / 4], size=(P, 1))
        depth = np.where(rng.random((P, D)) < 0.1, np.nan, depth)
        depth[0, 0] = 0.0
    shape = (P, D) if T is None else (T, P, D)
    dtype = [bool, np.uint8, np.int64, np.float32][seed % 4]
    mask = (rng.random(shape) < rng.choice([0.5, 0.98, 1.0])).astype(dtype)
    third = None if T is None else rng.integers(0, 3, size=T)
    return mask, ping_ns, depth, range_bin, bin_s, third


@pytest.mark.parametrize("seed", range(20))
def test_seeded_random_cases(seed):
    mask, ping_ns, depth, range_bin, bin_s, third = _random_case(seed)
    closed = "right" if seed % 3 == 0 else "left"
    # the loop over the cells where there are few of them, the counting form (held to the loop by the host tests) else
    cells = (len(R.time_edges(ping_ns, bin_s * S)) - 1) * (len(R.range_edges(depth, range_bin)) - 1)
    judge = R.regrid if cells <= 1500 else R.regrid_by_counts
    for func in ("logical-AND", "logical-OR"):
        _check(mask, ping_ns, depth, range_bin, bin_s, func, closed, third=third, device=bool(seed % 2), judge=judge)


def test_bad_arguments_are_refused():
    import torch

    from echopype_amd import ops

    mask = torch.ones((1, 4, 8), dtype=torch.uint8, device="cuda")
    rng = torch.arange(8, dtype=torch.float64, device="cuda")
    bs = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="range_bin must be positive"):
        ops.regrid_mask(mask, rng, bs, 1, 0.0, 4)
    with pytest.raises(ValueError, match="range must be float64"):
        ops.regrid_mask(mask, rng.float(), bs, 1, 2.0, 4)
    out, flag = ops.regrid_mask(mask, rng, bs, 1, 2.0, 4)
    assert out.cpu().numpy().tolist() == [[[1, 1, 1, 1]]] and int(flag.item()) == 0


def test_chain_from_differencing_to_the_masked_mvbs():
    """frequency_differencing -> regrid_mask -> apply_mask: a sample-resolution criterion applied to an MVBS-shaped
    dataset, everything on the device."""
    import torch

    import echopype_amd as ep
    import freq_diff_ref as F
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    P, D = 60, 48
    rng = np.random.default_rng(51)
    ping_ns = T0 + S * np.arange(P)
    depth = 0.5 * np.arange(D)
    sv = F.half_steps(rng, (2, P, D), np.float32, lo=-45, hi=-25)
    sv[0, 20:40, 8:24] = -30.0  # a patch where the difference is large everywhere
    sv[1, 20:40, 8:24] = -44.0
    ds = Dataset(coords={"channel": np.array(["chan1", "chan2"]), "ping_time": ping_ns.view("datetime64[ns]"),
                         "depth": depth})
    ds["Sv"] = DataArray(DeviceArray(torch.from_numpy(sv).cuda()), ("channel", "ping_time", "depth"), name="Sv")
    ds["frequency_nominal"] = (("channel",), np.array([38000.0, 120000.0]))
    mask = ep.mask.frequency_differencing(ds, freqABEq="38kHz - 120kHz >= 10dB")
    fine = F.freq_diff(sv, 0, 1, ">=", 10.0)
    assert np.array_equal(mask.data.tensor.cpu().numpy(), fine)
    coarse = ep.mask.regrid_mask(mask, DataArray(depth, ("depth",), name="depth"), range_bin="4m", ping_time_bin="10s")
    _, tedges, redges, want = R.regrid(fine[None], ping_ns, depth, 4.0, 10 * S)
    assert coarse.data.tensor.dtype == torch.bool and np.array_equal(coarse.data.tensor.cpu().numpy(), want[0])
    assert want[0].any() and not want[0].all() and coarse.name == "mask"
    nt, nr = want[0].shape
    mvbs = Dataset(coords={"channel": np.array(["chan1", "chan2"]), "ping_time": coarse.coords["ping_time"],
                           "depth": coarse.coords["depth"]})
    grid = rng.normal(-60, 5, (2, nt, nr))
    mvbs["Sv"] = DataArray(DeviceArray(torch.from_numpy(grid).cuda()), ("channel", "ping_time", "depth"), name="Sv")
    out = ep.mask.apply_mask(mvbs, coarse)
    np.testing.assert_array_equal(out["Sv"].values, np.where(want[0][None], grid, np.nan))


def test_foreign_arrays_in_foreign_array_out(monkeypatch):
    """DataArrays of an xarray-like library in (tests/fake_xarray.py stands in for it) -> one of that library out, the
    range coordinate with its attributes."""
    import fake_xarray as fx

    import echopype_amd as ep
    from echopype_amd import xr_lite

    monkeypatch.setattr(xr_lite, "_xr", fx)
    P, D = 30, 21
    rng = np.random.default_rng(61)
    ping_ns = T0 + S * np.arange(P)
    depth = 0.5 * np.arange(D)
    mask = rng.random((P, D)) < 0.95
    m = fx.DataArray(mask, ("ping_time", "depth"), {"ping_time": ping_ns.view("datetime64[ns]"), "depth": np.arange(D)},
                     name="m")
    out = ep.mask.regrid_mask(m, fx.DataArray(depth, ("depth",), name="depth"), range_bin="2m", ping_time_bin="10s")
    assert isinstance(out, fx.DataArray) and out.name == "m" and out.dims == ("ping_time", "depth")
    _, tedges, redges, want = R.regrid(mask[None], ping_ns, depth, 2.0, 10 * S)
    assert out.values.dtype == bool and np.array_equal(out.values, want[0])
    np.testing.assert_array_equal(out.coords["depth"].values, redges[:-1])
    assert out.coords["depth"].attrs == {"long_name": "Range distance", "units": "m"}
    assert out.attrs["range_meter_interval"] == "2.0m"
