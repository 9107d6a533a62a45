"""commongrid.regrid_Sv on the GPU (csrc/regrid.hip through ops.regrid_rows and commongrid.api.regrid_Sv) against its
NumPy restatement (tests/regrid_ref.py).

The judge: the NaN pattern and the infinities are the oracle's; a finite float64 value is within 1e-9 (the project's
fp64 tolerance on Sv), a finite float32 value within one float32 ulp of the oracle's value -- kernel and oracle both work
in float64 and round once, so their float32 results are the same number or neighbours.  ``coverage`` is held to the same
rule and never exceeds 1 + 1e-12.  The outputs are pre-filled with a value no result can take, so an element the kernel
left out shows."""
import numpy as np
import pytest

from regrid_cases import D0, grid, plant, volume
from regrid_ref import cell_bounds, conserved_sides, regrid_ref

pytestmark = pytest.mark.gpu

SENTINEL = 777.0  # (Sv is at most -30 dB or infinite, coverage at most 1)
PAIRS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)]
PAIR_IDS = ["f32", "f64", "f32_range_f64", "f64_range_f32"]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd as ep

    return torch, ep


def _judge(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    inf = np.isinf(got) | np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf], err_msg=what)
    f = np.isfinite(want)
    err = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64))
    tol = 1e-9 if want.dtype == np.float64 else np.spacing(np.abs(want[f])).astype(np.float64)
    if err.size:
        print(f"{what}: largest error {err.max():.3e}, {int((err > 0).sum())} of {err.size} differ")
    assert (err <= tol).all(), what


def _device_range(torch, r):
    t = torch.as_tensor(r).cuda()
    return t[:, None, :] if r.ndim == 2 else t  # (C, S): channel first, as in a dataset


def _run(torch, sv, r, range_bin, J, with_coverage=True, max_grid=0):
    """ops.regrid_rows into pre-filled outputs -> (Sv, coverage or None, count) on the host."""
    from echopype_amd import _lib, ops

    C, P, S = sv.shape
    tdt = torch.as_tensor(sv[:0]).dtype
    both = torch.full((2, C, P, J), SENTINEL, dtype=tdt, device="cuda")
    out = (both[0], both[1] if with_coverage else None)
    with _lib.launch_trace() as tr:
        got = ops.regrid_rows(torch.as_tensor(sv).cuda(), _device_range(torch, r), range_bin, J,
                              with_coverage=with_coverage, out=out, _max_grid=max_grid)
    assert tr.kernels == (["regrid_rows_kernel"] if C * P else [])
    assert got[0] is out[0] and got[1] is out[1]
    assert got[2].dtype == torch.int32 and tuple(got[2].shape) == (1,) and got[2].is_cuda
    host = both.cpu().numpy()
    assert not (host[0] == SENTINEL).any(), "an element of Sv was not written"
    if with_coverage:
        assert not (host[1] == SENTINEL).any(), "an element of coverage was not written"
        assert not (host[1] > 1 + 1e-12).any() and not (host[1] < 0).any()
    else:
        assert (host[1] == SENTINEL).all(), "the buffer behind Sv was written to"
    return host[0], host[1] if with_coverage else None, int(got[2].item())


def _against_the_oracle(torch, sv, r, e, what, **kw):
    J = len(e) - 1
    range_bin = float(e[1] - e[0]) if J else 1.0
    got_sv, got_cov, got_bad = _run(torch, sv, r, range_bin, J, **kw)
    want_sv, want_cov, want_bad = regrid_ref(sv, r, e)
    _judge(got_sv, want_sv, what + " Sv")
    if got_cov is not None:
        _judge(got_cov, want_cov, what + " coverage")
    assert got_bad == want_bad, what
    return want_sv, want_cov, want_bad


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 257])
def test_row_lengths(env, S, pair):
    """Three channels of spacings 1 : 4 : irregular, their ranges as (C, S); an odd number of cells, so that output rows
    start unaligned; more rows than workgroups."""
    torch, _ = env
    C, P = 3, 3
    sv, r = volume(11, C, P, S, pair[0], pair[1])
    e = grid(float(r.max()), 0.1, odd=True)
    assert (len(e) - 1) % 2 == 1
    want_sv, _, bad = _against_the_oracle(torch, sv, r, e, f"S={S}", max_grid=2)
    assert bad == (C * P if S == 1 else 0)
    assert S == 1 or np.isfinite(want_sv).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("tiles", ["T-1", "T", "T+1", "2T+3"])
def test_tile_seams(env, tiles, dtype):
    """Rows of one tile less a sample, one tile, one tile and a sample, two tiles and three, on three grids: cells of 3.7
    samples that straddle the seams, seven cells per sample (cut by the last edge in the coarser channels), and one cell
    for the whole row, which is handed from tile to tile."""
    torch, _ = env
    from echopype_amd import _lib

    T = _lib.REGRID_TILE
    S = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[tiles]
    sv, r = volume(13, 3, 2, S, dtype, dtype)
    reach = float(r[0].max())
    for name, e in (("straddle", grid(float(r.max()), 3.7 * D0, odd=True)), ("seven", grid(reach, D0 / 7, odd=True)),
                    ("one", grid(1.0, 1e6))):
        if name == "straddle" and S > T:  # the bound between the tiles lies inside a cell, in every channel
            for c in range(3):
                m = cell_bounds(r[c])[1]
                assert (m[T] / (3.7 * D0)) % 1.0 not in (0.0,) and m[T] < e[-1]
        if name == "one":
            assert len(e) == 2
        _against_the_oracle(torch, sv, r, e, f"{tiles} {name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("S", [70, "T+40"])
def test_planted_rows(env, S, dtype):
    """A cube range with a NaN tail of another length in every ping, three repeated leading zeros, +-inf samples, and
    three rows to refuse (one decreases once, one has a single finite range, one none): the counter says three.  Without
    ``with_coverage`` the buffer behind Sv keeps its bytes."""
    torch, _ = env
    from echopype_amd import _lib

    S = _lib.REGRID_TILE + 40 if S == "T+40" else S
    sv, r = volume(17, 3, 4, S, dtype, dtype, form="CPS")
    planted = plant(sv, r)
    e = grid(float(np.nanmax(r)), 0.1, odd=True)
    want_sv, want_cov, bad = _against_the_oracle(torch, sv, r, e, f"planted S={S}")
    assert bad == planted == 3
    assert np.isposinf(want_sv).any() and np.isneginf(want_sv).any() and np.isnan(want_sv[2, :2]).all()
    assert len({int(np.isfinite(r[0, p]).sum()) for p in range(4)}) == 4
    got_sv, got_cov, bad = _run(torch, sv, r, 0.1, len(e) - 1, with_coverage=False)
    assert got_cov is None and bad == 3
    _judge(got_sv, want_sv, "without coverage")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forms_of_the_range(env, dtype):
    """(S,), (C, S) and (C, P, S) ranges are read through their strides: the result is the one on the explicit cube."""
    torch, _ = env
    C, P, S = 3, 5, 65
    for form in ("S", "CS", "CPS"):
        sv, r = volume(19, C, P, S, dtype, dtype, form=form)
        assert r.ndim == {"S": 1, "CS": 2, "CPS": 3}[form]
        e = grid(float(r.max()), 0.2, odd=True)
        _against_the_oracle(torch, sv, r, e, f"range over {form}")
        cube = np.broadcast_to(r[:, None, :] if r.ndim == 2 else r, sv.shape).copy()
        a = _run(torch, sv, r, 0.2, len(e) - 1)
        b = _run(torch, sv, cube, 0.2, len(e) - 1)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_nothing_to_do(env):
    torch, _ = env
    from echopype_amd import ops

    sv, r = volume(23, 2, 3, 9, np.float32, np.float32)
    sv_t, r_t = torch.as_tensor(sv).cuda(), _device_range(torch, r)
    out, cov, bad = ops.regrid_rows(sv_t, r_t, 0.2, 0)  # no cell: the rows are still judged
    assert tuple(out.shape) == (2, 3, 0) and tuple(cov.shape) == (2, 3, 0) and int(bad.item()) == 0
    out, cov, bad = ops.regrid_rows(sv_t[:, :0], r_t, 0.2, 4, with_coverage=False)  # no row
    assert tuple(out.shape) == (2, 0, 4) and cov is None and int(bad.item()) == 0
    with pytest.raises(ValueError, match="out must hold contiguous"):
        ops.regrid_rows(sv_t, r_t, 0.2, 4, out=(torch.empty((2, 3, 4), device="cuda"), None))
    with pytest.raises(ValueError, match="does not broadcast"):
        ops.regrid_rows(sv_t, r_t[:, :, :5], 0.2, 4)


# ---- the public function -------------------------------------------------------------------------------------------------------
DIMS = ("channel", "ping_time", "range_sample")


def _dataset(torch, sv, r, range_var="echo_range", sv_on_device=True, range_on_device=True):
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    C, P, S = sv.shape
    ds = Dataset(coords={"channel": np.array([f"ch{i}" for i in range(C)]), "range_sample": np.arange(S),
                         "ping_time": np.datetime64("2026-01-01", "ns") + np.arange(P) * np.timedelta64(1, "s")})
    ds["Sv"] = DataArray(DeviceArray(torch.as_tensor(sv).cuda()) if sv_on_device else sv, DIMS)
    rdims = {1: DIMS[2:], 2: (DIMS[0], DIMS[2]), 3: DIMS}[r.ndim]
    ds[range_var] = DataArray(DeviceArray(torch.as_tensor(r).cuda()) if range_on_device else r, rdims)
    ds["frequency_nominal"] = (("channel",), np.array([38000.0, 200000.0, 120000.0, 70000.0][:C]))
    ds["latitude"] = (("ping_time",), np.linspace(45.0, 45.1, P))
    ds["angle_alongship"] = (DIMS, np.zeros(sv.shape, dtype=np.float32))  # carries range_sample: not carried over
    return ds


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_regrid_Sv_dataset(env, dtype):
    """Sv on the device with a device range, then on the host with a host ``depth``: variables, dimensions, coordinates,
    what is carried over and what is not, attributes; ``range_var_max``; ``with_coverage=False``; an empty range axis."""
    torch, ep = env
    from echopype_amd.commongrid.deferred import range_edges

    sv, r = volume(29, 3, 4, 130, dtype, np.float64)
    for on_device, range_var in ((True, "echo_range"), (False, "depth")):
        ds = _dataset(torch, sv, r, range_var, sv_on_device=on_device, range_on_device=on_device)
        out = ep.commongrid.regrid_Sv(ds, range_var=range_var, range_bin="0.2m")
        e = range_edges(float(r.max()), 0.2)  # the grid of compute_MVBS for the same range_bin
        want_sv, want_cov, _ = regrid_ref(sv, r, e)
        dims = ("channel", "ping_time", range_var)
        assert out["Sv"].dims == dims and out["coverage"].dims == dims and out["Sv"].shape == want_sv.shape
        assert out["Sv"].data.tensor.is_cuda and out["coverage"].data.tensor.is_cuda
        _judge(out["Sv"].values, want_sv, "regrid_Sv Sv")
        _judge(out["coverage"].values, want_cov, "regrid_Sv coverage")
        n_bad = out["n_rows_unordered"].data.tensor
        assert n_bad.is_cuda and n_bad.dtype == torch.int32 and n_bad.dim() == 0 and int(n_bad.item()) == 0
        np.testing.assert_array_equal(out[range_var].values, e[:-1])
        assert out[range_var].values.dtype == np.float64
        for d in ("channel", "ping_time"):
            np.testing.assert_array_equal(out[d].values, ds[d].values)
        np.testing.assert_array_equal(out["frequency_nominal"].values, ds["frequency_nominal"].values)
        np.testing.assert_array_equal(out["latitude"].values, ds["latitude"].values)
        assert "angle_alongship" not in out and "range_sample" not in out.coords
        assert out.attrs["processing_function"] == "commongrid.regrid_Sv" and out.attrs["range_var"] == range_var
        assert out.attrs["range_bin"] == "0.2m" and "midpoints" in out.attrs["regrid_cell_definition"]
        assert out["Sv"].attrs["units"] == "dB" and out["Sv"].attrs["range_meter_interval"] == "0.2m"
    # range_var_max cuts the grid as in compute_MVBS; without coverage there is no such variable
    out = ep.commongrid.regrid_Sv(ds, range_var="depth", range_bin="0.2m", range_var_max="3m", with_coverage=False)
    e = range_edges(3.0 + 1e-8, 0.2)
    assert "coverage" not in out and out["Sv"].shape[2] == len(e) - 1 == 16
    _judge(out["Sv"].values, regrid_ref(sv, r, e)[0], "range_var_max")
    # the only valid range is 0: an empty range axis, as for MVBS
    ds0 = _dataset(torch, sv, np.zeros_like(r))
    out = ep.commongrid.regrid_Sv(ds0)
    assert out["Sv"].shape == (3, 4, 0) and out["echo_range"].values.size == 0
    assert int(out["n_rows_unordered"].data.tensor.item()) == 0  # (equal ranges are in order)
    with pytest.raises(ValueError, match="range bins are empty"):
        ep.commongrid.regrid_Sv(_dataset(torch, sv, np.full_like(r, np.nan)))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_after_compute_Sv_with_a_deferred_Sv_and_a_lazy_range(env, dtype):
    """compute_Sv leaves Sv deferred and echo_range lazy: both are written through their accessors, and add_depth's
    ``depth`` serves as the range as well.  The rows carry NaN tails (padded pings)."""
    torch, ep = env
    from echopype_amd import echodata, synth
    from echopype_amd.commongrid.deferred import range_edges

    d = synth.ek60_numpy(2, 9, 300, seed=20261020)
    d["backscatter_r"][:, ::3, 260:] = np.nan
    ed = echodata.from_ek60_arrays(d).to_device()
    ds = ep.consolidate.add_depth(ep.calibrate.compute_Sv(ed, dtype=dtype), depth_offset=1.7)
    for range_var in ("echo_range", "depth"):
        out = ep.commongrid.regrid_Sv(ds, range_var=range_var, range_bin="1m")
        sv_h, r_h = ds["Sv"].values, ds[range_var].values
        assert sv_h.dtype == np.dtype(dtype) and np.isnan(r_h).any()
        e = range_edges(float(np.nanmax(r_h)), 1.0)
        want_sv, want_cov, bad = regrid_ref(sv_h, r_h, e)
        assert len(e) > 10 and np.isfinite(want_sv).any()
        _judge(out["Sv"].values, want_sv, f"after compute_Sv on {range_var}")
        _judge(out["coverage"].values, want_cov, f"after compute_Sv on {range_var} coverage")
        assert int(out["n_rows_unordered"].data.tensor.item()) == bad


def _two_channel_layer(dtype):
    """Two channels that see the same layer between 5 m and 7 m -- 10 dB stronger at 200 kHz -- over a background that is
    the same in both, sampled every 0.047 m and every 0.188 m; the coarser row is padded with NaN behind its 64 samples."""
    S = 256
    r = np.full((2, S), np.nan)
    r[0] = (np.arange(S) + 0.5) * 0.047
    r[1, :64] = (np.arange(64) + 0.5) * 0.188
    sv = np.full((2, 5, S), -70.0)
    with np.errstate(invalid="ignore"):
        layer = (r >= 5.0) & (r < 7.0)
    sv[0][:, layer[0]] = -60.0
    sv[1][:, layer[1]] = -50.0
    sv[1][:, 64:] = np.nan
    return sv.astype(dtype), r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_regrid_then_frequency_differencing(env, dtype):
    torch, ep = env
    sv, r = _two_channel_layer(dtype)
    ds = _dataset(torch, sv, r)
    rg = ep.commongrid.regrid_Sv(ds, range_bin="0.188m")
    mask = ep.mask.frequency_differencing(rg, freqABEq="200kHz - 38kHz >= 5dB")
    assert mask.dims == ("ping_time", "echo_range") and mask.data.tensor.is_cuda
    e = np.concatenate([rg["echo_range"].values, [rg["echo_range"].values[-1] + 0.188]])
    want_sv = regrid_ref(sv, r, np.arange(len(e)) * 0.188)[0]
    with np.errstate(invalid="ignore"):
        diff = want_sv[1] - want_sv[0]
        assert not (np.abs(diff - 5.0) < 1e-3).any()  # (no cell near the threshold: the mask does not hang on an ulp)
        want = diff >= 5.0
    got = mask.data.tensor.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    lo, hi = e[:-1], e[1:]
    assert got[:, (lo >= 5.2) & (hi <= 6.8)].all() and not got[:, hi <= 4.8].any() and not got[:, lo >= 7.2].any()
    assert got.any(axis=1).all() and 8 <= got[0].sum() <= 12
    # by sample index the two channels do not meet: the layer of the coarse channel lies at samples 27 .. 37
    by_index = ep.mask.frequency_differencing(ds, freqABEq="200kHz - 38kHz >= 5dB").data.tensor.cpu().numpy()
    assert by_index[0, 27:37].all() and not by_index[0, 107:148].any()
    # ... and the result goes into apply_mask as it is
    masked = ep.mask.apply_mask(rg, mask)
    kept = ~np.isnan(masked["Sv"].values)
    np.testing.assert_array_equal(kept, np.broadcast_to(want, kept.shape) & ~np.isnan(rg["Sv"].values))
    # detect_shoal works along a dimension called range_sample: the regridded array goes in under that name
    from echopype_amd.xr_lite import DataArray, Dataset

    by_cell = Dataset(coords={"channel": rg["channel"], "ping_time": rg["ping_time"], "range_sample": np.arange(len(lo))})
    by_cell["Sv"] = DataArray(rg["Sv"].data, ("channel", "ping_time", "range_sample"))
    shoal = ep.mask.detect_shoal(by_cell, "weill", {"var_name": "Sv", "channel": "ch1", "thr": -60.0, "maxvgap": 0})
    with np.errstate(invalid="ignore"):
        assert not (np.abs(want_sv[1] + 60.0) < 1e-3).any()
        np.testing.assert_array_equal(shoal.data.tensor.cpu().numpy(), want_sv[1] > -60.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_echo_integral_is_conserved_on_the_device_outputs(env, dtype):
    """sum_j 10^(Sv_j/10) coverage_j bin, evaluated with torch in float64 on the device outputs, against the integral
    of the samples over the grid (NumPy, float64).  float64 outputs: 1e-12 relative, the bound of the host test (an
    error of a few ulp of 90 dB in Sv_j is 1e-14 relative in 10^(Sv_j/10)).  float32 outputs: Sv_j is off by at most half
    a float32 ulp of a value below 128 dB, 2^-18 dB, which is 0.2303 * 2^-18 = 8.8e-7 relative in its linear value,
    coverage_j by 2^-24 = 6e-8 relative; every term is positive, so the sum is within 9.4e-7 < 1e-6."""
    torch, ep = env
    sv, r = volume(31, 3, 4, 257, dtype, dtype, form="CPS")
    ds = _dataset(torch, sv, r)
    out = ep.commongrid.regrid_Sv(ds, range_bin="0.2m", range_var_max="10m")
    got, cov = out["Sv"].data.tensor.double(), out["coverage"].data.tensor.double()
    lin = torch.where(cov > 0, torch.pow(10.0, got / 10.0), torch.zeros_like(got))
    lhs = (lin * cov * 0.2).sum(dim=2).cpu().numpy()
    e = np.arange(out["echo_range"].values.size + 1) * 0.2
    _, rhs = conserved_sides(sv, r, e)
    rel = np.abs(lhs - rhs) / rhs
    print("largest relative difference", rel.max())
    assert np.isfinite(rhs).all() and (rel <= (1e-12 if dtype == np.float64 else 1e-6)).all()


def test_no_host_synchronisation_with_range_var_max(env):
    """torch's synchronisation debug mode raises on any blocking call: with the dataset in HBM and ``range_var_max`` given,
    regrid_Sv makes none (the way test_gpu_line_mask.py checks line_mask)."""
    torch, ep = env
    sv, r = volume(37, 3, 4, 257, np.float32, np.float32, form="CPS")
    ds = _dataset(torch, sv, r)
    call = lambda: ep.commongrid.regrid_Sv(ds, range_bin="0.2m", range_var_max="10m")  # noqa: E731
    call()  # warm-up: the allocator's blocks
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    e = np.arange(out["echo_range"].values.size + 1) * 0.2
    _judge(out["Sv"].values, regrid_ref(sv, r, e)[0], "no synchronisation")
