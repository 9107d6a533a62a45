"""mask.label_regions / mask.region_statistics on the GPU (csrc/region_stats.hip through ops.region_stats /
ops.region_labels and mask/regions.py) against tests/region_ref.py, on planes chosen at the wave width (64 samples) and at
the limits of the labelling's table.

What is compared how
- ``region_label`` EQUAL to scipy's labels, and EQUAL: ``n_samples``, the bounding box, ``n_pings``,
  ``ping_time_start`` / ``ping_time_end``, ``n_valid``, ``Sv_max``, ``{range_var}_min`` / ``_max``: selection and
  counting only, and float32 -> float64 is exact.
- Every raw sum of ``ops.region_stats`` within ``(n + 8) * 2**-52 * sum|term|`` of the oracle's correctly rounded
  ``math.fsum``, n the number of terms.  Derivation, with u = 2**-53: a sum of n float64 terms taken in ANY order
  (registers along the pings, the shuffle tree over a run, the order in which the updates reach the table) is within
  (n - 1) u (1 + O(n u)) sum|term| of the exact sum, below n * 2**-53 * 1.01 for the n here; the terms themselves differ
  from the oracle's: ``lin_from_db`` is within 4e-16 < 1.81 * 2**-52 of 10**(Sv/10) (fast_math.h), the oracle's
  ``linear`` (quotient and power in np.longdouble, rounded once) within 2**-53 * 1.01, the products ``sv * r`` /
  ``sv * dz`` round once on each side (2 * 2**-53; a fused multiply-add rounds less), the oracle's final rounding is
  2**-53: together below (n/2 + 3.9) * 2**-52 sum|term|.  ``r`` and ``dz = r[s] - r[s-1]`` are the same float64 numbers
  on both sides.  (A float64 ``10 ** (Sv / 10)`` would not do as the oracle: rounding the quotient alone costs up to
  11 * 2**-53 at -95 dB.)  The bound is not to be loosened.
- The derived variables at the project's float64 standard, 1e-9 relative, ``Sv_mean`` at 1e-8 dB absolute.  The test
  depths are positive and increasing, so no sum cancels (sum|term| = |sum|) and the raw-sum bound implies these with
  room: 250 terms give 3e-14 relative.
- Between two calls, and between float32 and float64 storage of the same values, everything in the EQUAL list is
  identical; the sums may differ in their last bits (the order in which updates arrive) and are held to the bound."""
import numpy as np
import pytest

import region_ref as R

pytestmark = pytest.mark.gpu

EQUAL = ("n_samples", "ping_first", "ping_last", "sample_first", "sample_last", "n_pings", "ping_time_start",
         "ping_time_end")
EQUAL_C = ("n_valid", "Sv_max", "depth_min", "depth_max")
DERIVED = ("depth_mean", "center_of_mass", "height_mean", "NASC")
T0 = np.datetime64("2026-10-16T00:00:00", "ns")


def _ping_time(P):
    return T0 + np.arange(P) * np.timedelta64(1500, "ms")


def _dataset(sv, depth, depth_dims, on_device=True):
    import torch

    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    C, P, S = sv.shape
    ds = Dataset(coords={"channel": np.array([f"chan{i + 1}" for i in range(C)]), "ping_time": _ping_time(P),
                         "range_sample": np.arange(S)})
    for name, a, dims in (("Sv", sv, ("channel", "ping_time", "range_sample")), ("depth", depth, depth_dims)):
        data = DeviceArray(torch.as_tensor(np.ascontiguousarray(a)).cuda()) if on_device else a
        ds[name] = DataArray(data, dims, name=name)
    return ds


def _raw_sums(sv, depth, depth_dims, mask, connectivity):
    """The raw tables straight from ops.shoal_label + ops.region_stats, the regions in the order of their first pixel."""
    import torch

    from echopype_amd import ops

    C, P, S = sv.shape
    plane = torch.as_tensor(np.ascontiguousarray(mask)).cuda()
    state = ops.shoal_state(plane.device)
    code, _ = ops.shoal_label(plane, connectivity, state)
    n = int(state[1])
    r = torch.as_tensor(np.ascontiguousarray(depth)).cuda()
    r = r[tuple(slice(None) if d in depth_dims else None for d in ("channel", "ping_time", "range_sample"))]
    stats, ids = ops.region_stats(code, n, state, torch.as_tensor(np.ascontiguousarray(sv)).cuda(), r)
    assert int(state[0]) == 0
    assert tuple(stats.shape) == (C, n, 11) and tuple(ids.shape) == (n, 2)
    tabs = ops.region_tables(stats.cpu().numpy(), ids.cpu().numpy(), P * S)
    order = np.argsort(tabs["first"], kind="stable")
    return {k: v[..., order] for k, v in tabs.items()}


def _expand(depth, depth_dims):
    full = ("channel", "ping_time", "range_sample")
    return np.asarray(depth, dtype=np.float64)[tuple(slice(None) if d in depth_dims else None for d in full)]


def _check(sv, depth, depth_dims, mask, connectivity, n_regions=None, on_device=True):
    """region_statistics against the oracle; returns (result, oracle)."""
    import torch

    import echopype_amd as ep
    from echopype_amd.mask import regions

    C, P, S = sv.shape
    want = R.statistics(sv, _expand(depth, depth_dims), mask, connectivity, ping_time=_ping_time(P))
    n = want["n_regions"]
    if n_regions is not None:
        assert n == n_regions
    ds = _dataset(sv, depth, depth_dims, on_device)
    reads = []
    real = regions._to_host
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(regions, "_to_host", lambda t: (reads.append(t.numel()), real(t))[1])
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
        out = ep.mask.region_statistics(ds, mask, connectivity=connectivity)
    assert len(reads) == (2 if n else (1 if mask.size else 0)), reads
    lab = out["region_label"]
    assert lab.data.tensor.is_cuda and lab.data.tensor.dtype == torch.int32 and lab.dims == ("ping_time", "range_sample")
    assert dict(lab.attrs) == {"n_regions": n, "connectivity": connectivity}
    assert torch.equal(lab.data.tensor.cpu(), torch.from_numpy(want["region_label"]))
    np.testing.assert_array_equal(out["region"].values, np.arange(1, n + 1))
    np.testing.assert_array_equal(out["channel"].values, ds["channel"].values)
    for k in EQUAL:
        assert isinstance(out[k].data, np.ndarray) and out[k].dims == ("region",), k
        np.testing.assert_array_equal(out[k].values, want[k], err_msg=k)
    for k in EQUAL_C + DERIVED + ("Sv_mean",):
        assert isinstance(out[k].data, np.ndarray) and out[k].dims == ("channel", "region"), k
    for k in EQUAL_C:
        np.testing.assert_array_equal(out[k].values, want[k.replace("depth", "range")], err_msg=k)
    for k in DERIVED:
        np.testing.assert_allclose(out[k].values, want[k.replace("depth", "range")], rtol=1e-9, atol=0, err_msg=k)
    np.testing.assert_allclose(out["Sv_mean"].values, want["Sv_mean"], rtol=0, atol=1e-8, err_msg="Sv_mean")
    if n:
        _check_sums(_raw_sums(sv, depth, depth_dims, mask, connectivity), want)
    return out, want


def _check_sums(tabs, want):
    np.testing.assert_array_equal(tabs["n_samples"], want["n_samples"])
    np.testing.assert_array_equal(tabs["n_valid"], want["n_valid"])
    for name in R.SUMS:
        val, absum, cnt = want["sums"][name]
        err = np.abs(tabs[name] - val)
        bound = (cnt + 8) * 2.0 ** -52 * absum
        worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
        print(f"{name}: largest error / bound = {worst:.3f} over {err.size} entries, up to {int(cnt.max())} terms")
        assert np.all(err <= bound), (name, worst)


def _ramp(C, P, S, dtype=np.float64):
    """Positive depths increasing along the samples, different in every channel and ping: (C, P, S)."""
    c, p, s = np.meshgrid(np.arange(C), np.arange(P), np.arange(S), indexing="ij")
    return (3.0 + 0.5 * c + 0.015625 * p + (0.25 + 0.0625 * c) * s).astype(dtype)


def _sv(C, P, S, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    sv = (-70.0 + 6.0 * rng.standard_normal((C, P, S))).astype(dtype)
    sv[rng.random((C, P, S)) < 0.05] = np.nan
    return sv


FULL = ("channel", "ping_time", "range_sample")


def test_the_smallest_plane():
    """P = S = 1: one region of one pixel; a single sample has no dz (height_mean and NASC sum nothing)."""
    sv = np.array([[[-63.5]], [[np.nan]]])
    out, _ = _check(sv, _ramp(2, 1, 1), FULL, np.ones((1, 1), dtype=bool), 8, n_regions=1)
    assert out["n_valid"].values.tolist() == [[1], [0]] and out["Sv_mean"].values[0, 0] == pytest.approx(-63.5, abs=1e-8)
    assert np.isnan(out["Sv_mean"].values[1, 0]) and np.isnan(out["Sv_max"].values[1, 0])
    assert out["height_mean"].values.tolist() == [[0.0], [0.0]] and out["NASC"].values.tolist() == [[0.0], [0.0]]


@pytest.mark.parametrize("runs", [[(0, 0), (2, 5), (60, 66), (120, 127), (129, 129)],      # across 63/64, ending on 127
                                  [(61, 63), (65, 70), (100, 128)],                      # ending on 63, across 127/128
                                  [(64, 64), (66, 127)], [(1, 62), (128, 129)], [(0, 129)]])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_runs_cut_by_a_wave_edge(runs, connectivity):
    P, S = 1, 130
    mask = np.zeros((P, S), dtype=bool)
    for a, b in runs:
        mask[0, a:b + 1] = True
    _check(_sv(2, P, S, 5), _ramp(2, P, S), FULL, mask, connectivity, n_regions=len(runs))


@pytest.mark.parametrize("connectivity,n", [(4, 98), (8, 1)])
def test_checkerboard(connectivity, n):
    """3 x 65: at connectivity 4 every second pixel is a region of its own -- 98, the capacity of the labelling's
    table; at 8 they are one."""
    from echopype_amd import ops

    P, S = 3, 65
    pp, ss = np.meshgrid(np.arange(P), np.arange(S), indexing="ij")
    assert ops.shoal_table_capacity(P, S, 4) == 98
    _check(_sv(2, P, S, 6), _ramp(2, P, S), FULL, (pp + ss) % 2 == 0, connectivity, n_regions=n)


def test_one_region_every_wave_on_one_entry():
    """70 x 64, all True: three chunks of pings, every wave updates the same entry."""
    P, S = 70, 64
    out, _ = _check(_sv(2, P, S, 7), _ramp(2, P, S), FULL, np.ones((P, S), dtype=bool), 4, n_regions=1)
    assert out["n_samples"].values.tolist() == [P * S]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_interleaved_combs(connectivity):
    """40 x 64: the teeth of region A on samples 0, 4, 8, ... hang from a spine at ping 0, those of region B on samples
    2, 6, ... stand on a spine at the last ping, background between: the codes alternate inside every wave."""
    P, S = 40, 64
    mask = np.zeros((P, S), dtype=bool)
    mask[0, :] = True
    mask[:P - 2, 0::4] = True
    mask[P - 1, :] = True
    mask[2:, 2::4] = True
    out, _ = _check(_sv(3, P, S, 8), _ramp(3, P, S), FULL, mask, connectivity, n_regions=2)
    assert out["ping_first"].values.tolist() == [0, 2] and out["ping_last"].values.tolist() == [P - 3, P - 1]


def test_empty_mask_launches_no_statistics_kernel():
    import echopype_amd as ep
    from echopype_amd import _lib

    P, S = 5, 70
    with _lib.launch_trace() as t:
        out, _ = _check(_sv(2, P, S, 9), _ramp(2, P, S), FULL, np.zeros((P, S), dtype=bool), 8, n_regions=0)
        lab = ep.mask.label_regions(np.zeros((P, S), dtype=bool))
        none, _ = _check(np.zeros((2, 0, S)), np.zeros((2, S)), ("channel", "range_sample"), np.zeros((0, S), dtype=bool),
                         8, n_regions=0)
    assert "sh_box_kernel" in t.kernels
    assert "region_stats_kernel" not in t.kernels and "region_labels_kernel" not in t.kernels
    for o in (out, none):
        assert o["region"].shape == (0,) and o["n_samples"].shape == (0,) and o["NASC"].shape == (2, 0)
        assert o["ping_time_start"].dtype == _ping_time(1).dtype
    assert lab.attrs["n_regions"] == 0 and not bool(lab.data.tensor.any()) and tuple(lab.shape) == (P, S)
    assert tuple(none["region_label"].shape) == (0, S)


# ---- the realistic mix ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """synth.shoal_scene() (90 x 120) as channel 0 of a C = 3 cube of float32-representable values, the other channels
    offset copies; the mask is Sv > -70 of channel 0 with gaps of up to 3 samples filled, so it covers NaN pixels; the
    Sv of the largest 8-connected region is all NaN in channel 2.  scipy finds 154 regions in that mask at connectivity 4
    and 148 at 8, the largest of 280 and 281 pixels (the unfilled ``Sv > -70``: 191 and 166, of 244 and 254)."""
    import torch

    from echopype_amd import ops, synth

    base = synth.shoal_scene().astype(np.float32)
    sv = np.stack([base, base - np.float32(3.5), np.roll(base, 7, axis=1) + np.float32(1.25)])
    mask = ops.shoal_threshold_fill(torch.from_numpy(base).cuda(), -70.0, maxvgap=3).cpu().numpy()
    assert np.isnan(base[mask]).any()
    lab, n = R.label(mask, 8)
    big = int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
    sv[2][lab == big] = np.nan
    return {"sv": sv, "mask": mask, "big": big, "oracle": {}}


def _depth(form):
    C, P, S = 3, 90, 120
    d = _ramp(C, P, S, np.float32) if form == "cps" else _ramp(C, 1, S, np.float32)[:, 0]
    d = d.copy()
    d[1, ..., -7:] = np.nan
    return d, (FULL if form == "cps" else ("channel", "range_sample"))


@pytest.mark.parametrize("connectivity,n_regions,largest", [(4, 154, 280), (8, 148, 281)])
@pytest.mark.parametrize("form", ["cps", "cs"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_school_scene(scene, dtype, form, connectivity, n_regions, largest):
    depth, dims = _depth(form)
    sv = scene["sv"].astype(dtype)
    out, want = _check(sv, depth.astype(dtype), dims, scene["mask"], connectivity, n_regions=n_regions)
    assert int(out["n_samples"].values.max()) == largest
    if connectivity == 8:
        k = scene["big"] - 1
        assert out["n_valid"].values[2, k] == 0 and out["n_samples"].values[k] == largest
        assert np.isnan(out["Sv_mean"].values[2, k]) and np.isnan(out["Sv_max"].values[2, k])
        assert np.isnan(out["center_of_mass"].values[2, k]) and out["NASC"].values[2, k] == 0.0
        assert np.isfinite(out["Sv_mean"].values[:2, k]).all() and np.isfinite(out["depth_mean"].values[2, k])
    # the depth of channel 1 is NaN on its last 7 samples: regions that reach them count fewer ranges than pixels
    assert (out["n_valid"].values[1] <= out["n_samples"].values).all()
    # float32 and float64 storage of the same values: one result
    key = (form, connectivity)
    first = scene["oracle"].setdefault(key, out)
    if first is not out:
        for k in EQUAL + EQUAL_C:
            np.testing.assert_array_equal(first[k].values, out[k].values, err_msg=k)
        for k in DERIVED:
            np.testing.assert_allclose(first[k].values, out[k].values, rtol=1e-9, atol=0, err_msg=k)
        np.testing.assert_allclose(first["Sv_mean"].values, out["Sv_mean"].values, rtol=0, atol=1e-8)


def test_two_calls_agree_and_inputs_of_every_kind(scene):
    """Two calls give identical labels, counts, boxes and extrema (the sums are held to their bound by _check).  The
    mask as a bool DataArray on the device with its dimensions swapped and a channel of length 1, as a torch tensor, as
    a host array; Sv with the channel last, on the host; depth on (range_sample,) alone."""
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    sv, mask = scene["sv"], scene["mask"]
    depth, dims = _depth("cs")
    a, _ = _check(sv, depth, dims, mask, 8)
    b, _ = _check(sv, depth, dims, mask, 8, on_device=False)
    for k in EQUAL + EQUAL_C:
        np.testing.assert_array_equal(a[k].values, b[k].values, err_msg=k)
    assert torch.equal(a["region_label"].data.tensor, b["region_label"].data.tensor)

    C, P, S = sv.shape
    m_dev = DataArray(DeviceArray(torch.from_numpy(mask.T[None].copy()).cuda()), ("channel", "range_sample", "ping_time"),
                      coords={"ping_time": _ping_time(P), "range_sample": np.arange(S)})
    la = ep.mask.label_regions(m_dev)
    lb = ep.mask.label_regions(torch.from_numpy(mask).cuda(), connectivity=8)
    lc = ep.mask.label_regions(mask.astype(np.uint8))
    for lab in (la, lb, lc):
        assert lab.name == "region_label" and lab.dims == ("ping_time", "range_sample")
        assert torch.equal(lab.data.tensor, a["region_label"].data.tensor)
        assert lab.attrs["n_regions"] == 148
    np.testing.assert_array_equal(la.coords["ping_time"], _ping_time(P))

    ds = Dataset(coords={"channel": np.array(["a", "b", "c"]), "ping_time": _ping_time(P), "range_sample": np.arange(S)})
    ds["Sv"] = (("ping_time", "range_sample", "channel"), np.ascontiguousarray(sv.transpose(1, 2, 0)))
    ds["depth"] = (("range_sample",), depth[0])
    c = ep.mask.region_statistics(ds, m_dev)
    want = R.statistics(sv, depth[0], mask, 8)
    np.testing.assert_array_equal(c["n_valid"].values, want["n_valid"])
    np.testing.assert_array_equal(c["depth_max"].values, want["range_max"])
    np.testing.assert_allclose(c["NASC"].values, want["NASC"], rtol=1e-9, atol=0)
    # a plane without channel: the per-channel variables lie on region alone
    ds1 = Dataset(coords={"ping_time": _ping_time(P), "range_sample": np.arange(S)})
    ds1["Sv"] = (("ping_time", "range_sample"), sv[0])
    ds1["echo_range"] = (("ping_time", "range_sample"), _ramp(1, P, S)[0])
    d = ep.mask.region_statistics(ds1, mask, range_var="echo_range", connectivity=4)
    want1 = R.statistics(sv[:1], _ramp(1, P, S), mask, 4)
    assert d["Sv_mean"].dims == ("region",) and "channel" not in d.coords
    np.testing.assert_array_equal(d["echo_range_min"].values, want1["range_min"][0])
    np.testing.assert_allclose(d["Sv_mean"].values, want1["Sv_mean"][0], rtol=0, atol=1e-8)


def test_labels_give_the_mask_back_to_apply_mask(scene):
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray, DeviceArray

    sv, mask = scene["sv"].astype(np.float64), scene["mask"]
    depth, dims = _depth("cps")
    ds = _dataset(sv, depth.astype(np.float64), dims)
    lab = ep.mask.label_regions(mask, connectivity=4)
    again = DataArray(DeviceArray(lab.data.tensor > 0), lab.dims, coords=dict(lab.coords), name="mask")
    m = DataArray(DeviceArray(torch.from_numpy(mask).cuda()), lab.dims, coords=dict(lab.coords), name="mask")
    a = ep.mask.apply_mask(ds, again)["Sv"].data.tensor
    b = ep.mask.apply_mask(ds, m)["Sv"].data.tensor
    assert torch.equal(torch.nan_to_num(a, nan=1.0), torch.nan_to_num(b, nan=1.0))
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and bool(torch.isnan(a[0][~torch.from_numpy(mask).cuda()]).all())
