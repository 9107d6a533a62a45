"""``utils.align_to_ping_time`` and ``consolidate.add_location`` on a real MI355X: the kernel ``epa_align_to_ping_time``
against the NumPy restatement (tests/location_ref.py, itself held bit for bit to the reference's executed results by
tests/test_location_host.py) -- bit for bit in both modes, no tolerance: every operation of the linear formula is one
correctly rounded IEEE operation, so a differing bit means a contracted fma or a fast division --, add_location end to
end on a small EK60 EchoData, and the chain it exists for: compute_Sv -> add_depth -> add_location -> compute_NASC."""
import numpy as np
import pytest

import location_cases as C
import location_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert int(np.isnan(got).sum()) == int(np.isnan(want).sum()), (what, "NaN count")
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), got[~same][:4], want[~same][:4])


def _ext(ep, c, rows, on_device=False):
    import torch

    out = []
    for v in rows:
        data = ep.DeviceArray(torch.from_numpy(c["y"][v].copy()).cuda()) if on_device else c["y"][v]
        out.append(ep.DataArray(data, ("time1",), {"time1": c["t_ext"]}, {"units": "degrees"}, f"row{v}"))
    return out


def _ping(ep, c):
    return ep.DataArray(c["ping_time"], ("ping_time",), {"ping_time": c["ping_time"]})


# ---- the kernel, through the public helper -------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("name", list(C.ALIGN_CASES))
def test_align_equals_the_restatement_bit_for_bit(ep, name, method):
    from echopype_amd import _lib
    from echopype_amd.utils.align import align_many_to_ping_time

    c = C.align_case(name)
    V = c["y"].shape[0]
    want = R.align(c["t_ext"], c["y"], c["ping_time"], method)
    if name == "nat_ping":
        assert np.isnan(want[:, np.isnat(c["ping_time"])]).all()
    with _lib.launch_trace() as tr:  # all rows from one search: one launch
        got = align_many_to_ping_time(_ext(ep, c, range(V)), "time1", _ping(ep, c), method)
    assert tr.kernels == ["align_to_ping_time_kernel"], tr.kernels
    for v in range(V):
        assert isinstance(got[v].data, ep.DeviceArray) and got[v].dtype == np.float64
        assert got[v].dims == ("ping_time",) and "time1" not in got[v].coords and got[v].attrs == {"units": "degrees"}
        np.testing.assert_array_equal(got[v].coords["ping_time"], c["ping_time"])
        assert_bits(got[v].values, want[v], f"{name} {method} row {v} of {V}")
    # a row on its own (V = 1), from a variable that already lives on the device
    one = ep.utils.align_to_ping_time(_ext(ep, c, [V - 1], on_device=True)[0], "time1", _ping(ep, c), method=method)
    assert_bits(one.values, want[V - 1], f"{name} {method} row {V - 1} alone")


def test_ops_checks_its_arguments(ep):
    import torch

    t = torch.arange(4, dtype=torch.int64, device="cuda")
    y = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="'linear' or 'nearest'"):
        ep.ops.align_to_ping_time(t, y, t, "cubic")
    with pytest.raises(ValueError, match=r"float64 of shape \(V, 4\)"):
        ep.ops.align_to_ping_time(t, y[:, :3].contiguous(), t)
    with pytest.raises(ValueError, match="1-D int64"):
        ep.ops.align_to_ping_time(t.double(), y, t)
    with pytest.raises(ValueError, match="must be on one device"):
        ep.ops.align_to_ping_time(t.cpu(), y, t)
    with pytest.raises(ValueError, match="N=1 external times"):
        ep.ops.align_to_ping_time(t[:1], y[:, :1].contiguous(), t)


# ---- add_location end to end ---------------------------------------------------------------------------------------------------
CH, P, S, FIXES = 2, 300, 64, 41


def _track(pt, N=FIXES, seed=7):
    """A vessel steaming at about 5 m/s along a track of N fixes that starts after the first pings and ends before the
    last ones; fixes alternate between NMEA sentences."""
    rng = np.random.default_rng(seed)
    t0, t1 = pt[0].astype(np.int64) + 10_000_000_000, pt[-1].astype(np.int64) - 10_000_000_000
    t = np.sort(rng.choice(np.arange(t0, t1, 1_000_000, dtype=np.int64), N, replace=False))
    lat = 45.0 + 4.5e-5 * (t - t0) / 1e9 + rng.normal(0, 2e-6, N)
    lon = -125.0 + 1.5e-5 * (t - t0) / 1e9 + rng.normal(0, 2e-6, N)
    sentence = np.array(["GGA", "RMC"])[np.arange(N) % 2]
    return t.astype("datetime64[ns]"), lat, lon, sentence


def _with_platform(ep, ed, t, lat, lon, sentence=None):
    plat = ep.Dataset()
    plat["latitude"] = ep.DataArray(lat, ("time1",), {"time1": t}, {"standard_name": "latitude", "units": "degrees_north"})
    plat["longitude"] = ep.DataArray(lon, ("time1",), {"time1": t}, {"standard_name": "longitude", "units": "degrees_east"})
    if sentence is not None:
        plat["sentence_type"] = ep.DataArray(sentence, ("time1",), {"time1": t})
    ed["Platform"] = plat
    return ed


@pytest.fixture(scope="module")
def survey(ep):
    """The EK60 EchoData with its navigation track, the Sv dataset with depth, and the restated positions."""
    from echopype_amd.echodata import BEAM1, from_ek60_arrays

    ed = from_ek60_arrays(ep.synth.ek60_numpy(C=CH, P=P, S=S))
    pt = np.asarray(ed[BEAM1]["ping_time"].values)
    t, lat, lon, sentence = _track(pt)
    _with_platform(ep, ed, t, lat, lon, sentence)
    ds = ep.consolidate.add_depth(ep.calibrate.compute_Sv(ed))
    want = R.align(t, np.stack([lat, lon]), pt, "linear")
    return dict(ed=ed, ds=ds, pt=pt, t=t, lat=lat, lon=lon, sentence=sentence, want=want)


def test_add_location_end_to_end(ep, survey):
    from echopype_amd import _lib

    ds, ed = survey["ds"], survey["ed"]
    before = (list(ds.data_vars), list(ds.coords), dict(ds.attrs))
    with _lib.launch_trace() as tr:
        out = ep.consolidate.add_location(ds, ed)
    assert tr.kernels == ["align_to_ping_time_kernel"], tr.kernels  # latitude and longitude: one launch
    assert (list(ds.data_vars), list(ds.coords), dict(ds.attrs)) == before and "latitude" not in ds  # a copy is returned
    assert "time1" not in out and out["Sv"].data is ds["Sv"].data
    assert out.attrs["processing_level"] == "Level 2A" and "processing_level" not in ds.attrs  # Sv with valid positions
    for i, v in enumerate(("latitude", "longitude")):
        assert isinstance(out[v].data, ep.DeviceArray) and out[v].dims == ("ping_time",) and out[v].dtype == np.float64
        assert_bits(out[v].values, survey["want"][i], v)
        assert out[v].attrs["standard_name"] == v
        assert out[v].attrs["history"].endswith(
            ". `depth` calculated using:Interpolated or propagated from Platform latitude/longitude.")
    # pings before the first and after the last fix: the end segments extrapolate
    assert survey["pt"][0] < survey["t"][0] and survey["pt"][-1] > survey["t"][-1]
    assert np.isfinite(out["latitude"].values).all() and out["latitude"].values[-1] > survey["lat"].max()
    # the restatement through its own add_location gives the same numbers
    plat = {"latitude": ("time1", survey["t"], survey["lat"]), "longitude": ("time1", survey["t"], survey["lon"]),
            "sentence_type": ("time1", survey["t"], survey["sentence"])}
    la, lo, warned = R.add_location(survey["pt"], plat, "EK60")
    assert warned == []
    assert_bits(out["latitude"].values, la, "latitude")
    assert_bits(out["longitude"].values, lo, "longitude")


def test_add_location_selects_the_nmea_sentence(ep, survey):
    out = ep.consolidate.add_location(survey["ds"], survey["ed"], nmea_sentence="GGA")
    keep = survey["sentence"] == "GGA"
    want = R.align(survey["t"][keep], np.stack([survey["lat"][keep], survey["lon"][keep]]), survey["pt"], "linear")
    assert_bits(out["latitude"].values, want[0], "latitude of GGA")
    assert_bits(out["longitude"].values, want[1], "longitude of GGA")
    assert not np.array_equal(want[0], survey["want"][0])  # (the subset is another track)


def test_one_fix_and_a_track_on_ping_time_launch_nothing(ep, survey):
    from echopype_amd import _lib
    from echopype_amd.echodata import EchoData

    pt = survey["pt"]
    ds = ep.Dataset(coords={"ping_time": pt})
    one = _with_platform(ep, EchoData("EK60"), survey["t"][:1], survey["lat"][:1], survey["lon"][:1])
    lat_p, lon_p = np.linspace(44.0, 44.1, len(pt)), np.linspace(-124.0, -124.2, len(pt))
    same = _with_platform(ep, EchoData("EK60"), pt.copy(), lat_p, lon_p)
    with _lib.launch_trace() as tr:
        a = ep.consolidate.add_location(ds, one)
        b = ep.consolidate.add_location(ds, same)
    assert tr.kernels == []
    assert (a["latitude"].values == survey["lat"][0]).all() and (a["longitude"].values == survey["lon"][0]).all()
    assert a["latitude"].shape == pt.shape and a["latitude"].dtype == np.float64
    np.testing.assert_array_equal(b["latitude"].values, lat_p)
    np.testing.assert_array_equal(b["longitude"].values, lon_p)
    assert "time1" not in a and "time1" not in b and "history" in b["longitude"].attrs


def test_split_pings_equal_the_whole(ep, survey):
    """Both halves measure time from the same first fix: nothing depends on where a ping sits in its launch."""
    pt, ed = survey["pt"], survey["ed"]
    halves = [ep.consolidate.add_location(ep.Dataset(coords={"ping_time": part}), ed) for part in (pt[:137], pt[137:])]
    for i, v in enumerate(("latitude", "longitude")):
        assert_bits(np.concatenate([h[v].values for h in halves]), survey["want"][i], v)


# ---- the chain it exists for ---------------------------------------------------------------------------------------------------
def test_located_dataset_goes_through_compute_NASC_and_compute_MVBS(ep, survey):
    """compute_NASC of the located dataset against compute_NASC of the same dataset with the restatement's positions
    assigned by hand, compared exactly.

    Distance bins, their positions and times are host arithmetic on the positions: exact on any grid.  The NASC values
    are sums that ``epa_nasc`` gathers with floating-point atomics, one partial sum per workgroup and
    min(4096 / cells, pings per distance bin) workgroups per cell: two calls on the SAME input add those partials in
    whatever order the workgroups finish.  With at most two workgroups per cell the order cannot matter (a + b = b + a),
    and inside a workgroup the 64 samples of a ping are one wave's work, ping after ping.  So NASC is compared on a
    grid of at least P / 2 distance bins (0.005 nmi at 5 m/s and a ping a second), where equal positions give equal bits;
    the coarse grid compares everything but the NASC values."""
    ds, ed = survey["ds"], survey["ed"]
    located = ep.consolidate.add_location(ds, ed)
    by_hand = ds.copy()
    by_hand["latitude"] = (("ping_time",), survey["want"][0].copy(), dict(located["latitude"].attrs))
    by_hand["longitude"] = (("ping_time",), survey["want"][1].copy(), dict(located["longitude"].attrs))
    for dist_bin, with_nasc in (("0.1nmi", False), ("0.005nmi", True)):
        got = ep.commongrid.compute_NASC(located, range_bin="2m", dist_bin=dist_bin)
        want = ep.commongrid.compute_NASC(by_hand, range_bin="2m", dist_bin=dist_bin)
        n_dist = got["NASC"].shape[1]
        assert got["NASC"].shape == want["NASC"].shape and (n_dist >= P / 2 if with_nasc else 3 <= n_dist <= 20)
        assert np.isfinite(want["NASC"].values).any()
        for v in ("distance", "depth", "latitude", "longitude"):
            assert_bits(got[v].values, want[v].values, f"{dist_bin} {v}")
        np.testing.assert_array_equal(got["ping_time"].values, want["ping_time"].values)
        if with_nasc:
            assert_bits(got["NASC"].values, want["NASC"].values, f"{dist_bin} NASC")

    mvbs = ep.commongrid.compute_MVBS(located, range_var="depth", range_bin="2m", ping_time_bin="20s")
    assert mvbs.attrs["processing_level"] == "Level 3A"  # (inherited from the located dataset's Level 2A)
    mvbs_hand = ep.commongrid.compute_MVBS(by_hand, range_var="depth", range_bin="2m", ping_time_bin="20s")
    for v in ("latitude", "longitude"):
        assert v in mvbs and mvbs[v].dims == ("ping_time",)
        assert_bits(mvbs[v].values, mvbs_hand[v].values, f"MVBS {v}")


# ---- the reference's own add_location results, through the package and the kernel -------------------------------------------
def _golden_cases():
    return [r["name"] for r in C.load_fixture()[1] if "raised" not in r]


@pytest.mark.parametrize("name", _golden_cases())
def test_add_location_equals_the_reference_executed_results(ep, name, caplog):
    """Every case the reference's add_location answered (NMEA positions, ``latitude_mru1`` / ``latitude_idx`` on their own
    time dimensions, a sentence subset, NaNs and zeros in the track, AZFP): the package's result against the stored
    one bit for bit, with the reference's ``history`` wording, attributes and warnings."""
    import logging

    from echopype_amd import _lib
    from test_location_host import dataset_of, echodata_of

    _, records, z = C.load_fixture()
    rec = next(r for r in records if r["name"] == name)
    c = C.location_case(name)
    ds = dataset_of(c)
    with caplog.at_level(logging.WARNING, logger="echopype_amd.consolidate"), _lib.launch_trace() as tr:
        out = ep.consolidate.add_location(ds, echodata_of(c), c["datagram_type"], c["nmea_sentence"])
    launched = name not in ("single_fix", "track_on_ping_time")
    assert tr.kernels == (["align_to_ping_time_kernel"] if launched else []), tr.kernels
    assert [[r.levelname, r.getMessage()] for r in caplog.records if r.name == "echopype_amd.consolidate"] == rec["logged"]
    assert "latitude" not in ds and not any(t in out for t in ("time1", "time3", "time4"))
    for v in ("latitude", "longitude"):
        assert out[v].dims == ("ping_time",) and isinstance(out[v].data, ep.DeviceArray) == launched
        assert_bits(out[v].values, z[f"location/{name}/{v}"], f"{name} {v}")
        assert out[v].attrs["history"].partition(". ")[2] == rec["history"] and sorted(out[v].attrs) == rec["attrs"]
    assert out.attrs["processing_level"] == "Level 2A"
