"""clean.detect_transient on the GPU (csrc/transient.hip through ops.transient_* and the clean.transient_noise
package): the reference's own tests restated on synth.transient_scene, every reference-executed golden case (whole
masks: the generator keeps every fixture ping at least MARGIN from every threshold), seeded fuzz against
tests/transient_ref.py on the pings at least MARGIN from a threshold, device-resident results with only the documented
host copy, the bottom line of mask.detect_seafloor as bottom_var, the result into mask.apply_mask, and full-size
planes whose expected mask is a formula (constant background, raised pings)."""
import numpy as np
import pytest

import transient_ref as R

pytestmark = pytest.mark.gpu

DIMS = R.DIMS


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _dev_data(a):
    import torch

    from echopype_amd.xr_lite import DeviceArray

    return DeviceArray(torch.as_tensor(np.ascontiguousarray(a)).cuda())


def _scene_ds(C=2, P=150, S=420, dtype=np.float32, seed=41, on_device=True, **kw):
    """(dataset with Sv, depth (C, P, S) and bottom_depth (C, P); the per-channel scenes).  The water column reaches
    1047 m and more, the seafloor lies below the default 900-1000 m layer."""
    kw.setdefault("bottom_frac", (0.97, 1.05))
    from echopype_amd import synth
    from echopype_amd.xr_lite import DataArray, Dataset

    sc = [synth.transient_scene(P=P, S=S, seed=seed + c, dtype=dtype, dz=2.5 + 0.1 * c, **kw) for c in range(C)]
    wrap = _dev_data if on_device else (lambda a: a)
    ds = Dataset(coords={"channel": np.array([f"chan{c + 1}" for c in range(C)]),
                         "ping_time": np.datetime64("2026-01-01") + np.arange(P) * np.timedelta64(1, "s"),
                         "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(wrap(np.stack([s["Sv"] for s in sc])), DIMS, name="Sv")
    ds["depth"] = DataArray(wrap(np.ascontiguousarray(np.broadcast_to(np.stack([s["depth"] for s in sc])[:, None, :],
                                                                       (C, P, S)))), DIMS)
    ds["bottom_depth"] = DataArray(wrap(np.stack([s["bottom"] for s in sc])), DIMS[:2])
    return ds, sc


# ---- the reference's tests (echopype/tests/clean/test_transient_noise.py) on a synthetic water column --------------------
def test_dispatcher_rejects_unsupported_method():
    import echopype_amd as ep

    ds, _ = _scene_ds()
    with pytest.raises(ValueError, match="Unsupported transient noise removal method"):
        ep.clean.detect_transient(ds, method="not_a_method", params={})


@pytest.mark.parametrize("method,expected_name", [("fielding", "fielding_mask_valid"), ("matecho", "matecho_mask_valid")])
def test_dispatcher_returns_named_boolean_mask(method, expected_name):
    import torch

    import echopype_amd as ep

    ds, _ = _scene_ds()
    mask = ep.clean.detect_transient(ds, method=method, params={"range_var": "depth"})
    assert mask.dtype == bool and mask.data.tensor.dtype == torch.bool and mask.data.tensor.is_cuda
    assert mask.name == expected_name
    assert mask.attrs == {"meaning": "True = VALID (False = transient noise)"}
    sv = ds["Sv"]
    assert tuple(mask.dims) == tuple(sv.dims) and mask.shape == sv.shape
    for dim in sv.dims:
        np.testing.assert_array_equal(mask.coords[dim], sv.coords[dim])


def test_fielding_dimensions_and_determinism():
    import torch

    import echopype_amd as ep

    ds, sc = _scene_ds()
    params = dict(range_var="depth", r0=900, r1=1000, n=30, thr=(3, 1), roff=20, jumps=5, maxts=-35, start=0)
    m1 = ep.clean.detect_transient(ds, "fielding", params)
    m2 = ep.clean.detect_transient(ds, "fielding", params)
    assert tuple(m1.dims) == tuple(ds["Sv"].dims)
    assert torch.equal(m1.data.tensor, m2.data.tensor) and m1.name == m2.name and m1.attrs == m2.attrs
    got = m1.values
    assert 0 < (~got).sum() < got.size
    for c, s in enumerate(sc):  # the raised pings away from the ends are what is masked
        inner = [int(j) for j in s["pings"] if 30 <= j <= 150 - 1 - 30]
        assert set(np.flatnonzero(~got[c].all(axis=1))) <= set(inner) and inner


def test_invalid_inputs_raise():
    import echopype_amd as ep

    ds, _ = _scene_ds()
    for method in ("fielding", "matecho"):
        for name in ("Sv", "depth"):
            bad = ds.drop_vars(name)
            with pytest.raises(ValueError):
                ep.clean.detect_transient(bad, method, dict(range_var="depth"))


def test_matecho_dimensions_determinism_and_threshold_monotonicity():
    import torch

    import echopype_amd as ep

    ds, _ = _scene_ds()
    base = dict(range_var="depth", start_depth=220, window_meter=450, window_ping=100, percentile=25, extend_ping=0,
                min_window=20)
    m1 = ep.clean.detect_transient(ds, "matecho", dict(base, delta_db=12))
    m2 = ep.clean.detect_transient(ds, "matecho", dict(base, delta_db=12))
    assert tuple(m1.dims) == tuple(ds["Sv"].dims) and torch.equal(m1.data.tensor, m2.data.tensor)
    low = ep.clean.detect_transient(ds, "matecho", dict(base, delta_db=8))
    high = ep.clean.detect_transient(ds, "matecho", dict(base, delta_db=16))
    n_low, n_high = int(low.data.tensor.sum()), int(high.data.tensor.sum())
    assert n_high >= n_low and n_low < low.data.tensor.numel()  # delta_db = 8 flags something


def test_matecho_bottom_var_optional():
    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray

    ds, _ = _scene_ds()
    prm = dict(range_var="depth", start_depth=220, window_meter=450, window_ping=50, delta_db=12)
    m = ep.clean.detect_transient(ds, "matecho", prm)
    assert tuple(m.dims) == tuple(ds["Sv"].dims)
    # a shallow constant bottom, 300 m under a 220 m window top: runs, keeps the dims
    ds["bottom_var"] = DataArray(np.full(ds.sizes["ping_time"], 300.0), ("ping_time",))
    for prm2 in (prm, dict(prm, bottom_var="bottom_var")):
        m = ep.clean.detect_transient(ds, "matecho", prm2)
        assert tuple(m.dims) == tuple(ds["Sv"].dims) and m.shape == ds["Sv"].shape


# ---- the reference-executed fixture ------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_every_golden_case(g, on_device):
    import torch

    import echopype_amd as ep

    n = 0
    for c in R.cases(g):
        ds = R.case_dataset(g, c, _dev_data if on_device else (lambda a: a))
        if "error" in c or "diverges" in c:  # ("diverges": refused here before any launch)
            typ, msg = c.get("error") or c["diverges"]
            with pytest.raises(Exception) as ei:
                ep.clean.detect_transient(ds, c["method"], R.case_params(c))
            assert type(ei.value).__name__ == typ and str(ei.value) == msg, c["tag"]
            continue
        assert (g[c["tag"] + "_margin"] >= R.MARGIN[c["dtype"]]).all(), c["tag"]  # whole masks are compared
        out = ep.clean.detect_transient(ds, c["method"], R.case_params(c))
        t = out.data.tensor
        assert t.is_cuda and t.dtype == torch.bool, c["tag"]
        want = torch.from_numpy(R.unpack_mask(g, c["tag"], c["shape"])).cuda()
        assert torch.equal(t, want), (c["tag"], int((~t).sum()), c["masked"])
        assert out.name == c["name"] and list(out.dims) == c["dims"] and dict(out.attrs) == c["attrs"], c["tag"]
        C, P, S = c["shape"]
        np.testing.assert_array_equal(out.coords["ping_time"], np.arange(P))
        np.testing.assert_array_equal(out.coords["range_sample"], np.arange(S))
        n += 1
    assert n >= 45


def test_empty_axes_return_without_a_launch():
    import echopype_amd as ep
    from echopype_amd import _lib
    from echopype_amd.xr_lite import DataArray, Dataset

    for P, S in ((0, 12), (7, 0)):
        ds = Dataset(coords={"channel": np.array(["chan1"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
        ds["Sv"] = DataArray(np.zeros((1, P, S)), DIMS)
        ds["depth"] = DataArray(np.zeros((1, P, S)), DIMS)
        with _lib.launch_trace() as t:
            for method in ("fielding", "matecho"):
                out = ep.clean.detect_transient(ds, method, {"range_var": "depth"})
                assert out.shape == (1, P, S) and out.data.tensor.is_cuda and bool(out.data.tensor.all())
        assert t.kernels == []


def test_sv_in_another_dimension_order_and_without_channel():
    """The mask comes back in the dims and order of Sv."""
    import echopype_amd as ep
    from echopype_amd import synth
    from echopype_amd.xr_lite import DataArray, Dataset

    sc = synth.transient_scene(P=90, S=200, seed=3)
    prm = dict(range_var="depth", r0=300, r1=380, n=8, roff=40, jumps=10)
    want, _ = R.fielding(sc["Sv"], sc["depth"], **{k: v for k, v in prm.items() if k != "range_var"})
    assert 0 < (~want).sum()
    ds = Dataset(coords={"channel": np.array(["chan1"]), "ping_time": np.arange(90), "range_sample": np.arange(200)})
    ds["Sv"] = DataArray(np.ascontiguousarray(sc["Sv"].T[None]), ("channel", "range_sample", "ping_time"))
    ds["depth"] = DataArray(np.ascontiguousarray(np.broadcast_to(sc["depth"][None, :, None], (1, 200, 90))),
                            ("channel", "range_sample", "ping_time"))
    out = ep.clean.detect_transient(ds, "fielding", prm)
    assert out.dims == ("channel", "range_sample", "ping_time")
    np.testing.assert_array_equal(out.values[0], want.T)
    ds2 = Dataset(coords={"ping_time": np.arange(90), "range_sample": np.arange(200)})
    ds2["Sv"] = DataArray(sc["Sv"], DIMS[1:])
    ds2["depth"] = DataArray(sc["depth"], ("range_sample",))
    out = ep.clean.detect_transient(ds2, "fielding", prm)
    assert out.dims == DIMS[1:]
    np.testing.assert_array_equal(out.values, want)


# ---- fuzz against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.fuzz_cases(), ids=lambda c: c[0])
def test_fuzz_against_the_oracle(case):
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray, Dataset

    tag, method, dt, C, P, S, seed, prm = case
    sv, rng, bottom = R.fuzz_inputs(case)
    valid, margin, compare = R.fuzz_expected(case)
    left = int((~compare).sum())
    assert left <= max(2, (C * P) // 100)  # (a condition on the inputs: test_transient_host.py asserts it on the CPU)
    ds = Dataset(coords={"channel": np.array([f"chan{c + 1}" for c in range(C)]), "ping_time": np.arange(P),
                         "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(_dev_data(sv), DIMS)
    ds["depth"] = DataArray(_dev_data(np.ascontiguousarray(np.broadcast_to(rng[:, None, :], (C, P, S)))), DIMS)
    call = dict(prm, range_var="depth")
    if bottom is not None:
        ds["bottom_depth"] = DataArray(_dev_data(bottom), DIMS[:2])
        call["bottom_var"] = "bottom_depth"
    got = ep.clean.detect_transient(ds, method, call).data.tensor
    assert got.dtype == torch.bool and tuple(got.shape) == (C, P, S)
    got = got.cpu().numpy()
    wrong = (got != valid).any(axis=2) & compare
    print(tag, "left out", left, "smallest margin", float(margin.min()), "masked pings", int((~valid.all(axis=2)).sum()))
    assert not wrong.any(), (tag, np.argwhere(wrong)[:5].tolist(), margin[wrong][:5])
    flagged = ~valid.all(axis=2)
    assert flagged[compare].any() and not flagged[compare].all()


# ---- on the device, into apply_mask, with the seafloor detector's bottom ---------------------------------------------------
def test_results_stay_on_the_device_and_one_copy_is_all_the_host_reads(monkeypatch):
    """Device inputs: torch's synchronisation debug mode raises on any blocking call; the only one either detector
    makes is the documented copy of the C range rows (counted through utils._to_host and let through)."""
    import torch

    import echopype_amd as ep
    from echopype_amd.clean.transient_noise import utils

    ds, sc = _scene_ds(C=2, P=150, S=420, dtype=np.float32)
    fprm = dict(range_var="depth", n=20, thr=(3, 1))
    mprm = dict(range_var="depth", bottom_var="bottom_depth", start_depth=500, window_meter=600, window_ping=40,
                delta_db=5)
    for _ in range(2):  # warm-up: staging pools, the allocator's blocks
        ep.clean.detect_transient(ds, "fielding", fprm)
        ep.clean.detect_transient(ds, "matecho", mprm)
    torch.cuda.synchronize()
    reads = []

    def counted(t):
        reads.append(t.numel())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return t.cpu()
        finally:
            torch.cuda.set_sync_debug_mode("error")

    monkeypatch.setattr(utils, "_to_host", counted)
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ep.clean.detect_transient(ds, "fielding", fprm)
        b = ep.clean.detect_transient(ds, "matecho", mprm)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    masked = ep.mask.apply_mask(ds, a)
    assert reads == [2 * 420, 2 * 420]
    assert a.data.tensor.is_cuda and b.data.tensor.is_cuda and masked["Sv"].data.tensor.is_cuda
    sv = np.stack([s["Sv"] for s in sc])
    rng = np.stack([s["depth"] for s in sc])
    wa, ma = R.detect("fielding", sv, rng, n=20, thr=(3, 1))
    wb, mb = R.detect("matecho", sv, rng, np.stack([s["bottom"] for s in sc]), start_depth=500, window_meter=600,
                      window_ping=40, delta_db=5)
    for got, want, mar in ((a.values, wa, ma), (b.values, wb, mb)):
        ok = mar >= R.MARGIN["float32"]
        assert (~ok).sum() <= 3 and (~want).any()
        np.testing.assert_array_equal(got[ok], want[ok])
    # the mask goes into apply_mask as it is: True = keep
    np.testing.assert_array_equal(np.asarray(masked["Sv"].values), np.where(a.values, sv, np.nan))


def test_bottom_var_from_detect_seafloor_on_the_device():
    import echopype_amd as ep

    ds, sc = _scene_ds(C=1, P=120, S=300, dtype=np.float64, seed=77, bottom_frac=(0.55, 0.8))
    line = ep.mask.detect_seafloor(ds, "basic", {"var_name": "Sv", "channel": "chan1", "threshold": (-40.0, 0.0),
                                                 "offset_m": 0.5, "bin_skip_from_surface": 20})
    assert line.data.tensor.is_cuda and line.dims == ("ping_time",)
    ds["bottom_depth"] = line
    prm = dict(range_var="depth", bottom_var="bottom_depth", start_depth=200, window_meter=400, window_ping=30,
               delta_db=4, min_window=20)
    out = ep.clean.detect_transient(ds, "matecho", prm)
    bottom = np.asarray(line.values)
    assert 350 < bottom.min() < bottom.max() < 650  # the line cuts the 200-600 m window
    want, mar = R.matecho(sc[0]["Sv"], sc[0]["depth"], bottom, start_depth=200, window_meter=400, window_ping=30,
                          delta_db=4, min_window=20)
    free, _ = R.matecho(sc[0]["Sv"], sc[0]["depth"], None, start_depth=200, window_meter=400, window_ping=30,
                        delta_db=4, min_window=20)
    ok = mar >= R.MARGIN["float64"]
    assert ok.all() and 0 < (~want).sum() < want.size and (want != free).any()  # the seafloor echo changes the answer
    np.testing.assert_array_equal(out.values[0], np.broadcast_to(want[:, None], (120, 300)))


def test_library_argument_checks():
    import torch

    from echopype_amd import ops

    sv = torch.full((2, 30, 64), -80.0, dtype=torch.float32, device="cuda")
    chan = np.array([[10, 20, 2, 3], [10, 20, 2, 3]])
    assert bool(ops.transient_fielding(sv, chan, 3, 3.0, 1.0, -35.0).all())
    with pytest.raises(ValueError, match="window rows outside"):
        ops.transient_fielding(sv, np.array([[10, 64, 2, 3], [10, 20, 2, 3]]), 3, 3.0, 1.0, -35.0)
    with pytest.raises(ValueError, match="does not fit 31 bits"):
        ops.transient_fielding(sv, chan, 2 ** 30, 3.0, 1.0, -35.0)
    rows = np.broadcast_to(np.arange(64.0), (2, 64))
    ci, cd = np.array([[5, 40], [5, 40]]), np.array([[1.0, 63.0], [1.0, 63.0]])
    assert bool(ops.transient_matecho(sv, rows, ci, cd, None, 5, 25.0, 12.0, 0, 20.0).all())
    with pytest.raises(ValueError, match="window rows outside"):
        ops.transient_matecho(sv, rows, np.array([[5, 65], [5, 40]]), cd, None, 5, 25.0, 12.0, 0, 20.0)
    with pytest.raises(ValueError, match="bottom must be float64"):
        ops.transient_matecho(sv, rows, ci, cd, torch.zeros(30, device="cuda"), 5, 25.0, 12.0, 0, 20.0)
    with pytest.raises(ValueError, match="percentile 101 outside"):
        ops.transient_matecho(sv, rows, ci, cd, None, 5, 101.0, 12.0, 0, 20.0)


# ---- full size: constant background, raised pings: medians are exact and the expected mask is a formula ----------------
BASE, GAIN = -80.0, 10.0


def _raised_cube(C, P, S, tops, period=97, phase=7):
    """f32 (C, P, S) on the device: BASE everywhere; ping j = phase (mod period) raised by GAIN from row
    tops[(j // period) % len(tops)] to the end.  -> (cube, the raised pings, their first rows)."""
    import torch

    sv = torch.full((C, P, S), BASE, dtype=torch.float32, device="cuda")
    pings = np.arange(phase, P, period)
    first = np.asarray(tops)[(pings // period) % len(tops)]
    for t in sorted(set(first.tolist())):
        idx = torch.from_numpy(pings[first == t]).cuda()
        sv[:, idx, t:] += GAIN
    return sv, pings, first


def _cube_ds(sv, dz, per_ping=False):
    """``depth``: the 1-D range_sample vector on the host, or (``per_ping``: Matecho takes the first ping's row) a
    (ping_time, range_sample) device array that repeats it without holding P copies."""
    import torch

    from echopype_amd.xr_lite import DataArray, DeviceArray, Dataset

    C, P, S = sv.shape
    ds = Dataset(coords={"channel": np.array([f"chan{c + 1}" for c in range(C)]), "ping_time": np.arange(P),
                         "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(DeviceArray(sv), DIMS, name="Sv")
    r = dz * np.arange(S, dtype=np.float64)
    if per_ping:
        ds["depth"] = DataArray(DeviceArray(torch.from_numpy(r).cuda()[None, :].expand(P, S)), DIMS[1:])
    else:
        ds["depth"] = DataArray(r, ("range_sample",))
    return ds


def _fielding_first_rows(first, up, lw, rmin, sf, S, thr):
    """The walk of the reference on a column that is BASE above row t and BASE + GAIN from it on, beside quiet
    neighbours: window medians are BASE or BASE + GAIN exactly when t is a multiple of sf away from up (no window
    straddles t).  -> first masked row per raised ping, S where the ping is not flagged."""
    out = []
    for t in first:
        assert (up - t) % sf == 0 and t <= up
        r0 = up - sf
        while r0 > rmin:
            diff = GAIN if r0 >= t else 0.0
            r0 -= sf
            if diff < thr[1]:
                break
        out.append(S + r0 if r0 < 0 else r0)
    return np.asarray(out)


def _check_fielding_cube(C, P, S):
    import torch

    import echopype_amd as ep

    dz, n, thr = 0.4, 30, (3.0, 1.0)
    # the defaults: r0 = 900 m, r1 = 1000 m > r[-1] = 999.6 m, roff = 20 m, jumps = 5 m
    up, lw, rmin, sf = R.fielding_rows(dz * np.arange(S, dtype=np.float64), 900, 1000, 20, 5)
    assert (up, lw, rmin) == (2250, 2499, 50) and sf in (12, 13)
    tops = [up - 100 * sf, up, up - sf, 10 + (up - 10) % sf]  # ..., the last one above rmin: the walk runs out there
    sv, pings, first = _raised_cube(C, P, S, tops)
    out = ep.clean.detect_transient(_cube_ds(sv, dz), "fielding", {"range_var": "depth"}).data.tensor
    assert out.dtype == torch.bool and tuple(out.shape) == (C, P, S)
    rows = _fielding_first_rows(first, up, lw, rmin, sf, S, thr)
    rows[(pings < n) | (pings > P - 1 - n)] = S  # within n pings of an end: never flagged
    start = torch.full((P,), S, dtype=torch.int64, device="cuda")
    start[torch.from_numpy(pings).cuda()] = torch.from_numpy(rows).cuda()
    want = torch.arange(S, device="cuda")[None, :] < start[:, None]
    assert int((~want).sum()) > 1000 * 200 * (P // 200_000)
    for c in range(C):
        assert torch.equal(out[c], want), c
    return out, pings, rows


def test_full_size_fielding():
    out, pings, rows = _check_fielding_cube(1, 200_000, 2500)
    assert len(set(rows.tolist())) == 5  # four different walks, and the pings at the ends


def _check_matecho_cube(C, P, S):
    import torch

    import echopype_amd as ep

    dz = 0.4
    # defaults: rows 550 .. 1675 (220 - 670 m), h = 50, 25th percentile = BASE, delta_db = 12 > GAIN: lower it to 8
    r = dz * np.arange(S, dtype=np.float64)
    inside = np.flatnonzero((r >= 220) & (r <= 220 + 450))
    s_lo, s_top = int(inside[0]), int(inside[-1]) + 1
    assert abs(s_lo - 550) <= 1 and abs(s_top - 1676) <= 1
    mid = (s_lo + s_top) // 2  # raised over half the window: 10 log10((1 + 10) / 2) = 7.4 dB above BASE: not flagged
    sv, pings, first = _raised_cube(C, P, S, [100, s_lo, mid, s_top, 2400])
    out = ep.clean.detect_transient(_cube_ds(sv, dz, per_ping=True), "matecho", {"range_var": "depth", "delta_db": 8,
                                                                  "extend_ping": 1}).data.tensor
    bad = np.zeros(P, dtype=bool)
    hit = pings[first <= s_lo]
    for d in (-1, 0, 1):
        bad[np.clip(hit + d, 0, P - 1)] = True
    want = torch.from_numpy(~bad).cuda()[:, None].expand(P, S)
    for c in range(C):
        assert torch.equal(out[c], want), c
    assert bad.sum() == 3 * len(hit) > 2000


def test_full_size_matecho():
    _check_matecho_cube(1, 200_000, 2500)


def test_more_than_2_to_31_elements():
    """One cube of 3 x 300 000 x 2500 = 2.25e9 samples through both methods (64-bit element indices)."""
    C, P, S = 3, 300_000, 2500
    assert C * P * S > 2 ** 31
    out, pings, rows = _check_fielding_cube(C, P, S)
    assert not bool(out[2, int(pings[-40]), -1])  # masked samples at the far end of the cube
    del out
    _check_matecho_cube(C, P, S)


def test_random_full_size_plane_on_a_subset_of_pings():
    """1 x 200 000 x 2500 random f32 with raised pings: some pings, with the pings their windows reach, are copied to
    the host and decided by the oracle."""
    import torch

    import echopype_amd as ep

    P, S, dz = 200_000, 2500, 0.4
    gen = torch.Generator(device="cuda").manual_seed(5)
    sv = -78.0 + 2.0 * torch.randn((1, P, S), generator=gen, device="cuda", dtype=torch.float32)
    raised = np.arange(11, P, 53)
    tops = 300 + 37 * (np.arange(len(raised)) % 50)
    gains = 2.0 + 0.25 * (np.arange(len(raised)) % 40)
    for t in np.unique(tops):
        sel = tops == t
        sv[0, torch.from_numpy(raised[sel]).cuda(), t:] += torch.from_numpy(gains[sel]).float().cuda()[:, None]
    ds = _cube_ds(sv, dz, per_ping=True)
    fprm = dict(r0=900, r1=990, n=30, thr=(3, 1), roff=100, jumps=25, maxts=-35)
    mprm = dict(start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=4, min_window=20)
    mf = ep.clean.detect_transient(ds, "fielding", dict(fprm, range_var="depth")).data.tensor
    mm = ep.clean.detect_transient(ds, "matecho", dict(mprm, range_var="depth")).data.tensor
    r = dz * np.arange(S, dtype=np.float64)
    rs = np.random.default_rng(9)
    some = np.unique(np.r_[rs.choice(raised[(raised > 60) & (raised < P - 60)], 14, replace=False),
                           rs.integers(60, P - 60, 6), 50, P - 51])
    seen = {"fielding": [0, 0], "matecho": [0, 0]}
    for j in some.tolist():
        w = 50
        sub = sv[0, j - w:j + w].cpu().numpy()
        vf, marf = R.fielding(sub, r, pings=[w], **fprm)
        vm, marm = R.matecho(sub, r, pings=[w], **mprm)
        if marf[0] >= R.MARGIN["float32"]:
            np.testing.assert_array_equal(mf[0, j].cpu().numpy(), vf[0], err_msg=f"fielding ping {j}")
            seen["fielding"][int(vf[0].all())] += 1
        if marm[0] >= R.MARGIN["float32"]:
            assert bool(mm[0, j].all()) == bool(vm[0]) and bool(mm[0, j].any()) == bool(vm[0]), f"matecho ping {j}"
            seen["matecho"][int(vm[0])] += 1
    assert all(min(v) >= 2 and sum(v) >= len(some) - 2 for v in seen.values()), seen
