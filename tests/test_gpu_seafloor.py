"""mask.detect_seafloor on the GPU (csrc/seafloor.hip through ops.seafloor_* and the seafloor_detection package):
every reference-executed golden case bit for bit, seeded fuzz against tests/seafloor_ref.py (tile-crossing
components, a spiral and a diagonal-only checkerboard for long union-find chains, windows larger than the crop), the
whole chain from EK60 samples, device-resident results with only the documented host reads, and full-size
known-answer lines (basic over more than 2^31 samples of one channel, Blackwell over 1e6 x 2500)."""

import numpy as np
import pytest

import seafloor_ref as R
from test_seafloor_host import _cases, _inputs, _lite_ds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _thr_bw(p):
    thr = p.get("threshold", -75)
    if np.ndim(thr) == 0:
        return float(thr), 702.0, 282.0
    return (float(thr[0]), 702.0, 282.0) if len(thr) == 2 else tuple(float(t) for t in thr)


def _to_dev(ds):
    """The same dataset with every variable as a device array."""
    import torch

    from echopype_amd.xr_lite import Dataset, DeviceArray, DataArray

    out = Dataset(coords={k: c for k, c in ds.coords.items()})
    for k, v in ds.data_vars.items():
        out[k] = DataArray(DeviceArray(torch.as_tensor(np.ascontiguousarray(v.values)).cuda()), v.dims, name=k)
    return out


@pytest.mark.parametrize("on_device", [False, True])
def test_every_golden_case(g, on_device):
    import echopype_amd as ep

    n = 0
    for c in _cases(g):
        ds = _lite_ds(_inputs(g, c), **c["flags"])
        if on_device:
            ds = _to_dev(ds)
        if "error" in c:
            typ, msg = c["error"]
            with pytest.raises(Exception) as ei:
                ep.mask.detect_seafloor(ds, c["method"], c["params"])
            assert type(ei.value).__name__ == typ, c["tag"]
            assert str(ei.value) == msg, c["tag"]
            continue
        out = ep.mask.detect_seafloor(ds, c["method"], c["params"])
        assert out.data.tensor.is_cuda
        want = g[f"{c['tag']}_out"]
        got = out.values
        assert got.dtype == want.dtype, c["tag"]
        np.testing.assert_array_equal(got, want, err_msg=c["tag"])
        assert out.name == c["name"] and list(out.dims) == c["dims"]
        assert dict(out.attrs) == c["attrs"], c["tag"]
        np.testing.assert_array_equal(out.coords["ping_time"], np.arange(want.size))
        n += 1
    assert n >= 20


def _run_bw(sv, theta, phi, depth, tsv, tt, tp, offset=0.3, r0=0, r1=1e9, wt=28, wp=52):
    import echopype_amd as ep

    ds = _lite_ds({"sv": sv, "theta": theta, "phi": phi, "depth": depth})
    out = ep.mask.detect_seafloor(ds, "blackwell", {"var_name": "Sv", "channel": "chan1",
                                                    "threshold": (tsv, tt, tp), "offset": offset, "r0": r0,
                                                    "r1": r1, "wtheta": wt, "wphi": wp})
    want, info = R.blackwell(sv, theta, phi, depth[0], tsv, tt, tp, offset, r0, r1, wt, wp, details=True)
    assert info["margin"] >= 1e-9  # the oracle's smoothed angles keep clear of the thresholds
    np.testing.assert_array_equal(out.values, want)
    return info


@pytest.mark.parametrize("seed,P,S,dtype,wt,wp,r0,r1", [
    (1, 300, 700, np.float64, 28, 52, 0, 1e9),      # components across 256-wide tiles on both axes
    (2, 517, 333, np.float32, 28, 52, 3.3, 150.0),  # odd sizes, crop
    (3, 40, 30, np.float64, 45, 60, 0, 1e9),        # windows larger than the crop on both axes
    (4, 1200, 300, np.float32, 9, 13, 0, 1e9),
])
def test_fuzz_against_the_oracle(seed, P, S, dtype, wt, wp, r0, r1):
    from echopype_amd import synth

    d = synth.seafloor_scene(P=P, S=S, seed=seed, dtype=dtype, band_top=int(S * 0.7), slope=-S * 0.3 / P,
                             thickness=max(3, S // 40))
    info = _run_bw(d["sv"], d["theta"], d["phi"], d["depth"], -75.0, 0.5, 0.1, 0.3, r0, r1, wt, wp)
    assert info["n_masked"] > 0


def _shape_case(fg, seeds):
    """Sv bright on ``fg``; exact angles (sums of small integers: order-free box sums) large on ``seeds``."""
    P, S = fg.shape
    sv = np.where(fg, -30.0, -90.0)
    theta = np.where(seeds, 4.0, 0.0)
    phi = np.zeros_like(theta)
    depth = np.tile(np.arange(S) * 0.25, (P, 1))
    return sv, theta, phi, depth


def test_spiral_is_one_component():
    n = 257
    fg = np.zeros((n, n), dtype=bool)
    lo, hi = 1, n - 2
    while lo <= hi:  # a square spiral of 1-pixel arms, 1 pixel apart
        fg[lo, lo:hi + 1] = True
        fg[lo:hi + 1, hi] = True
        fg[hi, lo:hi + 1] = True
        if lo + 2 <= hi:
            fg[lo + 2:hi + 1, lo] = True
            fg[lo + 2, lo:lo + 3] = True
        lo, hi = lo + 2, hi - 2
    seeds = np.zeros_like(fg)
    seeds[n // 2 - 1:n // 2 + 2, n // 2 - 1:n // 2 + 2] = True  # the seed sits in the spiral's centre
    sv, theta, phi, depth = _shape_case(fg, seeds)
    _run_bw(sv, theta, phi, depth, -75.0, 0.001, 1.0, wt=3, wp=3)


def test_checkerboard_links_only_diagonally():
    P, S = 700, 900
    fg = (np.add.outer(np.arange(P), np.arange(S)) % 2) == 0
    fg[:, :5] = False
    seeds = np.zeros_like(fg)
    seeds[P - 3:, S - 3:] = True  # one seed in a corner: every pixel of the board is reached through diagonals
    sv, theta, phi, depth = _shape_case(fg, seeds)
    info = _run_bw(sv, theta, phi, depth, -75.0, 0.001, 1.0, wt=3, wp=3)
    assert info["n_masked"] > 0


def test_whole_chain_from_ek60_samples():
    import echopype_amd as ep
    from echopype_amd import echodata, synth

    d = synth.ek60_seafloor_numpy(C=2, P=96, S=400, band_top=300)
    ed = echodata.from_ek60_arrays(d)
    ds = ep.calibrate.compute_Sv(ed)
    ds = ep.consolidate.add_depth(ds)
    for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
              "angle_offset_athwartship"):
        if k not in ds:
            ds[k] = (("channel",), d[k])
    ds = ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)
    ch = str(np.asarray(ds["channel"].values)[1])
    sv = np.asarray(ds["Sv"].values)[1]
    th = np.asarray(ds["angle_alongship"].values)[1]
    ph = np.asarray(ds["angle_athwartship"].values)[1]
    dep = np.asarray(ds["depth"].values)[1]
    prm = {"var_name": "Sv", "channel": ch, "threshold": (-70.0, 1.0137, 0.6173), "r0": 0, "r1": 1e6,
           "wtheta": 11, "wphi": 15}
    with np.errstate(invalid="ignore"):
        assert np.all(np.nanmax(np.abs(dep - dep[0]), axis=1) < 1e-16)  # one sound speed: a uniform grid
    out = ep.mask.detect_seafloor(ds, "blackwell", prm)
    want, info = R.blackwell(sv, th, ph, dep[0], -70.0, 1.0137, 0.6173, 0.3, 0, 1e6, 11, 15, details=True)
    assert info["margin"] >= 1e-9 and info["n_masked"] > 0
    np.testing.assert_array_equal(out.values, want)
    b = ep.mask.detect_seafloor(ds, "basic", {"var_name": "Sv", "channel": ch, "threshold": (-60.0, 100.0),
                                              "bin_skip_from_surface": 50})
    np.testing.assert_array_equal(b.values, R.basic(sv, dep[0], -60.0, 100.0, 50, 0.5))


def test_results_stay_on_the_device(monkeypatch):
    """Device inputs: the planes are read where they are, the bottom line stays in HBM, and the host reads only what
    the docstrings list (basic: the depth-grid flag; Blackwell: that, the mask count with the median, the union-find
    error word); torch.cuda.synchronize is never called."""
    import torch

    import echopype_amd as ep
    from echopype_amd import ops, synth
    from echopype_amd.mask.seafloor_detection import utils

    d = synth.seafloor_scene(P=200, S=300, band_top=220)
    ds = _to_dev(_lite_ds(d))
    reads, big = [], []
    real_read, real_up = utils._to_host, ops.to_device
    monkeypatch.setattr(utils, "_to_host", lambda t: (reads.append(t.numel()), real_read(t))[1])
    monkeypatch.setattr(ops, "to_device", lambda a, *k, **kw: (big.append(np.shape(a)), real_up(a, *k, **kw))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
    out = ep.mask.detect_seafloor(ds, "blackwell", {"var_name": "Sv", "channel": "chan1",
                                                    "threshold": (-75.0, 0.5, 0.1)})
    assert isinstance(out.data.tensor, torch.Tensor) and out.data.tensor.is_cuda
    assert len(reads) == 3 and reads[0] == 1 + 300 and reads[1] == 8 and reads[2] == 1
    reads.clear()
    b = ep.mask.detect_seafloor(ds, "basic", {"var_name": "Sv", "channel": "chan1", "threshold": -35.0})
    assert b.data.tensor.is_cuda and len(reads) == 1
    assert not big
    monkeypatch.undo()
    want = R.blackwell(d["sv"], d["theta"], d["phi"], d["depth"][0], -75.0, 0.5, 0.1, 0.3, 0, 500, 28, 52)
    np.testing.assert_array_equal(out.values, want)


def test_lazy_depth_from_add_depth():
    """A lazy echo_range / depth (compute_Sv + add_depth) is materialised by the check and gives the host answer."""
    import echopype_amd as ep
    from echopype_amd import echodata, synth

    d = synth.ek60_seafloor_numpy(C=1, P=30, S=350, band_top=300)
    ds = ep.consolidate.add_depth(ep.calibrate.compute_Sv(echodata.from_ek60_arrays(d)))
    prm = {"var_name": "Sv", "channel": str(np.asarray(ds["channel"].values)[0]), "threshold": (-60.0, 100.0),
           "bin_skip_from_surface": 10}
    out = ep.mask.detect_seafloor(ds, "basic", prm)
    sv, dep = np.asarray(ds["Sv"].values)[0], np.asarray(ds["depth"].values)[0]
    np.testing.assert_array_equal(out.values, R.basic(sv, dep[0], -60.0, 100.0, 10, 0.5))


def test_library_rejects_bad_arguments():
    import torch

    from echopype_amd import ops

    sv = torch.zeros((4, 8), device="cuda")
    d0 = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="bin_skip"):
        ops.seafloor_basic(sv, 8, -1.0, 1.0, d0, 0.0)
    st = ops.seafloor_state(sv.device)
    with pytest.raises(ValueError, match="crop"):
        ops.seafloor_angle_mask(sv, sv, 4, 5, 3, 3, 1.0, 1.0, st)


def test_fullsize_basic_over_2g_samples():
    """One channel of 2 M x 4096 float32 (> 2^31 samples): a known crossing per ping, none in every 5th ping."""
    import torch

    from echopype_amd import ops

    P, S, skip = 2_000_000, 4096, 200
    sv = torch.full((P, S), -120.0, dtype=torch.float32, device="cuda")
    p = torch.arange(P, device="cuda")
    k = skip + (p * 7919) % (S - skip)
    hit = (p % 5) != 0
    sv[p[hit], k[hit]] = -30.0
    sv[p[hit], k[hit] - 1] = -10.0  # above tmax: not a crossing
    depth0 = torch.arange(S, dtype=torch.float64, device="cuda") * 0.125
    out = ops.seafloor_basic(sv, skip, -50.0, -20.0, depth0, 0.5)
    want = torch.where(hit, k, torch.full_like(k, skip)).double() * 0.125 - 0.5
    assert torch.equal(out, want)
    del sv


def test_fullsize_blackwell_1m_pings():
    """1 x 1 000 000 x 2500 float32: a band of exact angles whose top moves by one sample at a time; the median
    under the mask is the background, below tSv, so the line is the band's top by construction."""
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    P, S, T = 1_000_000, 2500, 6
    p = torch.arange(P, device="cuda")
    top = 1500 + ((p // 1000) % 400) - 200 * ((p // 400_000) % 2)
    sv = torch.full((1, P, S), -90.0, dtype=torch.float32, device="cuda")
    theta = torch.zeros((1, P, S), dtype=torch.float32, device="cuda")
    for j in range(T):
        sv[0, p, top + j] = -25.0
        theta[0, p, top + j] = 8.0
    phi = torch.zeros_like(theta)
    depth = (torch.arange(S, dtype=torch.float32, device="cuda") * 0.25).expand(1, P, S).contiguous()
    dims = ("channel", "ping_time", "range_sample")
    ds = Dataset(coords={"channel": np.array(["c"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    for k, t in (("Sv", sv), ("angle_alongship", theta), ("angle_athwartship", phi), ("depth", depth)):
        ds[k] = DataArray(DeviceArray(t), dims, name=k)
    out = ep.mask.detect_seafloor(ds, "blackwell", {"var_name": "Sv", "channel": "c", "r1": 1e6,
                                                    "threshold": (-75.0, 0.3001, 0.5)})
    want = top.float() * 0.25 - 0.3
    assert torch.equal(out.data.tensor, want)
