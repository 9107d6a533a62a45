"""mask.detect_seafloor on the host (no GPU): the reference's signatures, its checks and their messages, the threshold
parsers, the dispatcher, and tests/seafloor_ref.py (the NumPy oracle of the GPU fuzz tests) pinned to the
reference-executed goldens (scripts/gen_seafloor_goldens.py)."""
import inspect
import json

import numpy as np
import pytest

import seafloor_ref as R


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _cases(g):
    return json.loads(g["cases"].item())


def _inputs(g, c):
    return {k: g[v] for k, v in c["inputs"].items()}


def _lite_ds(inp, var="Sv", with_channel=True, with_depth=True, channel="chan1"):
    from echopype_amd.xr_lite import Dataset

    P, S = inp["sv"].shape
    coords = {"ping_time": np.arange(P), "range_sample": np.arange(S)}
    if with_channel:
        coords["channel"] = np.array([channel])
    ds = Dataset(coords=coords)
    dims = ("channel", "ping_time", "range_sample")
    ds[var] = (dims, inp["sv"][None])
    if with_depth:
        ds["depth"] = (dims, inp["depth"][None])
    for k, name in (("theta", "angle_alongship"), ("phi", "angle_athwartship")):
        if k in inp:
            ds[name] = (dims, inp[k][None])
    return ds


def test_signatures_equal_the_reference(g):
    import echopype_amd as ep
    from echopype_amd.mask.seafloor_detection import bottom_basic, bottom_blackwell

    ref = json.loads(g["signatures"].item())
    for name, fn in (("detect_seafloor", ep.mask.detect_seafloor), ("bottom_basic", bottom_basic),
                     ("bottom_blackwell", bottom_blackwell)):
        got = [[p.name, "positional_or_keyword", None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        extra = [p for p in inspect.signature(fn).parameters.values() if p.kind != p.POSITIONAL_OR_KEYWORD]
        assert got == ref[name]["params"], name
        assert all(p.kind == p.KEYWORD_ONLY and p.default is None for p in extra), name


def test_registry_and_exports():
    import echopype_amd as ep
    from echopype_amd.mask.seafloor_detection import bottom_basic, bottom_blackwell

    assert ep.mask.METHODS_BOTTOM == {"basic": bottom_basic, "blackwell": bottom_blackwell}
    assert "detect_seafloor" in ep.mask.__all__


def test_unknown_method_raises():
    import echopype_amd as ep

    with pytest.raises(ValueError, match="^Unsupported bottom detection method: otsu$"):
        ep.mask.detect_seafloor(None, "otsu", {})


@pytest.mark.parametrize("tag", ["e_var_name", "e_no_depth", "e_no_channel", "e_no_angles", "e_bw_var_name"])
def test_host_checks_raise_the_reference_error(g, tag):
    """The checks that precede any device work: same type and message as the reference, in its order."""
    import echopype_amd as ep

    c = next(c for c in _cases(g) if c["tag"] == tag)
    ds = _lite_ds(_inputs(g, c), **c["flags"])
    typ, msg = c["error"]
    with pytest.raises(Exception) as ei:
        ep.mask.detect_seafloor(ds, c["method"], c["params"])
    assert type(ei.value).__name__ == typ
    assert str(ei.value) == msg


def test_missing_channel_label_is_a_key_error(g):
    import echopype_amd as ep

    c = next(c for c in _cases(g) if c["tag"] == "e_tmax")
    with pytest.raises(KeyError):
        ep.mask.detect_seafloor(_lite_ds(_inputs(g, c)), "basic", {"var_name": "Sv", "channel": "nope"})


def test_threshold_parsers(g):
    from echopype_amd.mask.seafloor_detection.utils import _parse_blackwell_thresholds, _validate_threshold

    assert _validate_threshold(-50) == (-50.0, -40.0)
    assert _validate_threshold(-50.5) == (-50.5, -40.5)
    assert _validate_threshold((-60, -20)) == (-60.0, -20.0)
    assert _validate_threshold([-60.0, -20.0]) == (-60.0, -20.0)
    for bad in ((-20, -50), (-20, -20)):
        with pytest.raises(ValueError, match="^threshold upper bound must be > lower bound$"):
            _validate_threshold(bad)
    assert _parse_blackwell_thresholds(-75) == (-75.0, 702.0, 282.0)
    assert _parse_blackwell_thresholds(-75.5) == (-75.5, 702.0, 282.0)
    assert _parse_blackwell_thresholds((-60, 0.01)) == (-60.0, 702.0, 282.0)  # the second value is dropped
    assert _parse_blackwell_thresholds([-60, 1, 2]) == (-60.0, 1.0, 2.0)
    with pytest.raises(ValueError, match="^`threshold` must have 1, 2, or 3 values$"):
        _parse_blackwell_thresholds([1, 2, 3, 4])
    with pytest.raises(ValueError):
        _parse_blackwell_thresholds([-75])
    with pytest.raises(TypeError, match="must be float or tuple/list of 1–3 floats"):
        _parse_blackwell_thresholds("x")
    # the messages the goldens recorded from the reference
    msgs = {c["tag"]: c["error"] for c in _cases(g) if "error" in c}
    assert msgs["e_thr_len"] == ["ValueError", "`threshold` must have 1, 2, or 3 values"]
    assert msgs["e_thr_type"][0] == "TypeError"
    assert msgs["e_tmax"] == ["ValueError", "threshold upper bound must be > lower bound"]


def test_oracle_matches_the_reference_goldens(g):
    """tests/seafloor_ref.py reproduces every golden bottom line bit for bit, with every smoothed angle square at
    least 1e-9 (relative) away from its threshold -- the margin the GPU comparisons rely on."""
    n = 0
    for c in _cases(g):
        if "error" in c:
            continue
        inp, p = _inputs(g, c), c["params"]
        want = g[f"{c['tag']}_out"]
        if c["method"] == "basic":
            thr = p.get("threshold", -50.0)
            tmin, tmax = (float(thr), float(thr) + 10.0) if np.ndim(thr) == 0 else map(float, thr)
            got = R.basic(inp["sv"], inp["depth"][0], tmin, tmax, p.get("bin_skip_from_surface", 200),
                          p.get("offset_m", 0.5))
        else:
            thr = p.get("threshold", -75)
            tsv, tt, tp = (thr, 702.0, 282.0) if np.ndim(thr) == 0 else (
                (thr[0], 702.0, 282.0) if len(thr) == 2 else thr)
            got, info = R.blackwell(inp["sv"], inp["theta"], inp["phi"], inp["depth"][0], tsv, tt, tp,
                                    p.get("offset", 0.3), p.get("r0", 0), p.get("r1", 500), p.get("wtheta", 28),
                                    p.get("wphi", 52), details=True)
            assert info["margin"] >= 1e-9, c["tag"]
        assert got.dtype == want.dtype, c["tag"]
        np.testing.assert_array_equal(got, want, err_msg=c["tag"])
        n += 1
    assert n >= 20


def test_goldens_cover_the_issue_cases(g):
    tags = {c["tag"] for c in _cases(g)}
    for t in ("b_unit_band", "b_unit_none", "b_scalar", "k_tuple2", "k_no_detection", "k_below_tsv",
              "k_allnan_median", "k_even_count", "k_empty_mask", "k_small_crop", "k_f32", "e_depth_varies",
              "e_depth_allnan_ping", "b_depth_nan_ping0", "b_depth_nan_later", "e_skip"):
        assert t in tags


def test_box_mean_is_convolve2d():
    from scipy.signal import convolve2d

    rng = np.random.default_rng(3)
    for shape, w in (((30, 40), 5), ((7, 9), 28), ((3, 2), 8), ((20, 20), 1), ((11, 6), 4)):
        x = rng.normal(size=shape)
        x[rng.random(shape) < 0.02] = np.nan
        want = convolve2d(x, np.ones((w, w)) / w ** 2, "same", boundary="symm")
        got = R.box_mean(x, w)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        f = ~np.isnan(want)
        assert np.all(np.abs(got[f] - want[f]) <= 1e-12)


def test_scene_generators():
    from echopype_amd import synth

    d = synth.seafloor_scene(P=60, S=90, band_top=60)
    assert d["sv"].shape == d["theta"].shape == d["depth"].shape == (60, 90)
    assert np.isnan(d["sv"]).any() and not np.isnan(d["depth"]).any()
    e = synth.ek60_seafloor_numpy(C=1, P=12, S=200, band_top=150)
    assert e["angle_alongship"].dtype == np.int8 and (e["angle_alongship"][0, 0, 150:158] == 40).all()
