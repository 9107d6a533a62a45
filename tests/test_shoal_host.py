"""mask.detect_shoal on the host (no GPU): the reference's signatures, its checks and their messages, the dispatcher,
and tests/shoal_ref.py (the NumPy / scipy oracle of the GPU fuzz tests) pinned to the reference-executed goldens
(scripts/gen_shoal_goldens.py)."""
import inspect
import json
import os

import numpy as np
import pytest

import shoal_ref as R

DIMS = ("channel", "ping_time", "range_sample")


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _cases(g):
    return json.loads(g["cases"].item())


def _params(g, c):
    """The keyword arguments of a case as the reference got them (idim / jdim arrays, tuples for the sizes)."""
    p = dict(c["params"])
    for k in ("idim", "jdim"):
        if k in c:
            p[k] = g[c[k]]
    for k in ("mincan", "maxlink", "minsho"):
        if k in p:
            p[k] = tuple(p[k])
    return p


def _lite_ds(sv, layout="cps", channel="chan1", var="Sv"):
    from echopype_amd.xr_lite import Dataset

    P, S = sv.shape
    ds = Dataset(coords={"channel": np.array([channel]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    dims = {"cps": DIMS, "ps": DIMS[1:], "p": ("channel", "ping_time", "beam"),
            "s": ("channel", "beam", "range_sample")}[layout]
    ds[var] = (dims, sv if layout == "ps" else sv[None])
    return ds


def _oracle(g, c):
    p, sv = _params(g, c), g[c["sv"]]
    kw = {k: v for k, v in p.items() if k not in ("var_name", "channel")}
    return R.weill(sv, **kw) if c["method"] == "weill" else R.echoview(sv, **kw)


def test_signatures_equal_the_reference(g):
    import echopype_amd as ep
    from echopype_amd.mask.shoal_detection import shoal_echoview, shoal_weill

    ref = json.loads(g["signatures"].item())
    for name, fn in (("detect_shoal", ep.mask.detect_shoal), ("shoal_weill", shoal_weill),
                     ("shoal_echoview", shoal_echoview)):
        got = [[p.name, "positional_or_keyword", None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        extra = [p for p in inspect.signature(fn).parameters.values() if p.kind != p.POSITIONAL_OR_KEYWORD]
        assert got == ref[name]["params"], name
        assert all(p.kind == p.KEYWORD_ONLY and p.default is None for p in extra), name


def test_registry_and_exports():
    import echopype_amd as ep
    from echopype_amd.mask.shoal_detection import shoal_echoview, shoal_weill

    assert ep.mask.METHODS_SHOAL == {"echoview": shoal_echoview, "weill": shoal_weill}
    assert "detect_shoal" in ep.mask.__all__ and "METHODS_SHOAL" in ep.mask.__all__
    assert "detect_seafloor" in ep.mask.__all__ and "apply_mask" in ep.mask.__all__


@pytest.mark.parametrize("tag", ["x_method", "x_w_var_name", "x_w_channel_none", "x_w_no_ping_time",
                                 "x_w_no_range_sample", "x_e_var_name", "x_e_channel_none", "x_e_idim_nan",
                                 "x_e_jdim_nan"])
def test_host_checks_raise_the_reference_error(g, tag):
    """The checks that precede any device work: same type and message as the reference."""
    import echopype_amd as ep

    c = next(c for c in _cases(g) if c["tag"] == tag)
    typ, msg = c["error"]
    with pytest.raises(Exception) as ei:
        ep.mask.detect_shoal(_lite_ds(g[c["sv"]], c["layout"]), c["method"], _params(g, c))
    assert type(ei.value).__name__ == typ
    assert str(ei.value) == msg


def test_axes_that_the_device_search_cannot_take():
    from echopype_amd.mask.shoal_detection.shoal_echoview import _axis

    np.testing.assert_array_equal(_axis([0, 1, 1, 2.5], "idim", 4), [0.0, 1.0, 1.0, 2.5])
    assert _axis(np.arange(9, dtype=np.int32), "jdim", 5).dtype == np.float64  # longer than needed is allowed
    with pytest.raises(NotImplementedError, match="idim must be nondecreasing"):
        _axis([0.0, 2.0, 1.0], "idim", 3)
    with pytest.raises(NotImplementedError, match="jdim with infinite entries"):
        _axis([0.0, 1.0, np.inf], "jdim", 3)
    with pytest.raises(IndexError, match="idim has 3 entries"):
        _axis([0.0, 1.0, 2.0], "idim", 4)


def test_oracle_matches_the_reference_goldens(g):
    """tests/shoal_ref.py reproduces every golden mask of both methods."""
    n = 0
    for c in _cases(g):
        if "error" in c:
            continue
        want = R.unpack_mask(g, c["tag"], c["shape"])
        got = _oracle(g, c)
        assert got.dtype == np.bool_ and got.shape == want.shape, c["tag"]
        assert int(want.sum()) == c["count"], c["tag"]
        np.testing.assert_array_equal(got, want, err_msg=c["tag"])
        n += 1
    assert n >= 60


def test_oracle_gap_filling_by_hand():
    m = np.array([[1, 0, 0, 1, 0, 0, 0, 1, 0]], dtype=bool)
    np.testing.assert_array_equal(R.fill_gaps(m, 2, 1)[0], [1, 1, 1, 1, 0, 0, 0, 1, 0])
    np.testing.assert_array_equal(R.fill_gaps(m, 3, 1)[0], [1, 1, 1, 1, 1, 1, 1, 1, 0])
    np.testing.assert_array_equal(R.fill_gaps(m, 0, 1)[0], m[0])
    np.testing.assert_array_equal(R.fill_gaps(m.T, 2, 0)[:, 0], [1, 1, 1, 1, 0, 0, 0, 1, 0])


def test_goldens_cover_the_issue_cases(g):
    cases = {c["tag"]: c for c in _cases(g)}
    for t in ("w_default", "w_default_f32", "w_zeros", "w_all", "w_vgap_3", "w_vgap_4", "w_vgap_5", "w_hgap_2",
              "w_hgap_3", "w_hgap_4", "w_borders", "w_none", "w_full", "w_allnan", "w_one_ping", "w_one_sample",
              "w_thr_f32", "w_thr_f64", "w_no_channel_dim", "w_checker", "w_long_139", "e_default", "e_default_f32",
              "e_zeros", "e_irregular", "e_irregular_f32", "e_repeated_jdim", "e_repeated_jdim_neg",
              "e_maxlink_-1.0_-1.0", "e_maxlink_0.0_0.0", "e_three_short", "e_three_chain", "e_three_direct",
              "e_ell_bbox_only", "e_ell_linked", "e_ring_linked", "e_tie", "e_tie_wider", "e_checker", "e_none",
              "e_full", "e_one_ping", "e_one_sample", "e_no_channel_dim"):
        assert t in cases, t
    # the cases say what their names promise
    assert cases["w_vgap_3"]["count"] < cases["w_vgap_4"]["count"]      # a gap of 4 samples: filled from maxvgap = 4
    assert cases["w_hgap_2"]["count"] < cases["w_hgap_3"]["count"] == cases["w_hgap_4"]["count"]  # a gap of 3 pings
    assert cases["e_three_short"]["count"] == 0 and cases["e_three_chain"]["count"] == 12  # chained through the middle
    assert cases["e_ell_bbox_only"]["count"] == 0 and cases["e_ell_linked"]["count"] == 50  # boxes that overlap: no link
    assert cases["e_tie"]["count"] == 0 and cases["e_tie_wider"]["count"] == 12
    assert cases["e_checker"]["count"] == 50 and cases["w_checker"]["count"] == 0
    assert cases["w_thr_f32"]["count"] == 9 and cases["w_thr_f64"]["count"] == 9
    assert np.isnan(g[cases["w_default"]["sv"]]).mean() > 0.01
    # an untouched component that the reference keeps whatever its size (negative maxlink): the oracle sees some
    c = cases["e_maxlink_-3.0_-2.0"]
    kw = {k: v for k, v in _params(g, c).items() if k not in ("var_name", "channel")}
    assert R.echoview(g[c["sv"]], details=True, **kw)[1]["untouched"] > 0
    assert os.path.getsize(R.GOLDEN_PATH) < 512 * 1024


def test_threshold_is_compared_in_float64(g):
    """np.ma.masked_greater hands the threshold over as a float64 array: a float32 sample equal to float32(-70.1)
    lies above -70.1, and the reference marks it (the golden has 3 of 5 samples per ping, not 2)."""
    c = next(c for c in _cases(g) if c["tag"] == "w_thr_f32")
    sv = g[c["sv"]]
    assert sv.dtype == np.float32 and sv[0, 1] == np.float32(-70.1)
    np.testing.assert_array_equal(R.threshold(sv, -70.1)[0], [False, True, True, False, True])
    np.testing.assert_array_equal(R.unpack_mask(g, "w_thr_f32", c["shape"])[0], [False, True, True, False, True])
    np.testing.assert_array_equal(R.threshold(sv.astype(np.float64), -70.1)[0], [False, True, True, False, True])


def test_scene_generator():
    from echopype_amd import synth

    sv = synth.shoal_scene(P=60, S=90, seed=5, dtype=np.float32)
    assert sv.shape == (60, 90) and sv.dtype == np.float32 and np.isnan(sv).any()
    frac = np.nanmean(sv > -70.0)
    assert 0.02 < frac < 0.6
    np.testing.assert_array_equal(sv, synth.shoal_scene(P=60, S=90, seed=5, dtype=np.float32))
