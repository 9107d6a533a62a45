"""clean.detect_transient on the host (no GPU): the reference's signatures, its checks and their messages, the
dispatcher, and tests/transient_ref.py (the NumPy oracle of the GPU tests) pinned to the reference-executed goldens
(scripts/gen_transient_goldens.py) bit for bit, decision margins included."""
import inspect
import json
import os

import numpy as np
import pytest

import transient_ref as R


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _case(g, tag):
    return next(c for c in R.cases(g) if c["tag"] == tag)


def _mask(g, tag):
    c = _case(g, tag)
    return R.unpack_mask(g, tag, c["shape"])


def test_signatures_equal_the_reference(g):
    import echopype_amd as ep
    from echopype_amd.clean.transient_noise import transient_noise_fielding, transient_noise_matecho

    ref = json.loads(g["signatures"].item())
    for name, fn in (("detect_transient", ep.clean.detect_transient),
                     ("transient_noise_fielding", transient_noise_fielding),
                     ("transient_noise_matecho", transient_noise_matecho)):
        got = [[p.name, "positional_or_keyword", None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        extra = [p for p in inspect.signature(fn).parameters.values() if p.kind != p.POSITIONAL_OR_KEYWORD]
        assert got == ref[name]["params"], name
        assert all(p.kind == p.KEYWORD_ONLY and p.default is None for p in extra), name


def test_registry_and_exports():
    import echopype_amd as ep
    from echopype_amd.clean.transient_noise import transient_noise_fielding, transient_noise_matecho

    assert ep.clean.METHODS_TRANSIENT == {"fielding": transient_noise_fielding, "matecho": transient_noise_matecho}
    assert "detect_transient" in ep.clean.__all__ and "METHODS_TRANSIENT" in ep.clean.__all__
    assert "mask_transient_noise" in ep.clean.__all__ and "remove_background_noise" in ep.clean.__all__


@pytest.mark.parametrize("tag", ["x_method", "x_f_var_name", "x_f_range_var", "x_f_cannot_infer", "x_m_var_name",
                                 "x_m_range_var", "x_m_time_var"])
def test_host_checks_raise_the_reference_error(g, tag):
    """The checks that precede any device work: same type and message as the reference."""
    import echopype_amd as ep

    c = _case(g, tag)
    typ, msg = c["error"]
    with pytest.raises(Exception) as ei:
        ep.clean.detect_transient(R.case_dataset(g, c), c["method"], R.case_params(c))
    assert type(ei.value).__name__ == typ
    assert str(ei.value) == msg


def test_what_the_device_cannot_take_is_refused_before_any_launch(g):
    from echopype_amd.clean.transient_noise.transient_fielding import _layer_rows, transient_noise_fielding
    from echopype_amd.clean.transient_noise.transient_matecho import _window_rows, transient_noise_matecho

    r = 2.5 * np.arange(40)
    with pytest.raises(NotImplementedError, match="range_var='depth' must be nondecreasing"):
        _window_rows(np.r_[r[:10], r[8], r[11:]], 20.0, 50.0, "depth")
    with pytest.raises(NotImplementedError, match="range_var='depth' has NaN between"):
        _window_rows(np.r_[r[:10], np.nan, r[11:]], 20.0, 50.0, "depth")
    assert _window_rows(np.r_[r[:30], [np.nan] * 10], 20.0, 50.0, "depth")[:2] == (8, 29)
    assert _window_rows(r, 500.0, 50.0, "depth")[:2] == (0, 0)
    # the Fielding expressions are the reference's own: they raise what it raises (the fixture has both)
    for tag, row in (("x_f_dr_zero", np.full(40, 50.0)), ("x_f_dr_nan", np.where(np.arange(39) % 2, np.nan, r[:39]))):
        typ, msg = _case(g, tag)["error"]
        with pytest.raises(Exception) as ei:
            _layer_rows(row, 40.0, 60.0, 10.0, 5.0)
        assert (type(ei.value).__name__, str(ei.value)) == (typ, msg)
    assert _layer_rows(r, 60.0, 40.0, 10.0, 5.0) is None and _layer_rows(r, 200.0, 300.0, 10.0, 5.0) is None
    assert _layer_rows(r, 50.0, 75.0, 10.0, 5.0) == (20, 30, 4, 2)
    # start > 0: refused (the reference fails for both shapes: the fixture records how)
    c = _case(g, "f_basic")
    with pytest.raises(NotImplementedError, match="start > 0"):
        transient_noise_fielding(R.case_dataset(g, c), **dict(R.case_params(c), start=4))
    st = json.loads(g["fielding_start"].item())
    assert st["tall"]["S"] > st["tall"]["P"] - st["tall"]["start"] and st["tall"]["error"][0] == "ValueError"
    assert st["wide"]["S"] <= st["wide"]["P"] - st["wide"]["start"]
    assert st["wide"]["rows"] == st["wide"]["P"] + st["wide"]["start"]
    # time_var: another dimension of Sv than the ping axis is not supported
    with pytest.raises(NotImplementedError, match="time_var='channel'"):
        transient_noise_matecho(R.case_dataset(g, _case(g, "m_basic")), time_var="channel")
    # window_ping = 1: an empty ping window -- np.min of nothing, in the reference and here
    c = _case(g, "m_window_ping_1")
    assert c["error"] == ["ValueError", "zero-size array to reduction operation minimum which has no identity"]


def test_oracle_matches_the_reference_goldens(g):
    """tests/transient_ref.py reproduces every golden mask and every margin, to the bit."""
    n = 0
    for c in R.cases(g):
        if "error" in c:
            continue
        want = R.unpack_mask(g, c["tag"], c["shape"])
        got, margin = R.case_oracle(g, c)
        assert got.dtype == np.bool_ and got.shape == want.shape, c["tag"]
        np.testing.assert_array_equal(got, want, err_msg=c["tag"])
        assert int((~want).sum()) == c["masked"], c["tag"]
        ref = g[c["tag"] + "_margin"]
        assert margin.shape == ref.shape and margin.tobytes() == ref.tobytes(), \
            (c["tag"], float(np.nanmax(np.abs(np.where(np.isfinite(ref), margin - ref, 0.0)))))
        n += 1
    assert n >= 45


def test_no_fixture_ping_is_closer_to_a_threshold_than_the_margin(g):
    for c in R.cases(g):
        if "error" in c:
            continue
        m = g[c["tag"] + "_margin"]
        assert (m >= R.MARGIN[c["dtype"]]).all(), c["tag"]


def test_goldens_cover_the_issue_cases(g):
    cs = {c["tag"]: c for c in R.cases(g)}
    for t in ("f_basic", "f_basic_f32", "f_odd_layer", "f_n0", "f_n1", "f_range_1d", "f_up_ge_lw", "f_r0_gt_r1",
              "f_below_data", "f_above_data", "f_nan_tail", "f_allnan_layer_and_ping", "f_p75_across_maxts",
              "f_negative_start", "f_step_beyond_column", "f_three_channels", "f_three_channels_f32", "m_basic",
              "m_basic_f32", "m_extend", "m_extend_f32", "m_odd_window", "m_window_ping_1", "m_window_ping_2",
              "m_bottom_cuts", "m_bottom_removes", "m_bottom_min_window", "m_bottom_nan", "m_bottom_slope",
              "m_bottom_per_channel", "m_bottom_per_channel_f32", "m_three_channels", "m_three_channels_f32",
              "m_window_outside", "m_nan_tail", "m_nan_tail_bottom", "m_allnan_ping", "m_f32_start_limit",
              "m_f32_bottom_limit", "x_f_dr_zero", "x_f_dr_nan", "f_p75_across_maxts_f32", "f_p75_across_maxts_7",
              "m_small_window_t75", "m_small_window_t75_f32", "m_small_window_t18", "m_small_window_t18_f32",
              "x_m_percentile", "m_percentile_unreached"):
        assert t in cs, t
    # ---- fielding: rows [120, 140) of a 2.5 m grid, n = 5, 40 pings, steps of 5 rows, stop row 20
    m = _mask(g, "f_basic")[0]
    flagged = np.flatnonzero(~m.all(axis=1))
    np.testing.assert_array_equal(flagged, [5, 12, 20, 27, 30, 34])  # 3 and 37 are raised too, within n of the ends
    assert 5 - 5 == 0 and 34 + 5 == 40 - 1                            # ... 5 and 34 are the first / last computable
    first = {int(j): int(np.argmin(m[j])) for j in flagged}           # first masked row
    assert all(not m[j, first[j]:].any() and m[j, :first[j]].all() for j in flagged)
    assert first[27] == 110   # raised from row 120 = up: the first window [115, 120) stops the walk, mask one step above
    assert first[30] == 20    # raised from row 10 < rmin = 20: the walk runs out at rmin (last window [25, 30))
    assert first[20] in (85, 90, 95)  # raised from row 100: stops in the first window above it
    assert np.isnan(g[cs["f_basic"]["sv"]]).mean() > 0.005
    assert cs["f_odd_layer"]["params"]["r1"] == 347.5  # lw = 139: 19 samples (odd), f_basic has 20 (even)
    for t in ("f_n0", "f_up_ge_lw", "f_r0_gt_r1", "f_below_data", "f_above_data", "f_nan_tail", "f_defaults_no_layer"):
        assert cs[t]["masked"] == 0, t
    assert np.isnan(g[cs["f_nan_tail"]["rows"]][0, -1])
    assert cs["f_n1"]["masked_pings"] == 8  # n = 1: pings 3 and 37 are computable as well
    # an all-NaN layer makes a raised ping uncomputable; an all-NaN ping inside a block does not stop its neighbour
    h = _mask(g, "f_allnan_layer_and_ping")[0]
    assert h[12].all() and h[19].all() and not h[20].all() and cs["f_allnan_layer_and_ping"]["masked_pings"] == 5
    # the negative-start walk: up = 360, sf = 380 -> r0_ = -20: exactly the last 20 samples of the flagged pings
    ng = _mask(g, "f_negative_start")[0]
    assert cs["f_negative_start"]["masked_pings"] == 2 and cs["f_negative_start"]["masked"] == 2 * 20
    assert all((~ng[j]).sum() in (0, 20) and ng[j, :380].all() for j in range(ng.shape[0]))
    assert cs["f_step_beyond_column"]["masked"] == 2 * 400  # r0_ < -S: the whole column
    t3 = _mask(g, "f_three_channels")
    rows3 = g[cs["f_three_channels"]["rows"]]
    assert len({tuple(r) for r in rows3}) == 3 and all((~t3[c]).any() for c in range(3))
    # ---- matecho: rows [40, 120] of the same grid, 10-ping windows; pings 0, 7, 20, 39 raised by 9 dB and more
    mm = _mask(g, "m_basic")[0]
    np.testing.assert_array_equal(np.flatnonzero(~mm.all(axis=1)), [0, 7, 20, 39])
    assert all(not mm[j].any() for j in (0, 7, 20, 39))  # whole columns, both ends of the axis
    me = _mask(g, "m_extend")[0]
    np.testing.assert_array_equal(np.flatnonzero(~me.all(axis=1)), [0, 1, 2, 5, 6, 7, 8, 9, 18, 19, 20, 21, 22, 37, 38, 39])
    assert cs["m_bottom_cuts"]["masked_pings"] == 4 and cs["m_bottom_cuts"]["min_margin"] != cs["m_basic"]["min_margin"]
    assert cs["m_bottom_removes"]["masked"] == 0 and cs["m_bottom_removes"]["min_margin"] is None
    assert cs["m_bottom_min_window"]["masked"] == 0 and cs["m_bottom_min_window"]["min_margin"] == 10.0  # H = 4 x 2.5 m
    assert np.isnan(g[cs["m_bottom_nan"]["bottom"]]).any() and cs["m_bottom_nan"]["masked_pings"] == 4
    assert cs["m_bottom_per_channel"]["bottom_dims"] == ["channel", "ping_time"]
    assert cs["m_nan_tail"]["masked"] == 0 and cs["m_nan_tail_bottom"]["masked_pings"] == 4  # r[-1] = NaN is the bottom
    assert cs["m_window_outside"]["masked"] == 0
    assert cs["m_allnan_ping"]["masked_pings"] == 3  # ping 7 is all NaN: its mean is NaN, it is never flagged
    assert cs["m_window_ping_2"]["masked_pings"] == 3  # h = 1: ping 0 has only itself ... ping 39 too
    assert os.path.getsize(R.GOLDEN_PATH) < 512 * 1024


@pytest.mark.parametrize("tag", ["m_small_window_t75", "m_small_window_t75_f32", "m_small_window_t18",
                                 "m_small_window_t18_f32"])
def test_small_window_cases_are_decided_by_the_percentile_itself(g, tag):
    """The device settles most pings by counting; these cases hold pings whose threshold lies BETWEEN the two ranks
    the percentile interpolates (count == k + 1), where the selection and the dB interpolation decide -- with both
    outcomes, and with the interpolation weight on the side the name says.  Asserted from the oracle's replay of the
    device's counting sweep, so the cases cannot silently stop covering that branch."""
    c = _case(g, tag)
    sv, rows, _ = R.case_arrays(g, c)
    p = R.case_params(c)
    route, frac = R.matecho_route(sv[0], rows[0], **{k: v for k, v in p.items() if k not in ("var_name", "range_var")})
    sel = route == 3
    np.testing.assert_array_equal(np.flatnonzero(sel), c["select_pings"])
    flagged = ~_mask(g, tag)[0].all(axis=1)
    assert (sel & flagged).sum() >= 2 and (sel & ~flagged).sum() >= 2
    assert (route == 1).any() and (route == 2).any()  # ... and pings the count alone settles, both ways
    inner = sel.copy()
    inner[:2] = inner[-2:] = False  # (a full 4-ping window)
    want_high = tag.startswith("m_small_window_t75")
    # (a NaN in a window changes its count and with it the weight: most, not all, have the weight of the name)
    assert inner.sum() >= 3 and ((frac[inner] >= 0.5) == want_high).sum() >= 3
    assert g[tag + "_margin"][0][sel].min() >= 10 * R.MARGIN[c["dtype"]]


@pytest.mark.parametrize("tag,count", [("f_p75_across_maxts", 6), ("f_p75_across_maxts_f32", 6),
                                       ("f_p75_across_maxts_7", 7), ("f_p75_across_maxts_7_f32", 7)])
def test_p75_cases_are_decided_by_the_interpolation(g, tag, count):
    """A layer of 6 / 7 samples: the 75th percentile interpolates between two of them, and maxts lies between those two
    for raised pings that pass thr[0] -- some kept by maxts, some flagged."""
    c = _case(g, tag)
    sv, rows, _ = R.case_arrays(g, c)
    p = R.case_params(c)
    kw = {k: p[k] for k in ("r0", "r1", "n", "thr", "roff", "jumps", "maxts")}
    br, cnt = R.fielding_p75_bracket(sv[0], rows[0], **kw)
    assert (cnt == count).all()
    loud = ~R.fielding(sv[0], rows[0], **dict(kw, maxts=0.0))[0].all(axis=1)
    np.testing.assert_array_equal(np.flatnonzero(br & loud), c["bracket_pings"])
    flagged = ~_mask(g, tag)[0].all(axis=1)
    assert (br & loud & flagged).any() and (br & loud & ~flagged).any()


def test_percentile_outside_0_100(g):
    """np.percentile raises when a ping reaches it; with no ping that far the reference returns all-True, where this
    package refuses the argument before any launch (recorded as a divergence in the fixture and in DESIGN)."""
    import echopype_amd as ep

    assert _case(g, "x_m_percentile")["error"] == ["ValueError", "Percentiles must be in the range [0, 100]"]
    c = _case(g, "m_percentile_unreached")
    assert c["masked"] == 0 and c["diverges"] == ["ValueError", "Percentiles must be in the range [0, 100]"]
    with pytest.raises(ValueError, match="Percentiles must be in the range"):
        ep.clean.detect_transient(R.case_dataset(g, c), "matecho", R.case_params(c))


def test_float32_limits_are_compared_as_numpy_compares_them(g):
    """A Python float against a float32 row is rounded to float32 first (start_depth a hair above a sample includes
    it); the bottom is an np.float64 scalar and is compared in float64 (a bottom a hair above a sample keeps it)."""
    c = _case(g, "m_f32_start_limit")
    r = g[c["rows"]][0]
    lim = c["params"]["start_depth"]
    assert r.dtype == np.float32 and float(r[40]) < lim and np.float32(lim) == r[40]
    assert (r >= lim)[40] and not (r.astype(np.float64) >= lim)[40]
    assert c["masked_pings"] == 4  # flagged only because sample 40 counts: without it the window is below min_window
    n_with = int(((r >= lim) & (r <= lim + c["params"]["window_meter"])).sum())
    dz = float(r[1] - r[0])
    assert dz * (n_with - 1) < c["params"]["min_window"] < dz * n_with
    c = _case(g, "m_f32_bottom_limit")
    b = np.float64(g[c["bottom"]][0])
    assert (r < b)[100] and not (r < float(b))[100]
    assert c["masked_pings"] == 4 and dz * 60 < c["params"]["min_window"] < dz * 61


def test_fuzz_cases_stay_within_the_cap_on_left_out_pings():
    """The GPU fuzz test may leave out the pings closer than MARGIN to a threshold: at most 1 % of a case's pings, or 2
    where that is more -- a condition on the seeded inputs, asserted here from the oracle's margins.  Every case flags
    some ping and leaves some alone."""
    seen = set()
    for case in R.fuzz_cases():
        valid, margin, compare = R.fuzz_expected(case)
        tag, method, dt, C, P, S = case[:6]
        assert P >= 80 and 1 <= C <= 3
        left = int((~compare).sum())
        print(tag, method, dt, (C, P, S), "left out", left, "smallest margin", float(margin.min()))
        assert left <= max(2, (C * P) // 100), tag
        flagged = ~valid.all(axis=2)
        assert flagged[compare].any() and not flagged[compare].all(), tag
        seen.add((method, dt))
    assert len(seen) == 4


def test_scene_generator():
    from echopype_amd import synth

    sc = synth.transient_scene(P=120, S=200, seed=5, dtype=np.float32)
    sv = sc["Sv"]
    assert sv.shape == (120, 200) and sv.dtype == np.float32 and sc["depth"].dtype == np.float32
    assert 0.005 < np.isnan(sv).mean() < 0.05
    assert sc["bottom"].shape == (120,) and sc["bottom"][0] < sc["bottom"][-1] < sc["depth"][-1]
    assert len(sc["pings"]) == 6 and len(set(sc["tops"])) > 1
    j, t = int(sc["pings"][0]), int(sc["tops"][0])
    quiet = np.setdiff1d(np.arange(120), sc["pings"])
    assert np.nanmedian(sv[j, t:150]) > np.nanmedian(sv[quiet][:, t:150]) + 4.0
    np.testing.assert_array_equal(sv, synth.transient_scene(P=120, S=200, seed=5, dtype=np.float32)["Sv"])
