"""targets.track_targets without a GPU: the NumPy restatement tests/track_ref.py against answers worked out by hand;
on the restatement alone, that every table of tests/track_cases.py keeps its decisions away from the edge (so that the
GPU test may ask for equal integers); parameter and table validation before any device work; the exports."""
import os
import re

import numpy as np
import pytest
import track_cases as K
import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against answers worked out by hand ----------------------------------------------------------------
def test_two_crossing_fish():
    """Rows alternate between fish a (on the axis) and fish b (1 degree alongship: 0.17 m beside it, outside the gate of
    0.1 m): their ranges cross between pings 2 and 3, and each stays its own track of six."""
    out = K.expected("crossing")
    assert out["track_id"].tolist() == [1, 2] * 6
    assert out["next_target"].tolist() == [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, -1, -1]
    assert out["n_targets"].tolist() == [6, 6] and out["target_first"].tolist() == [0, 1]
    assert out["ping_first"].tolist() == [0, 0] and out["ping_last"].tolist() == [5, 5]
    assert out["TS_mean"].tolist() == pytest.approx([-45.0, -42.0], abs=1e-12)
    assert out["path_length"][0] == pytest.approx(0.1, abs=1e-12) and out["delta_range"][0] == pytest.approx(0.1, abs=1e-12)
    assert out["tortuosity"][0] == pytest.approx(1.0, abs=1e-9)
    assert out["duration"].tolist() == [5.0, 5.0] and out["speed"][0] == pytest.approx(0.02, abs=1e-12)
    assert out["n_tracks"].tolist() == [2] and out["n_links"].tolist() == [10]
    assert out["n_tracked_targets"].tolist() == [12]


def test_a_gap_of_max_ping_gap_links_and_one_more_does_not():
    """Rows by ping: 10.00 and 12.00 m (ping 0), 10.01 and 12.01 (ping 1), 10.04 (ping 4: two pings missed), 12.05
    (ping 5: three)."""
    out = K.expected("gap")
    assert out["next_target"].tolist() == [2, 3, 4, -1, -1, -1]
    assert out["track_id"].tolist() == [1, 2, 1, 2, 1, 0]
    assert out["n_targets"].tolist() == [3, 2] and out["ping_last"].tolist() == [4, 1]


def test_a_short_chain_is_rejected_and_keeps_its_links():
    out = R.track(K.CASES["gap"][0], K.GATES)  # min_targets = min_pings = 3
    assert out["track_id"].tolist() == [1, 0, 1, 0, 1, 0]
    assert out["next_target"].tolist() == [2, 3, 4, -1, -1, -1]
    assert out["n_tracks"].tolist() == [1] and out["n_links"].tolist() == [3] and out["n_tracked_targets"].tolist() == [3]


def test_contention_for_one_successor():
    """A (10.00 m) and B (10.06 m) at ping 0, J (10.02 m) and K (10.12 m) at ping 1, gates of 0.1 m: both propose to J
    (costs 40 * 0.2**2 = 1.6 and 40 * 0.4**2 = 6.4), J accepts A.  After one round B is alone; in a second round it
    proposes to K, 0.06 m away, which A (0.12 m away) cannot reach."""
    one, three = K.expected("contention_1"), K.expected("contention_3")
    assert one["next_target"].tolist() == [2, -1, -1, -1] and one["track_id"].tolist() == [1, 0, 1, 0]
    assert three["next_target"].tolist() == [2, 3, -1, -1] and three["track_id"].tolist() == [1, 2, 1, 2]
    _, choice = K.case_margins("contention_1")
    # B chose J over K (40 * 0.6**2 = 14.4); J chose A over B.  A had J alone: K is outside its gate
    assert choice.tolist() == pytest.approx([14.4 - 6.4, 6.4 - 1.6], abs=1e-9)


def test_what_the_other_cases_are_there_for():
    assert K.expected("expansion_off")["n_targets"].tolist() == [2] and K.expected("expansion_on")["n_targets"].tolist() == [3]
    assert K.expected("ts_gate_off")["next_target"].tolist() == [1, 3, 4, -1, -1]
    assert K.expected("ts_gate_on")["next_target"].tolist() == [2, 3, 4, -1, -1]
    mirror = K.expected("mirror")
    assert mirror["next_target"].tolist() == [1, -1, -1, 5, -1, -1]  # the lower row wins both ties
    assert sorted(K.expected("chains")["n_targets"].tolist()) == [3, 32, 33]
    assert K.expected("min_rules")["track_id"].tolist() == [0, 0, 1, 0, 1, 0, 1, 0, 1]
    nan = K.expected("nan_lone_targets")
    holes = np.isnan(nan["x"]) | np.isnan(K.CASES["nan"][0]["TS_comp"])
    assert holes.sum() == 5 and not nan["track_id"][holes].any() and (nan["next_target"][holes] == -1).all()
    assert (nan["n_targets"] == 1).sum() == 1 and len(K.expected("nan")["n_targets"]) == 4
    two = K.expected("two_channels")
    t = K.CASES["two_channels"][0]
    last0 = np.flatnonzero((t["channel_index"] == 0) & (t["target_range"] == 12.0))[0]
    assert t["channel_index"][last0 + 1] == 1 and t["target_range"][last0 + 1] == 12.0  # adjoining rows, one position
    assert two["next_target"][last0] == -1 and two["n_links"].tolist() == [2, 4]
    assert len(K.expected("nothing")["n_targets"]) == 0 and len(K.expected("empty")["track_id"]) == 0
    assert "time_first" not in K.expected("no_time") and "time_first" in K.expected("counts")
    counts = np.bincount(K.CASES["counts"][0]["ping_index"], minlength=14).tolist()
    assert {0, 1, 2, 63, 64, 65, K.TILE - 1, K.TILE, K.TILE + 1} == set(counts)
    assert len(K.CASES["dropped"][0]["channel_index"]) == 80


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_decision_of_a_case_keeps_its_distance(name):
    """Every gate quantity that decided something is at least 1e-9 away from 1, and every choice among several
    candidates has at least 1e-9 between the best and the second-best cost -- further than the last bits of the device's
    tan and sqrt can move them -- or exactly 0 at the planted ties, which bit-equal costs keep on the device."""
    gate, choice = K.case_margins(name)
    ties = K.CASES[name][2]
    assert (gate >= 1e-9).all(), gate.min()
    assert int((choice == 0).sum()) == ties
    assert (choice[choice != 0] >= 1e-9).all()
    if len(K.CASES[name][0]["channel_index"]) > 1 and name != "nothing":
        assert len(gate) > 0


@pytest.mark.parametrize("name", sorted(K.BAD))
def test_the_restatement_refuses_a_bad_table(name):
    with pytest.raises(ValueError):
        R.track(K.BAD[name], K.GATES)


# ---- validation before any device work ---------------------------------------------------------------------------------
def _host_ds(t=None, drop=()):
    import echopype_amd as ep

    t = K.CASES["gap"][0] if t is None else t
    ds = ep.Dataset(coords={"channel": [f"ch{i}" for i in range(t["C"])], "ping_time": np.arange(t["P"])})
    for k, v in t.items():
        if isinstance(v, np.ndarray) and k not in drop:
            ds[k] = (("target",), v)
    return ds


def _no_device(monkeypatch):
    from echopype_amd import ops

    for name in ("to_device", "track_prepare"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("device work before the checks"))


@pytest.mark.parametrize("change, match", [
    ({"bogus": 1.0}, "Unknown tracking parameter.*bogus"),
    ({"gate_range": None}, "Missing tracking parameter.*gate_range"),
    ({"gate_alongship": "wide"}, "gate_alongship must be a finite real number"),
    ({"gate_athwartship": True}, "gate_athwartship must be a finite real number"),
    ({"gate_range": float("inf")}, "gate_range must be a finite real number"),
    ({"weight_range": float("nan")}, "weight_range must be a finite real number"),
    ({"missed_ping_expansion": 1j}, "missed_ping_expansion must be a finite real number"),
    ({"gate_range": 0.0}, "gate_range must be positive"),
    ({"gate_alongship": -0.1}, "gate_alongship must be positive"),
    ({"max_ping_gap": -1}, "max_ping_gap must be an integer >= 0"),
    ({"max_ping_gap": 1.5}, "max_ping_gap must be an integer >= 0"),
    ({"link_rounds": 0}, "link_rounds must be an integer >= 1"),
    ({"min_targets": 0}, "min_targets must be an integer >= 1"),
    ({"min_pings": 2.5}, "min_pings must be an integer >= 1"),
    ({"missed_ping_expansion": -5.0}, "missed_ping_expansion must not be negative"),
    ({"weight_TS": -1.0}, "weight_TS must not be negative"),
    ({"weight_alongship": 0, "weight_athwartship": 0, "weight_range": 0}, "must not all be zero"),
    ({"max_TS_difference": 0.0}, "max_TS_difference must be positive or None"),
    ({"weight_TS": 2.0}, "weight_TS > 0 needs max_TS_difference"),
])
def test_parameters_are_checked_before_any_device_work(change, match, monkeypatch):
    import echopype_amd as ep

    _no_device(monkeypatch)
    prm = {k: v for k, v in {**K.GATES, **change}.items() if not (k == "gate_range" and v is None)}
    with pytest.raises(ValueError, match=match):
        ep.targets.track_targets(_host_ds(), "gated_nearest", prm)
    with pytest.raises(ValueError, match="params must be a dict"):
        ep.targets.track_targets(_host_ds(), "gated_nearest", [0.1, 0.1, 0.1])


def test_method_and_columns_are_checked_before_any_device_work(monkeypatch):
    import echopype_amd as ep

    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="Unsupported target tracking method: 'alpha_beta'.*gated_nearest"):
        ep.targets.track_targets(_host_ds(), "alpha_beta", K.GATES)
    for name in ("channel_index", "ping_index", "target_range", "angle_alongship", "angle_athwartship", "TS_comp"):
        with pytest.raises(ValueError, match=f"does not contain the column '{name}'"):
            ep.targets.track_targets(_host_ds(drop=[name]), "gated_nearest", K.GATES)
    ds = _host_ds().drop_vars(["ping_time"])
    with pytest.raises(ValueError, match="no ping_time coordinate"):
        ep.targets.track_targets(ds, "gated_nearest", K.GATES)
    ds = _host_ds()
    ds["TS_comp"] = (("target",), K.CASES["gap"][0]["TS_comp"][:-1])
    with pytest.raises(ValueError, match="TS_comp must be a column on target of 6 rows"):
        ep.targets.track_targets(ds, "gated_nearest", K.GATES)
    ds = _host_ds()
    ds["ping_index"] = (("target",), K.CASES["gap"][0]["ping_index"].astype(np.float64))
    with pytest.raises(ValueError, match="ping_index holds 'f' data"):
        ep.targets.track_targets(ds, "gated_nearest", K.GATES)


def test_exports():
    import echopype_amd as ep
    from echopype_amd import _lib, build, ops

    assert {"track_targets", "METHODS_TRACK", "detect_single_targets", "METHODS_SINGLE_TARGET"} == set(ep.targets.__all__)
    assert ep.targets.METHODS_TRACK.keys() == {"gated_nearest"}
    assert "track.hip" in build.SOURCES
    entries = {"epa_track_prepare", "epa_track_propose", "epa_track_accept", "epa_track_roots", "epa_track_chains",
               "epa_track_table"}
    assert entries == {k for k in _lib.SIGNATURES if k.startswith("epa_track_")}
    hdr = open(os.path.join(ROOT, "include", "echopype_amd.h")).read()
    assert int(re.search(r"#define EPA_TRACK_TILE (\d+)", hdr).group(1)) == ops.TRACK_TILE == _lib.TRACK_TILE == K.TILE
    assert int(re.search(r"#define EPA_TRACK_PARAMS (\d+)", hdr).group(1)) == len(_lib.TRACK_PARAM_NAMES)
    assert int(re.search(r"#define EPA_TRACK_ICOLS (\d+)", hdr).group(1)) == len(_lib.TRACK_ICOL_NAMES)
    assert int(re.search(r"#define EPA_TRACK_FCOLS (\d+)", hdr).group(1)) == len(_lib.TRACK_FCOL_NAMES)
    assert _lib.TRACK_ICOL_NAMES == R.TRACK_INTS and _lib.TRACK_FCOL_NAMES == R.TRACK_FLOATS
    assert ep.targets.track.DEFAULTS == R.DEFAULTS
    doc = ep.targets.track_targets.__doc__
    assert "never been run against Echoview nor on recorded data" in doc and "Sharded datasets are not supported" in doc
    assert "track_targets" in ep.targets.detect_single_targets.__doc__
    assert _lib.lib.epa_version() == 104


def test_the_library_checks_its_arguments_without_a_gpu():
    from echopype_amd import _lib

    with pytest.raises(ValueError, match="epa_track_prepare: bad shape"):
        _lib.call("epa_track_prepare", None, None, None, None, None, -1, 1, 1, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="epa_track_roots: n=4 passes=0"):
        _lib.call("epa_track_roots", None, 4, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="epa_track_table: n=4 T=3 M=2"):
        _lib.call("epa_track_table", *([None] * 9), 4, 3, 2, *([None] * 6))
    with pytest.raises(ValueError, match="epa_track_chains: n=4 min_targets=0"):
        _lib.call("epa_track_chains", *([None] * 6), 4, 0, 1, None, None)
    with pytest.raises(ValueError, match="epa_track_propose: bad params"):
        _lib.call("epa_track_propose", *([None] * 4), 4, 1, 1, None, None, None, None, None, None)
