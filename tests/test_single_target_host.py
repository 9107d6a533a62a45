"""targets.detect_single_targets without a GPU: the two worked rows of the rules against the NumPy restatement, to the
digits written down with them; parameter validation; the exports; and, on the restatement alone, that every scene the
GPU test uses exercises what it is there for."""
import numpy as np
import pytest
import single_target_cases as K
import single_target_ref as R

NAN = float("nan")


def _one_row(ts, al, at, dr, spp=4.0):
    ts = np.asarray(ts, dtype=np.float64)
    S = ts.size
    return R.detect(ts[None, None], np.full((1, 1, S), al), np.full((1, 1, S), at), dr * np.arange(S), spp, 7.0, 7.0,
                    0.0, 0.0, R.DEFAULTS)


def test_worked_row_one_target():
    out = _one_row([-80, -60, -47, -42, -40, -43, -49, -70, -80], 1.0, -0.5, 0.2)
    assert out["n_candidates"].tolist() == [1] and out["n_rejected"].tolist() == [[0, 0, 0, 0]]
    assert out["n_targets"].tolist() == [[1]]
    assert (out["range_sample"].tolist(), out["sample_first"].tolist(), out["sample_last"].tolist()) == ([4], [3], [5])
    assert out["normalized_pulse_length"][0] == 0.75
    assert out["TS_uncomp"][0] == -40.0
    assert out["beam_compensation"][0] == pytest.approx(0.6125415110370679, rel=0, abs=1e-15)
    assert out["TS_comp"][0] == pytest.approx(-39.387458488962935, rel=0, abs=1e-14)
    assert out["target_range"][0] == pytest.approx(0.7878272691087292, rel=0, abs=1e-15)
    assert out["angle_alongship"][0] == 1.0 and out["angle_athwartship"][0] == -0.5
    assert out["std_angle_alongship"][0] == 0.0 and out["std_angle_athwartship"][0] == 0.0


def test_worked_row_candidates_and_rejections():
    ts = [-40, -41, -45, -60, -44, -44, -45, -60, -45, -42, -44, -39, -43, -46, -60, -45, NAN, -44, -45, -60, -48, -44,
          -41]
    assert R.candidates(np.asarray(ts, dtype=np.float64), -50.0) == [0, 4, 9, 11, 15, 17, 22]
    out = _one_row(ts, 0.0, 0.0, 1.0)
    assert out["n_candidates"].tolist() == [7]
    assert out["range_sample"].tolist() == [0, 4, 11]
    assert out["sample_first"].tolist() == [0, 4, 8] and out["sample_last"].tolist() == [2, 6, 12]
    assert out["n_rejected"].tolist() == [[3, 1, 0, 0]]
    assert R.envelope(np.asarray(ts, dtype=np.float64), 9, 6.0) == (8, 13)  # holds the stronger -39: rule 2
    for s in (15, 17, 22):  # cut short by NaN or a row end: rule 1
        lo, hi = R.envelope(np.asarray(ts, dtype=np.float64), s, 6.0)
        assert (hi - lo + 1) / 4.0 < 0.7


def test_exports():
    import echopype_amd as ep
    from echopype_amd import _lib, build, ops

    assert "targets" in ep.__all__ and ep.__all__[-1] == "targets"
    assert "single_target.hip" in build.SOURCES
    assert {"epa_single_target_count", "epa_single_target_emit"} <= set(_lib.SIGNATURES)
    assert ep.targets.METHODS_SINGLE_TARGET.keys() == {"split_beam"}
    assert ops.SINGLE_TARGET_TILE == _lib.SINGLE_TARGET_TILE == 1024
    assert _lib.SINGLE_TARGET_ICOL_NAMES == R.ICOLS and _lib.SINGLE_TARGET_FCOL_NAMES == R.FCOLS
    doc = ep.targets.detect_single_targets.__doc__
    assert "6.0206" in doc and "never been run against Echoview" in doc


def _host_ds(S=9, drop=()):
    import echopype_amd as ep

    z = np.zeros((1, 2, S))
    ds = ep.Dataset(coords={"channel": ["ch1"], "ping_time": np.arange(2), "range_sample": np.arange(S)})
    dims = ("channel", "ping_time", "range_sample")
    for k in ("TS", "angle_alongship", "angle_athwartship"):
        ds[k] = (dims, z - 60.0)
    ds["echo_range"] = (("range_sample",), 0.2 * np.arange(S))
    for k in ("beamwidth_alongship", "beamwidth_athwartship", "angle_offset_alongship", "angle_offset_athwartship"):
        ds[k] = (("channel",), np.array([7.0]))
    return ds.drop_vars(list(drop)) if drop else ds


@pytest.mark.parametrize("change, match", [
    ({"bogus": 1.0}, "Unknown single-target parameter.*bogus"),
    ({"pldl": None}, "Missing single-target parameter.*pldl"),
    ({"TS_threshold": "loud"}, "TS_threshold must be a finite real number"),
    ({"max_std_alongship": True}, "max_std_alongship must be a finite real number"),
    ({"max_beam_compensation": float("inf")}, "max_beam_compensation must be a finite real number"),
    ({"min_norm_pulse_length": float("nan")}, "min_norm_pulse_length must be a finite real number"),
    ({"pldl": 0.0}, "pldl must be positive"),
    ({"pldl": -6.0}, "pldl must be positive"),
    ({"min_norm_pulse_length": 2.0}, "exceeds max_norm_pulse_length"),
    ({"var_name": 3}, "var_name must be a string"),
])
def test_parameters_are_checked_before_any_device_work(change, match, monkeypatch):
    import echopype_amd as ep
    from echopype_amd import ops

    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work before the checks"))
    prm = {**R.DEFAULTS, "pulse_length_samples": 4.0, **change}
    prm = {k: v for k, v in prm.items() if not (k == "pldl" and v is None)}
    with pytest.raises(ValueError, match=match):
        ep.targets.detect_single_targets(_host_ds(), "split_beam", prm)


def test_method_and_variables_are_checked(monkeypatch):
    import echopype_amd as ep
    from echopype_amd import ops

    monkeypatch.setattr(ops, "to_device", lambda *a, **k: pytest.fail("device work before the checks"))
    prm = {**R.DEFAULTS, "pulse_length_samples": 4.0}
    with pytest.raises(ValueError, match="Unsupported single-target detection method: 'single_beam'.*split_beam"):
        ep.targets.detect_single_targets(_host_ds(), "single_beam", prm)
    for name in ("TS", "angle_alongship", "angle_athwartship", "echo_range", "beamwidth_alongship",
                 "beamwidth_athwartship", "angle_offset_alongship", "angle_offset_athwartship"):
        with pytest.raises(ValueError, match=f"does not contain the variable '{name}'"):
            ep.targets.detect_single_targets(_host_ds(drop=[name]), "split_beam", prm)
    with pytest.raises(ValueError, match="does not contain the variable 'Sp'"):
        ep.targets.detect_single_targets(_host_ds(), "split_beam", {**prm, "var_name": "Sp"})
    with pytest.raises(ValueError, match="not among the Dataset's channels"):
        ep.targets.detect_single_targets(_host_ds(), "split_beam", {**prm, "channel": "ch9"})


def test_samples_per_pulse_must_come_from_somewhere():
    import echopype_amd as ep

    with pytest.raises(ValueError, match="samples per pulse are needed"):
        ep.targets.detect_single_targets(_host_ds(), "split_beam", dict(R.DEFAULTS))


# ---- the scenes of the GPU test, judged on the restatement alone ------------------------------------------------------
FULL = [S for S in K.SIZES if S not in K.TINY]


@pytest.mark.parametrize("S", FULL)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_scene_exercises_every_rule(S, dtype):
    want = K.expected(S, dtype)
    first, last = want["sample_first"], want["sample_last"]
    assert len(first) >= 5
    assert (want["n_rejected"].sum(axis=0) >= 3).all(), want["n_rejected"]
    assert (first == 0).any() and (last == S - 1).any()  # an envelope touches each row end
    for seam in range(K.TILE, S, K.TILE):
        assert ((first < seam) & (last >= seam)).any(), f"no envelope crosses the seam at {seam}"
    # the device's fused multiply-adds cannot flip a decision of rule 3 or 4
    assert min(m for _, m in want["margins"]) > 1e-9
    assert want["n_candidates"].sum() == want["n_rejected"].sum() + len(first)
    assert np.isnan(want["target_range"]).sum() < len(first)


@pytest.mark.parametrize("S", K.TINY)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_tiny_rows_exercise_what_their_size_allows(S, dtype):
    """Rows of one to three samples meet the conditions of the full scenes as far as their size allows.  Impossible,
    and therefore not asked: at S = 1 an envelope is one sample, which nothing in it exceeds (rule 2) and whose
    angles have no spread (rule 4: the deviations are 0); at S = 2 the weaker of two samples is no candidate unless
    the other is NaN, so an envelope never holds a stronger sample (rule 2).  At S = 3 all four rules can reject and
    must.  There is no tile seam in such a row."""
    want = K.expected(S, dtype)
    first, last = want["sample_first"], want["sample_last"]
    rejected = want["n_rejected"].sum(axis=0)
    assert len(first) >= 5
    possible = {1: (0, 2), 2: (0, 2, 3), 3: (0, 1, 2, 3)}[S]
    for rule in range(4):
        assert (rejected[rule] >= 3) if rule in possible else (rejected[rule] == 0), (rule + 1, rejected)
    assert (first == 0).any() and (last == S - 1).any()
    assert min(m for _, m in want["margins"]) > 1e-9
    assert want["n_candidates"].sum() == rejected.sum() + len(first)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_long_pulses_reach_the_loops_past_the_kept_samples_and_the_walk_past_the_halo(dtype):
    """The scene with long pulses under the conditions of the full scenes, per channel, and what it is there for:
    accepted envelopes longer than the samples a lane fetches in one go (the loops that read the rest of the angles
    and of the range decide a target), and accepted envelopes that leave the tile of their peak by more than the
    halo, on either side (the walk goes on in global memory), across a tile seam."""
    want = K.long_expected(dtype)
    S = K.LONG_S
    assert min(m for _, m in want["margins"]) > 1e-9
    assert (want["n_rejected"] >= 3).all(), want["n_rejected"]
    n_all = want["sample_last"] - want["sample_first"] + 1
    for c in range(K.C):
        keep = want["channel_index"] == c
        first, last, peak = want["sample_first"][keep], want["sample_last"][keep], want["range_sample"][keep]
        assert keep.sum() >= 5
        assert (first == 0).any() and (last == S - 1).any()
        for seam in range(K.TILE, S, K.TILE):
            assert ((first < seam) & (last >= seam)).any(), f"channel {c}: no envelope crosses the seam at {seam}"
        n = n_all[keep]
        if c == 0:  # up to 1.5 * 12.85 = 19 samples: 1 .. 11 of them read by the loops
            assert (n > K.KEEP).sum() >= 5 and n.max() <= 19 and (n >= 2 * K.KEEP).any()
            assert np.isnan(want["target_range"][keep]).any() and not np.isnan(want["target_range"][keep]).all()
        else:
            tile0 = (peak // K.TILE) * K.TILE
            left = first < tile0 - K.HALO
            right = last >= tile0 + K.TILE + K.HALO
            assert left.sum() >= 3 and right.sum() >= 3, (left.sum(), right.sum())
            # ... and those walks start in one tile and end in another
            assert (first[left] < tile0[left]).all() and (last[right] >= tile0[right] + K.TILE).all()
    # rejections decided out there as well: a candidate of channel 1 whose envelope holds a stronger sample
    assert want["n_rejected"][1, 1] >= 3


def test_the_combination_of_the_host_input_test_keeps_its_distance():
    """tests/test_gpu_single_target.py::test_host_inputs_and_samples_per_pulse_per_channel judges scene(64) with beam
    parameters and pulse lengths of its own: the same margins, here as there."""
    for spp in K.HOST_SPP:
        want = K.host_expected(spp)
        assert len(want["range_sample"]) >= 5 and min(m for _, m in want["margins"]) > 1e-9


def test_the_range_variants_and_the_channel_selection_differ():
    a, b, c = (K.expected(257, "float64", kind)["target_range"] for kind in ("cube", "cs", "s"))
    assert not np.array_equal(a, b, equal_nan=True) and not np.array_equal(b, c, equal_nan=True)
    one = K.expected(257, "float64", "cube", (1,))
    both = K.expected(257, "float64", "cube")
    keep = both["channel_index"] == 1
    assert keep.any() and np.array_equal(one["range_sample"], both["range_sample"][keep])
    assert (one["channel_index"] == 0).all()
