"""targets.track_targets on the GPU (csrc/track.hip through ops.track_* and targets/track.py) against the NumPy
restatement tests/track_ref.py, on the hand-made tables of tests/track_cases.py and, end to end, on the table
detect_single_targets leaves of a small planted cube.

What is compared how
- EQUAL: ``track_id``, ``next_target``, the int32 track columns, the int64 times and the per-channel counts.
  tests/test_track_host.py holds every gate quantity of these tables at least 1e-9 away from 1 and every choice at least
  1e-9 between its best and second-best cost, or exactly 0 at the planted ties: the device's tan and sqrt move a position
  by a few 2**-53 relative, a cost below 100 by less than 1e-12, and the cost itself is evaluated without fused
  multiply-adds, the same bits in propose and accept.
- The float64 columns at the project's float64 bar: |got - want| <= 1e-9 * max(|want|, 1), with identical NaN (and
  infinity) patterns.  A track has at most 33 targets here: its sums are of fewer than 33 terms of one sign."""
import numpy as np
import pytest
import track_cases as K
import track_ref as R

pytestmark = pytest.mark.gpu

FLOATS = ("x", "y", "z") + R.TRACK_FLOATS
INTS = ("track_id", "next_target") + R.TRACK_INTS


def _dataset(t, device=True):
    import torch

    import echopype_amd as ep

    ds = ep.Dataset(coords={"channel": np.array([f"chan{i + 1}" for i in range(t["C"])]),
                            "ping_time": K.T0.astype("datetime64[ns]") + np.arange(t["P"]) * np.timedelta64(1, "s")})
    for k, v in t.items():
        if isinstance(v, np.ndarray):
            ds[k] = ep.DataArray(ep.DeviceArray(torch.as_tensor(v).cuda()), ("target",), name=k) if device \
                else (("target",), v)
    return ds


def _launches(t, prm, want):
    if len(t["channel_index"]) == 0:
        return []
    rounds = {**R.DEFAULTS, **prm}["link_rounds"]
    passes = (max(t["P"], 2) - 1).bit_length()
    return ["track_prepare_kernel"] + ["track_propose_kernel", "track_accept_kernel"] * rounds + \
        ["track_roots_kernel"] * passes + ["track_chains_kernel"] + \
        (["track_order_kernel", "track_table_kernel"] if len(want["n_targets"]) else [])


def _compare(out, want, n):
    T = len(want["n_targets"])
    assert out["target"].shape == (n,) and out["track"].shape == (T,)
    assert out["track"].values.tolist() == list(range(1, T + 1))
    for k in INTS:
        got = out[k].values
        assert got.dtype == np.int32 and np.array_equal(got, want[k]), k
    for k in R.CHANNEL_VARS:
        assert np.array_equal(out[k].values, want[k]) and out[k].dims == ("channel",), k
    times = R.TRACK_TIMES if "time_first" in want else ()
    for k in R.TRACK_TIMES:
        assert (k in out) == bool(times), k
    for k in times[:2]:
        assert out[k].values.dtype == np.int64 and np.array_equal(out[k].values, want[k]), k
    worst = {}
    for k in FLOATS + times[2:]:
        got, ref = out[k].values, want[k]
        assert got.dtype == np.float64 and got.shape == ref.shape, k
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), k
        assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), k
        f = np.isfinite(ref)
        worst[k] = float(np.max(np.abs(got[f] - ref[f]) / np.maximum(np.abs(ref[f]), 1.0))) if f.any() else 0.0
    print("largest errors relative to max(|want|, 1):", worst)
    for k, e in worst.items():
        assert e <= 1e-9, (k, e)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_tracks_equal_the_restatement(name):
    """Per case: the result against the restatement, everything resident on the device, the kernels launched, one host
    copy per call (of three numbers), and a second call bit-identical to the first."""
    import torch

    import echopype_amd as ep
    from echopype_amd import _lib
    from echopype_amd.targets import track as api

    t, prm, _ = K.CASES[name]
    want = K.expected(name)
    n = len(t["channel_index"])
    ds = _dataset(t)
    reads = []
    real = api._to_host
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(api, "_to_host", lambda x: (reads.append(x.numel()), real(x))[1])
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
        with _lib.launch_trace() as trace:
            out = ep.targets.track_targets(ds, "gated_nearest", prm)
        again = ep.targets.track_targets(ds, "gated_nearest", prm)
    assert trace.kernels == _launches(t, prm, want)
    assert reads == ([3, 3] if n else [])
    _compare(out, want, n)
    names = INTS + FLOATS + R.CHANNEL_VARS + (R.TRACK_TIMES if "time_first" in want else ())
    for k in names:
        assert ep.xr_lite.is_device(out[k].data), k
        assert np.array_equal(out[k].values, again[k].values, equal_nan=True), k
    assert out["channel"].values.tolist() == ds["channel"].values.tolist()
    assert np.array_equal(out["ping_time"].values, ds["ping_time"].values)
    assert out.attrs["method"] == "gated_nearest" and out.attrs["gate_range"] == prm["gate_range"]
    assert out.attrs["link_rounds"] == {**R.DEFAULTS, **prm}["link_rounds"]


@pytest.mark.parametrize("name", sorted(K.BAD))
def test_a_bad_table_raises_after_the_one_host_copy(name):
    import echopype_amd as ep
    from echopype_amd.targets import track as api

    reads = []
    real = api._to_host
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(api, "_to_host", lambda x: (reads.append(x.numel()), real(x))[1])
        with pytest.raises(ValueError, match="not ordered by .channel_index, ping_index., or holds an index outside"):
            ep.targets.track_targets(_dataset(K.BAD[name]), "gated_nearest", K.GATES)
    assert reads == [3]


def test_host_columns_of_other_types():
    """NumPy-backed columns are uploaded; float32 columns are converted to float64 (exactly), int64 indices to int32."""
    import echopype_amd as ep

    t, prm, _ = K.CASES["dropped"]
    t32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in t.items()}
    t32["channel_index"], t32["ping_index"] = t["channel_index"].astype(np.int64), t["ping_index"].astype(np.int64)
    t64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in t32.items()}
    gate, choice = R.margins(t64, prm)
    assert min(gate.min(), choice.min()) >= 1e-9
    want = R.track(t64, prm)
    assert len(want["n_targets"]) >= 5
    _compare(ep.targets.track_targets(_dataset(t32, device=False), "gated_nearest", prm), want, len(t["channel_index"]))
    big = dict(t32, ping_index=t32["ping_index"] + 2 ** 32)  # would wrap into range as int32
    with pytest.raises(ValueError, match="holds an index outside"):
        ep.targets.track_targets(_dataset(big, device=False), "gated_nearest", prm)


# ---- end to end: detect_single_targets -> track_targets ----------------------------------------------------------------
E2E_C, E2E_P, E2E_S = 2, 12, 90
DETECT = {"TS_threshold": -60.0, "pldl": 6.0, "min_norm_pulse_length": 0.7, "max_norm_pulse_length": 1.5,
          "max_beam_compensation": 6.0, "max_std_alongship": 1.0, "max_std_athwartship": 1.0, "pulse_length_samples": 4.0}
TRACK = {"gate_alongship": 0.25, "gate_athwartship": 0.25, "gate_range": 0.25, "weight_ping_gap": 10.0}
# (first sample, pings per sample of drift, alongship, athwartship, peak TS, pings without an echo)
ECHOES = ((20, 3, 0.5, -0.3, -40.0, (3,)), (45, 4, -0.8, 0.2, -43.0, (5, 6)), (70, -5, 0.1, 0.9, -38.0, (9,)))


def _planted_cube():
    """Two channels of a dozen pings and 90 samples at 0.2 m, silent but for three echoes of three samples (a peak and
    two shoulders 6 dB below: 0.75 pulse lengths) that drift a sample every few pings and miss a ping or two."""
    ts = np.full((E2E_C, E2E_P, E2E_S), -90.0)
    al, at = np.zeros_like(ts), np.zeros_like(ts)
    for c in range(E2E_C):
        for s0, per, a, b, peak, missing in ECHOES:
            for p in range(E2E_P):
                if p in missing:
                    continue
                s = s0 + 3 * c + p // per
                ts[c, p, s - 1:s + 2] = (peak - 6.0 - 0.5 * c, peak - 0.5 * c, peak - 6.0 - 0.5 * c)
                al[c, p, s - 1:s + 2], at[c, p, s - 1:s + 2] = a, b
    return ts, al, at


def test_detector_then_tracker_on_a_planted_cube():
    """The table the detector leaves on the device goes into the tracker as it is; the judge is the restatement run on
    that table, downloaded.  Its decisions must keep the distance the hand-made tables keep: asserted, not assumed."""
    import torch

    import echopype_amd as ep

    ts, al, at = _planted_cube()
    dims = ("channel", "ping_time", "range_sample")
    ds = ep.Dataset(coords={"channel": np.array(["chan1", "chan2"]), "range_sample": np.arange(E2E_S),
                            "ping_time": K.T0.astype("datetime64[ns]") + np.arange(E2E_P) * np.timedelta64(500, "ms")})
    for k, v in (("TS", ts), ("angle_alongship", al), ("angle_athwartship", at)):
        ds[k] = ep.DataArray(ep.DeviceArray(torch.as_tensor(v).cuda()), dims, name=k)
    ds["echo_range"] = (("range_sample",), 0.2 * np.arange(E2E_S))
    for k, v in (("beamwidth_alongship", 7.0), ("beamwidth_athwartship", 7.0), ("angle_offset_alongship", 0.0),
                 ("angle_offset_athwartship", 0.0)):
        ds[k] = (("channel",), np.full(E2E_C, v))
    table = ep.targets.detect_single_targets(ds, "split_beam", DETECT)
    n_echoes = E2E_C * sum(E2E_P - len(e[5]) for e in ECHOES)
    assert table["target"].shape == (n_echoes,)
    out = ep.targets.track_targets(table, "gated_nearest", TRACK)

    host = {k: table[k].values for k in ("channel_index", "ping_index", "target_range", "angle_alongship",
                                         "angle_athwartship", "TS_comp", "target_ping_time")}
    host.update(C=E2E_C, P=E2E_P)
    gate, choice = R.margins(host, TRACK)
    assert len(gate) > 100 and len(choice) > 20
    assert gate.min() >= 1e-9 and choice.min() >= 1e-9, (gate.min(), choice.min())
    want = R.track(host, TRACK)
    assert want["n_targets"].tolist() == [E2E_P - len(e[5]) for e in ECHOES] * E2E_C  # every echo in its fish's track
    _compare(out, want, n_echoes)
    assert out["duration"].values.max() == 5.5
