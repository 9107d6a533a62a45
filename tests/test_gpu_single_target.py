"""targets.detect_single_targets on the GPU (csrc/single_target.hip through ops.single_target_count /
ops.single_target_emit and targets/api.py) against the NumPy restatement tests/single_target_ref.py, on the scenes of
tests/single_target_cases.py: two channels of 37 pings whose rows end at the edges of a row (1, 2, 3 samples), of a
wave (63, 64, 65), of the kernel's tile (one less, exactly, one more) and after several tiles.

What is compared how
- EQUAL: the int32 columns (channel, ping, peak, envelope), ``target_ping_time``, ``n_targets``, ``n_candidates``,
  ``n_rejected``: rules 1 and 2 are one subtraction or one division on exact inputs (float32 -> float64 is exact), and
  tests/test_single_target_host.py holds every rule-3 / rule-4 quantity of these scenes at least 1e-9 away from its
  limit, further than the orders of summation and the device's fused multiply-adds can move it (see below).
- The float64 columns at the project's float64 bar: |got - want| <= 1e-9 * max(|want|, 1), with identical NaN
  patterns.  An envelope has at most max_norm_pulse_length * spp samples, below 200 in the scene with long pulses and
  below 10 elsewhere: means, deviations and the weighted range are sums of fewer than 200 terms of one sign or of
  magnitude below 100, off by a few hundred 2**-53 relative at the most -- orders of magnitude inside the bar."""
import numpy as np
import pytest
import single_target_cases as K
import single_target_ref as R

pytestmark = pytest.mark.gpu

DIMS = ("channel", "ping_time", "range_sample")
T0 = np.datetime64("2026-10-20T00:00:00", "ns")
COUNTS = ("n_targets", "n_candidates", "n_rejected")


def _ping_time(P):
    return T0 + np.arange(P) * np.timedelta64(1000, "ms")


def _dataset(d, range_kind="cube", order=DIMS, P=K.P):
    """The scene ``d`` as a device-resident Dataset, its cubes stored with the dimensions in ``order``."""
    import torch

    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    C, _, S = d["TS"].shape
    ds = Dataset(coords={"channel": np.array([f"chan{i + 1}" for i in range(C)]), "ping_time": _ping_time(P),
                         "range_sample": np.arange(S)})
    perm = [DIMS.index(x) for x in order]
    for k in ("TS", "angle_alongship", "angle_athwartship"):
        t = torch.as_tensor(d[k].transpose(perm).copy()).cuda()
        ds[k] = DataArray(DeviceArray(t), order, name=k)
    rdims = {"cube": DIMS, "cs": ("channel", "range_sample"), "s": ("range_sample",)}[range_kind]
    ds["echo_range"] = DataArray(DeviceArray(torch.as_tensor(np.array(d["range_" + range_kind])).cuda()), rdims)
    ds["beamwidth_alongship"] = (("channel", "ping_time"), K.BEAMWIDTH_AL[:C, :P])
    ds["beamwidth_athwartship"] = (("channel",), K.BEAMWIDTH_AT[:C])
    ds["angle_offset_alongship"] = (("channel",), K.OFFSET_AL[:C])
    ds["angle_offset_athwartship"] = (("channel",), K.OFFSET_AT[:C])
    return ds


def _compare(out, want, P=K.P):
    n = len(want["range_sample"])
    assert out["target"].shape == (n,)
    for k in R.ICOLS:
        got = out[k].values
        assert got.dtype == np.int32 and np.array_equal(got, want[k]), k
    for k in COUNTS:
        assert np.array_equal(out[k].values, want[k]), k
    assert out["n_targets"].values.dtype == np.int32
    assert np.array_equal(out["target_ping_time"].values, _ping_time(P).view(np.int64)[want["ping_index"]])
    worst = {}
    for k in R.FCOLS:
        got, ref = out[k].values, want[k]
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(ref)), k
        f = ~np.isnan(ref)
        worst[k] = float(np.max(np.abs(got[f] - ref[f]) / np.maximum(np.abs(ref[f]), 1.0))) if f.any() else 0.0
    print("largest errors relative to max(|want|, 1):", worst)
    for k, e in worst.items():
        assert e <= 1e-9, (k, e)


def _params(d, **extra):
    return {**K.PARAMS, "pulse_length_samples": np.array(d["spp"]), **extra}


@pytest.mark.parametrize("S", K.SIZES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_table_equals_the_restatement(S, dtype):
    import echopype_amd as ep
    from echopype_amd import _lib

    d = K.scene(S, dtype)
    want = K.expected(S, dtype)
    with _lib.launch_trace() as t:
        out = ep.targets.detect_single_targets(_dataset(d), "split_beam", _params(d))
    assert t.kernels == ["single_target_count_kernel", "single_target_emit_kernel"]
    assert len(want["range_sample"]) >= 5
    _compare(out, want)
    for k in R.ICOLS + R.FCOLS + COUNTS + ("target_ping_time",):
        assert ep.xr_lite.is_device(out[k].data), k


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_long_pulses(dtype):
    """Envelopes of up to 19 samples (channel 0) and of 113 .. 154 (channel 1): the loops that read the angles and the
    range past the samples a lane fetches in one go, and the walks that leave the halo of the tile and go on in global
    memory, decide targets (tests/test_single_target_host.py holds the scene to that)."""
    import echopype_amd as ep

    d = K.long_scene(dtype)
    want = K.long_expected(dtype)
    n = want["sample_last"] - want["sample_first"] + 1
    assert (n > K.KEEP).sum() >= 10 and (n > K.HALO).sum() >= 10
    _compare(ep.targets.detect_single_targets(_dataset(d), "split_beam", _params(d)), want)


@pytest.mark.parametrize("range_kind", ["cs", "s"])
def test_range_is_read_through_its_strides(range_kind):
    import echopype_amd as ep

    d = K.scene(257, "float64")
    out = ep.targets.detect_single_targets(_dataset(d, range_kind), "split_beam", _params(d))
    _compare(out, K.expected(257, "float64", range_kind))


def test_dimensions_in_another_order_and_mixed_types():
    """TS stored (ping_time, range_sample, channel); float32 TS with float64 angles and range: all go to float64."""
    import echopype_amd as ep
    import torch

    d = K.scene(65, "float64")
    ds = _dataset(d, order=("ping_time", "range_sample", "channel"))
    _compare(ep.targets.detect_single_targets(ds, "split_beam", _params(d)), K.expected(65, "float64"))
    d32 = K.scene(65, "float32")
    ds = _dataset(d32)
    for k in ("angle_alongship", "angle_athwartship", "echo_range"):
        ds[k] = ep.DataArray(ep.DeviceArray(ds[k].data.tensor.double()), ds[k].dims, name=k)
    assert ds["TS"].data.tensor.dtype == torch.float32
    _compare(ep.targets.detect_single_targets(ds, "split_beam", _params(d32)), K.expected(65, "float32"))


def test_one_channel_selected():
    import echopype_amd as ep

    d = K.scene(257, "float64")
    out = ep.targets.detect_single_targets(_dataset(d), "split_beam", _params(d, channel="chan2"))
    _compare(out, K.expected(257, "float64", "cube", (1,)))
    assert out["channel"].values.tolist() == ["chan2"]


def test_host_inputs_and_samples_per_pulse_per_channel():
    """NumPy-backed variables are uploaded; ``pulse_length_samples`` as a scalar and as one number per channel."""
    import echopype_amd as ep

    d = K.scene(64, "float32")
    ds = ep.Dataset(coords={"channel": ["a", "b"], "ping_time": _ping_time(K.P), "range_sample": np.arange(64)})
    for k in ("TS", "angle_alongship", "angle_athwartship"):
        ds[k] = (DIMS, np.array(d[k]))
    ds["echo_range"] = (("range_sample",), np.array(d["range_s"]))
    for k, v in zip(("beamwidth_alongship", "beamwidth_athwartship", "angle_offset_alongship",
                     "angle_offset_athwartship"), K.HOST_BEAM):
        ds[k] = (("channel",), np.full(K.C, v))
    for spp in K.HOST_SPP:
        out = ep.targets.detect_single_targets(ds, "split_beam", {**K.PARAMS, "pulse_length_samples": np.asarray(spp)})
        want = K.host_expected(spp)
        assert len(want["range_sample"]) >= 5 and min(m for _, m in want["margins"]) > 1e-9
        _compare(out, want)


def test_nothing_to_find_gives_an_empty_table_without_an_emit_launch():
    import echopype_amd as ep
    from echopype_amd import _lib

    d = K.scene(65, "float64")
    quiet = {**d, "TS": np.minimum(d["TS"], -50.5)}
    dark = {**d, "TS": np.full_like(d["TS"], np.nan)}
    none = {k: (v[:, :0] if v.ndim == 3 else v) for k, v in d.items()}
    none["spp"] = d["spp"][:, :0]
    for case, P, launches in ((quiet, K.P, ["single_target_count_kernel"]), (dark, K.P, ["single_target_count_kernel"]),
                              (none, 0, [])):
        ds = _dataset(case, P=P)
        with _lib.launch_trace() as t:
            out = ep.targets.detect_single_targets(ds, "split_beam", _params(case))
        assert t.kernels == launches
        assert out["target"].shape == (0,)
        for k in R.ICOLS + R.FCOLS + ("target_ping_time",):
            assert out[k].shape == (0,), k
        assert out["n_targets"].shape == (K.C, P) and not out["n_targets"].values.any()
        assert out["n_rejected"].shape == (K.C, 4) and out["n_candidates"].shape == (K.C,)
        assert out["TS_comp"].values.dtype == np.float64 and out["range_sample"].values.dtype == np.int32
        assert not out["n_candidates"].values.any() and not out["n_rejected"].values.any()
    no_samples = {k: (v[..., :0] if v.ndim == 3 or k == "range_s" else v) for k, v in d.items()}
    out = ep.targets.detect_single_targets(_dataset(no_samples), "split_beam", _params(d))
    assert out["target"].shape == (0,) and out["n_targets"].shape == (K.C, K.P)


def test_two_calls_agree_and_the_host_waits_once():
    import torch

    import echopype_amd as ep
    from echopype_amd.targets import api

    d = K.scene(K.TILE + 1, "float32")
    ds = _dataset(d)
    reads = []
    real = api._to_host
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(api, "_to_host", lambda t: (reads.append(t.numel()), real(t))[1])
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
        a = ep.targets.detect_single_targets(ds, "split_beam", _params(d))
        assert reads == [1]
        b = ep.targets.detect_single_targets(ds, "split_beam", _params(d))
        assert reads == [1, 1]
    for k in R.ICOLS + R.FCOLS + COUNTS + ("target_ping_time",):
        assert np.array_equal(a[k].values, b[k].values, equal_nan=True), k


def test_whole_chain_from_ek60_samples():
    """compute_TS -> add_splitbeam_angle -> detect_single_targets on a synthetic EK60 EchoData equals the restatement
    fed the arrays the first two leave, with spp from the beam group."""
    import echopype_amd as ep
    from echopype_amd import echodata, synth

    d = synth.ek60_splitbeam_numpy(C=2, P=24, S=300)
    ed = echodata.from_ek60_arrays(d)
    ds = ep.calibrate.compute_TS(ed)
    for k, v in (("angle_sensitivity_alongship", d["angle_sensitivity_alongship"]),
                 ("angle_sensitivity_athwartship", d["angle_sensitivity_athwartship"]),
                 ("angle_offset_alongship", d["angle_offset_alongship"]),
                 ("angle_offset_athwartship", d["angle_offset_athwartship"]),
                 ("beamwidth_alongship", np.full(2, 7.0)), ("beamwidth_athwartship", np.full(2, 7.2))):
        if k not in ds:
            ds[k] = (("channel",), np.asarray(v, dtype=np.float64))
    ds = ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)
    ts = np.asarray(ds["TS"].values)
    # synthetic noise has no echoes: the threshold is set where the strongest 2 % of the samples are, the pulse-length
    # window wide, the compensation and spread limits loose enough for the scattered angles of the scene to pass some
    prm = {"TS_threshold": float(np.nanpercentile(ts, 98.0)), "pldl": 6.0, "min_norm_pulse_length": 0.1,
           "max_norm_pulse_length": 3.0, "max_beam_compensation": 12.0, "max_std_alongship": 3.0,
           "max_std_athwartship": 3.0}
    out = ep.targets.detect_single_targets(ds, "split_beam", prm, echodata=ed)
    beam = ed[echodata.BEAM1]
    spp = np.asarray(beam["transmit_duration_nominal"].values) / np.asarray(beam["sample_interval"].values)

    def cp(name):
        return np.asarray(ds[name].values, dtype=np.float64)

    want = R.detect(ts, np.asarray(ds["angle_alongship"].values), np.asarray(ds["angle_athwartship"].values),
                    np.asarray(ds["echo_range"].values), spp, cp("beamwidth_alongship"), cp("beamwidth_athwartship"),
                    cp("angle_offset_alongship"), cp("angle_offset_athwartship"), prm)
    assert len(want["range_sample"]) >= 5 and min(m for _, m in want["margins"]) > 1e-9
    n = len(want["range_sample"])
    assert out["target"].shape == (n,)
    for k in R.ICOLS + COUNTS:
        assert np.array_equal(out[k].values, want[k]), k
    for k in R.FCOLS:
        got, ref = out[k].values, want[k]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), k
        f = ~np.isnan(ref)
        assert np.all(np.abs(got[f] - ref[f]) <= 1e-9 * np.maximum(np.abs(ref[f]), 1.0)), k
