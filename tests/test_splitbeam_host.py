"""consolidate.add_splitbeam_angle on the host (no GPU): the reference-executed goldens against the NumPy restatement
of tests/splitbeam_ref.py, the drop-in signature, and every validation error of the reference (consolidate/api.py:423-495,
split_beam_angle.py:155-170, 240-264) with its exception type -- raised before anything is allocated on a device
(a device allocation on a machine without a GPU raises something else)."""
import json
import os

import numpy as np
import pytest

from splitbeam_ref import GOLDEN, load_goldens, assert_complex_close, complex_angles, power_angles

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g():
    return load_goldens(os.path.join(HERE, "golden", GOLDEN))


def _prm(g, tag):
    return [g[f"{tag}_{k}"] for k in ("sens_al", "sens_at", "off_al", "off_at")]


def _replicas(g, tag):
    reps, k = [], 0
    while f"{tag}_replica{k}_0" in g:
        c = 0
        while f"{tag}_replica{k}_{c}" in g:
            reps.append(g[f"{tag}_replica{k}_{c}"])
            c += 1
        k += 1
    return reps


@pytest.mark.parametrize("tag", ["pow_i8", "pow_f32"])
def test_power_goldens_equal_the_restatement(g, tag):
    th, ph = power_angles(g[f"{tag}_angle_alongship"], g[f"{tag}_angle_athwartship"], *_prm(g, tag))
    for got, want in ((th, g[f"{tag}_theta"]), (ph, g[f"{tag}_phi"])):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        f = ~np.isnan(want)
        assert np.max(np.abs(got[f] - want[f])) <= 1e-12


@pytest.mark.parametrize("tag", ["cx_bt1", "cx_bt17", "cx_bt49", "cx_bt65", "cx_bt81", "cx_mixed", "pc_fft", "pc_fft17",
                                 "pc_short", "pc_long", "pc_multi"])
def test_complex_goldens_equal_the_restatement(g, tag):
    reps = _replicas(g, tag) or None
    rid = g[f"{tag}_replica_id"] if reps else None
    sa, st, oa, ot = _prm(g, tag)
    th, ph, _, weak = complex_angles(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"], sa, st, oa, ot, reps, rid)
    assert_complex_close(th, g[f"{tag}_theta"], sa, oa, weak)
    assert_complex_close(ph, g[f"{tag}_phi"], st, ot, weak)


def test_goldens_hold_what_they_are_for(g):
    """The cases the GPU tests rely on: both tap regimes of each form, a skipped channel, NaN patterns."""
    taps = {tag: max(r.size for r in _replicas(g, tag)) for tag in ("pc_fft", "pc_short", "pc_long", "pc_multi")}
    assert 16 <= taps["pc_fft"] <= 1024 and taps["pc_short"] < 16 and taps["pc_long"] > 1024
    assert len(np.unique(g["pc_multi_replica_id"])) == 4
    assert g["pc_fft_re"].shape[2] > 2048  # crosses the overlap-save seam (2049 - taps) and the direct tile edge
    assert np.isnan(g["cx_mixed_theta"][2]).all() and not np.isnan(g["cx_mixed_theta"][:2]).all()
    one = np.isnan(g["cx_bt1_re"]) | np.isnan(g["cx_bt1_im"])
    assert (one.sum(axis=-1) == 1).any()  # a sample with exactly one NaN sector


def test_signature_equals_the_reference(g):
    import inspect

    import echopype_amd as ep

    ref = json.loads(str(g["signature"]))["params"]
    got = [(p.name, p.kind, p.default) for p in inspect.signature(ep.consolidate.add_splitbeam_angle).parameters.values()]
    core = [x for x in got if x[0] not in ("dtype", "device", "fft_dtype")]
    assert [x[0] for x in core] == [r[0] for r in ref]
    for (name, kind, default), (_, rkind, rsrc) in zip(core, ref):
        assert kind == inspect.Parameter.POSITIONAL_OR_KEYWORD and rkind == "positional_or_keyword"
        if rsrc is None:
            assert default is inspect.Parameter.empty, name
        else:
            assert default == eval(rsrc) and type(default) is type(eval(rsrc)), name  # noqa: S307 - fixture literals
    for name, kind, default in got:
        if name in ("dtype", "device", "fft_dtype"):
            assert kind == inspect.Parameter.KEYWORD_ONLY and default is None


# ---- validation ----------------------------------------------------------------------------------------------------
def _ek80(beam_type=1, encode="complex", waveform="BB", B=4):
    from echopype_amd import echodata, synth

    d, _, _ = synth.ek80_splitbeam_numpy(C=2, P=3, S=40, B=B, beam_type=beam_type, waveform=waveform)
    ed = echodata.from_ek80_arrays(d, synth.ek80_filters(), encode=encode)
    return ed, d


def _sv_like(d, C=2, drop=None, attrs=None):
    from echopype_amd.xr_lite import Dataset

    P, S = d["backscatter_r"].shape[1:3]
    ds = Dataset(coords={"channel": list(d["channel"])[:C], "ping_time": d["ping_time"], "range_sample": np.arange(S)},
                 attrs=attrs or {"processing_function": "calibrate.compute_Sv"})
    ds["Sv"] = (("channel", "ping_time", "range_sample"), np.zeros((C, P, S)))
    for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
              "angle_offset_athwartship"):
        if k != drop:
            ds[k] = (("channel",), np.asarray(d[k], float)[:C])
    return ds


@pytest.fixture
def no_device(monkeypatch):
    """Any device allocation or upload fails loudly with a type no validation error has."""
    import torch

    from echopype_amd import ops

    class Allocated(Exception):
        pass

    def boom(*a, **k):
        raise Allocated("device touched before validation finished")

    monkeypatch.setattr(ops, "to_device", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    return Allocated


def test_to_disk_with_a_dataset_is_the_first_error(no_device):
    import echopype_amd as ep

    ed, d = _ek80()
    with pytest.raises(ValueError, match="must be a path when to_disk=True"):
        ep.consolidate.add_splitbeam_angle(_sv_like(d), ed, "BB", "complex")
    with pytest.raises(ValueError, match="must be a path when to_disk=True"):  # before the sonar model is looked at
        ep.consolidate.add_splitbeam_angle(_sv_like(d), None, "XX", "complex")


def test_paths_are_not_implemented(no_device, tmp_path):
    import echopype_amd as ep

    ed, d = _ek80()
    with pytest.raises(NotImplementedError, match="file path"):
        ep.consolidate.add_splitbeam_angle(str(tmp_path / "sv.zarr"), ed, "BB", "complex")
    with pytest.raises(NotImplementedError, match="file path"):
        ep.consolidate.add_splitbeam_angle(_sv_like(d), tmp_path / "raw.zarr", "BB", "complex", to_disk=False)


def test_sonar_model_mvbs_and_channel(no_device):
    import echopype_amd as ep
    from echopype_amd.echodata import EchoData

    ed, d = _ek80()
    azfp = EchoData("AZFP", {})
    with pytest.raises(ValueError, match="does not have split-beam"):
        ep.consolidate.add_splitbeam_angle(_sv_like(d), azfp, "CW", "power", to_disk=False)
    with pytest.raises(NotImplementedError, match="MVBS"):
        ep.consolidate.add_splitbeam_angle(_sv_like(d, attrs={"processing_function": "commongrid.compute_MVBS"}), ed,
                                           "BB", "complex", to_disk=False)
    with pytest.raises(RuntimeError):  # retrieve_correct_beam_group: no power group in this file
        ep.consolidate.add_splitbeam_angle(_sv_like(d), ed, "CW", "power", to_disk=False)
    from echopype_amd.xr_lite import Dataset

    no_channel = Dataset(attrs={"processing_function": "calibrate.compute_Sv"})
    with pytest.raises(ValueError, match="must have a channel dimension"):
        ep.consolidate.add_splitbeam_angle(no_channel, ed, "BB", "complex", to_disk=False)


@pytest.mark.parametrize("missing", ["angle_sensitivity_alongship", "angle_sensitivity_athwartship",
                                     "angle_offset_alongship", "angle_offset_athwartship"])
def test_missing_angle_parameter(no_device, missing):
    import echopype_amd as ep

    ed, d = _ek80()
    with pytest.raises(ValueError, match=f"necessary parameter {missing}"):
        ep.consolidate.add_splitbeam_angle(_sv_like(d, drop=missing), ed, "BB", "complex", to_disk=False)


def test_power_samples_of_single_beam_transducers(no_device):
    import echopype_amd as ep
    from echopype_amd import echodata, synth

    d = synth.ek60_splitbeam_numpy(C=2, P=4, S=30)
    d["beam_type"] = np.zeros(2, dtype=np.int64)
    ed = echodata.from_ek60_arrays(d)
    ds = _sv_like({**d, "backscatter_r": d["backscatter_r"][..., None]})
    with pytest.raises(ValueError, match="only available for data from split-beam transducers"):
        ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)


@pytest.mark.parametrize("bt,exc", [(97, NotImplementedError), (3, ValueError), (0, ValueError)])
def test_one_unsupported_beam_type_for_every_channel(no_device, bt, exc):
    import echopype_amd as ep

    ed, d = _ek80(beam_type=1)
    ed["Sonar/Beam_group1"]["beam_type"] = (("channel",), np.array([bt, bt]))
    with pytest.raises(exc):
        ep.consolidate.add_splitbeam_angle(_sv_like(d), ed, "BB", "complex", to_disk=False)


def test_builders_without_the_new_keys_build_what_they_built():
    """from_ek60_arrays / from_ek80_arrays: the split-beam keys are optional and add nothing when absent."""
    from echopype_amd import echodata, synth

    d60 = synth.ek60_numpy(2, 5, 20)
    beam = echodata.from_ek60_arrays(d60)["Sonar/Beam_group1"]
    assert not {"angle_alongship", "angle_athwartship", "beam_type"} & set(beam.data_vars)
    d80 = synth.ek80_numpy(C=2, P=3, S=20)
    beam = echodata.from_ek80_arrays(d80, synth.ek80_filters())["Sonar/Beam_group1"]
    assert "beam_type" not in beam.data_vars
    d = synth.ek60_splitbeam_numpy(C=2, P=4, S=30)
    beam = echodata.from_ek60_arrays(d)["Sonar/Beam_group1"]
    assert beam["angle_alongship"].dtype == np.int8 and list(beam["beam_type"].values) == [1, 1]


def test_known_target_generator_encodes_its_angles():
    from echopype_amd import synth

    for bt, B in ((1, 4), (17, 3), (49, 4), (81, 4)):
        d, th, ph = synth.ek80_splitbeam_numpy(C=2, P=3, S=64, B=B, beam_type=bt)
        got_th, got_ph, _, _ = complex_angles(d["backscatter_r"], d["backscatter_i"], d["beam_type"],
                                              d["angle_sensitivity_alongship"], d["angle_sensitivity_athwartship"],
                                              d["angle_offset_alongship"], d["angle_offset_athwartship"])
        assert np.max(np.abs(got_th - th)) < 1e-12 and np.max(np.abs(got_ph - ph)) < 1e-12
