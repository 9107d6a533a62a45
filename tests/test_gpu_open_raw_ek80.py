"""``open_raw_ek80`` on a real MI355X: the RAW3 unpack kernel alone, bit-equal to what the REFERENCE's parsers read and
padded from the same bytes (tests/golden/open_raw_ek80.npz); every output element written exactly once and nothing behind
the outputs touched -- with pre-filled ``out=`` planes and with the whole call under ``tests/poison.py``, which is the
property tests/test_gpu_poisoned_buffers.py checks for the wrappers of ``ops.py``; the product (``compute_Sv``,
``compute_TS``, ``add_splitbeam_angle`` on what ``open_raw_ek80`` returns) bit-equal to the same calls on an EchoData built
from the same arrays; positions; cut and broken files.

There is no tolerance anywhere: the kernel copies bits, compared as int32 words; NaN is NumPy's 0x7FC00000 exactly where
the reference has it -- padding, imaginary parts equal to 0, sectors and rows a channel lacks."""
import logging

import numpy as np
import pytest

import raw3_cases as R
from poison import BYTES, Poisoned

pytestmark = pytest.mark.gpu

KERNEL = "raw3_unpack_kernel"
NAN_BITS = np.int32(0x7FC00000)
SENTINELS = (-559038737, 0x5A5A5A5A)  # 0xDEADBEEF and a second pattern: neither is a sample of the fixtures nor the NaN
GUARD = 64


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


_plans = {}


def _plan(case):
    from echopype_amd.convert import parse_ek80

    if case not in _plans:
        _plans[case] = parse_ek80.plan(R.file_bytes(case))
    return _plans[case]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(what, re, im, want_re, want_im):
    for name, got, want in (("backscatter_r", re, want_re), ("backscatter_i", im, want_im)):
        assert got.dtype == np.float32 and got.shape == want.shape, (what, name, got.shape, want.shape)
        bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
        assert bad.size == 0, f"{what}: {bad.size} {name} words differ, first at {np.unravel_index(bad[0], got.shape)}"
        assert np.array_equal(_bits(got) == NAN_BITS, np.isnan(want))


def _complex_groups(case):
    return [(g, R.expected_groups(case)[g.descr]) for g in _plan(case).groups if g.descr != "power"]


def _channel_alone(g, e, ci):
    """One channel of a group as a launch of its own with B = the channel's sector count: (table, S, B, real, imag)."""
    tab = g.table.reshape(g.C, g.P, 3)[ci]
    S, B = int(max(1, tab[:, 1].max())), int(tab[:, 2].max())
    return tab, S, B, e["real"][ci:ci + 1, :, :S, :B], e["imag"][ci:ci + 1, :, :S, :B]


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_kernel_alone_is_bit_equal_to_the_reference_parse(ep, case):
    from echopype_amd import _lib
    from echopype_amd.convert.raw3_unpack import raw3_unpack

    dev, n = ep.ops.upload_file_bytes(R.file_bytes(case))
    assert dev.numel() % 16 == 0 and n == R.file_bytes(case).size
    groups = _complex_groups(case)
    assert groups
    for g, e in groups:
        with _lib.launch_trace() as tr:
            re, im = raw3_unpack(dev, g.table, g.C, g.P, g.S, g.B, n_bytes=n)
        assert tr.kernels == [KERNEL], tr.kernels
        _check(f"{case}/{g.descr}", re.cpu().numpy(), im.cpu().numpy(), e["real"], e["imag"])
    if case in ("edges", "mixed"):  # channel by channel: rows of odd S * B (edges), B = 3 as the plane's own width (mixed)
        g, e = groups[-1]
        odd = set()
        for ci in range(g.C):
            tab, S, B, want_re, want_im = _channel_alone(g, e, ci)
            odd.add((S * B) % 2)
            with _lib.launch_trace() as tr:
                re, im = raw3_unpack(dev, tab, 1, g.P, S, B, n_bytes=n)
            assert tr.kernels == [KERNEL]
            _check(f"{case}/channel {ci} alone", re.cpu().numpy(), im.cpu().numpy(), want_re, want_im)
        assert case != "edges" or odd == {0, 1}


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_long_rows_at_every_byte_offset(ep, shift):
    """The ``long`` file moved ``shift`` bytes back in its buffer: complex blocks at every offset mod 4 in rows where a lane
    takes several (unrolled) steps of the chunk loop."""
    from echopype_amd.convert.raw3_unpack import raw3_unpack

    (g, e), = _complex_groups("long")
    dev, n = ep.ops.upload_file_bytes(np.concatenate([np.zeros(shift, np.uint8), R.file_bytes("long")]))
    tab = g.table.copy()
    tab[:, 0] += shift
    assert {int(v) % 4 for v in tab[:, 0]} == {(2 + shift) % 4} and int(tab[0, 1]) == g.S == 1300 and g.B == 4
    assert g.S * g.B // 4 > 2 * 64 * 2  # more chunks than two unrolled steps of a wavefront
    re, im = raw3_unpack(dev, tab, g.C, g.P, g.S, g.B, n_bytes=n)
    _check(f"long+{shift}", re.cpu().numpy(), im.cpu().numpy(), e["real"], e["imag"])


def _launches():
    """(case, table, C, P, S, B, real, imag) of the launches the written-once test repeats under two sentinels."""
    out = []
    for case in ("fm", "mixed", "long"):
        g, e = _complex_groups(case)[-1]
        out.append((case, g.table, g.C, g.P, g.S, g.B, e["real"], e["imag"]))
    g, e = _complex_groups("edges")[0]
    for ci in range(g.C):
        tab, S, B, want_re, want_im = _channel_alone(g, e, ci)
        out.append((f"edges/{ci}", tab, 1, g.P, S, B, want_re, want_im))
    return out


def test_every_element_is_written_and_nothing_behind_the_outputs(ep):
    import torch

    from echopype_amd.convert.raw3_unpack import raw3_unpack

    devs = {}
    for what, tab, C, P, S, B, want_re, want_im in _launches():
        case = what.split("/")[0]
        if case not in devs:
            devs[case] = ep.ops.upload_file_bytes(R.file_bytes(case))
        dev, n = devs[case]
        count = C * P * S * B
        results = []
        for fill in SENTINELS:
            flats = [torch.full((count + GUARD,), fill, dtype=torch.int32, device=dev.device) for _ in range(2)]
            outs = tuple(f[:count].view(torch.float32).view(C, P, S, B) for f in flats)
            got = raw3_unpack(dev, tab, C, P, S, B, n_bytes=n, out=outs)
            assert got[0] is outs[0] and got[1] is outs[1]
            host = [f.cpu().numpy() for f in flats]
            for h in host:
                assert (h[count:] == fill).all(), f"{what}: the guard behind an output was written"
                assert not (h[:count] == fill).any(), f"{what}: an output element was never written"
            planes = [h[:count].view(np.float32).reshape(C, P, S, B) for h in host]
            _check(what, planes[0], planes[1], want_re, want_im)
            results.append(planes)
        for a, b in zip(*results):
            assert a.tobytes() == b.tobytes()


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(np.asarray(data, np.uint8).tobytes())
    return str(path)


def _all_bytes(ed):
    out = {}
    for gname in ed.group_paths:
        ds = ed[gname]
        for name, da in list(ds.data_vars.items()) + list(ds.coords.items()):
            v = np.asarray(da.values)
            out[gname, name] = (str(v.dtype), v.shape, v.astype(str).tobytes() if v.dtype.kind == "O" else v.tobytes())
    return out


def test_the_whole_call_depends_on_the_file_alone(ep, tmp_path):
    """``open_raw_ek80`` of ``mixed`` (three beam groups, both unpack kernels, the positions kernel) with every fresh device
    allocation pre-filled with either byte of ``BYTES``: identical bits in every variable, no band touched."""
    import torch

    from echopype_amd import _lib

    path = _write(tmp_path, "mixed.raw", R.file_bytes("mixed"))
    runs = []
    for byte in BYTES:
        with Poisoned(torch, ep.ops, byte) as p:
            with _lib.launch_trace() as tr:
                ed = ep.open_raw_ek80(path)
            got = _all_bytes(ed)
        n_out, _ = p.check()
        assert n_out >= 2 * 2 + 3  # two complex groups, the power group's three planes
        assert tr.kernels.count(KERNEL) == 2 and tr.kernels.count("raw0_unpack_kernel<power, float32 angles>") == 1
        assert tr.kernels.count("nmea_positions_kernel") == 1
        runs.append(got)
    assert runs[0].keys() == runs[1].keys()
    for key in runs[0]:
        assert runs[0][key] == runs[1][key], key
    want = R.expected_groups("mixed")
    for i, descr in enumerate(R.GROUP_ORDER):
        beam = ed[f"Sonar/Beam_group{i + 1}"]
        if descr == "power":
            assert np.array_equal(_bits(beam["backscatter_r"].values), _bits(want[descr]["power"]))
            assert np.array_equal(_bits(beam["angle_athwartship"].values), _bits(want[descr]["athw"]))
            assert np.array_equal(_bits(beam["angle_alongship"].values), _bits(want[descr]["along"]))
        else:
            _check(descr, beam["backscatter_r"].values, beam["backscatter_i"].values, want[descr]["real"], want[descr]["imag"])
    assert list(ed["Sonar"]["waveform_encode_descr"].values) == list(R.GROUP_ORDER)
    assert list(ed["Sonar"]["beam_group"].values) == ["Beam_group1", "Beam_group2", "Beam_group3"]


def test_arguments_are_checked_before_anything_is_launched(ep):
    import torch

    from echopype_amd import _lib
    from echopype_amd.convert.raw3_unpack import raw3_unpack

    (g, _), = _complex_groups("fm")
    dev, n = ep.ops.upload_file_bytes(R.file_bytes("fm"))
    args = (g.C, g.P, g.S, g.B)
    with _lib.launch_trace() as tr:
        t = g.table.copy()
        t[0, 0] = n - 8  # a block that leaves the file
        with pytest.raises(ValueError, match="leaves the"):
            raw3_unpack(dev, t, *args, n_bytes=n)
        t = g.table.copy()
        t[0, 1] = g.S + 1
        with pytest.raises(ValueError, match="count="):
            raw3_unpack(dev, t, *args, n_bytes=n)
        t = g.table.copy()
        t[0, 2] = g.B + 1
        with pytest.raises(ValueError, match="sectors, 0 .. B"):
            raw3_unpack(dev, t, *args, n_bytes=n)
        with pytest.raises(ValueError, match="sectors are served"):
            raw3_unpack(dev, np.tile([[-1, 0, 0]], (g.C * g.P, 1)), g.C, g.P, g.S, 9, n_bytes=n)
        with pytest.raises(ValueError, match="padded to a multiple of 16"):
            raw3_unpack(dev[:-8], g.table, *args, n_bytes=n - 16)
        with pytest.raises(ValueError, match="rows, C \\* P"):
            raw3_unpack(dev, g.table[:-1], *args, n_bytes=n)
        with pytest.raises(ValueError, match="out must hold"):
            raw3_unpack(dev, g.table, *args, n_bytes=n, out=(torch.empty(1, device=dev.device),) * 2)
    assert tr.kernels == []
    torch.cuda.synchronize()


# ---- the product ------------------------------------------------------------------------------------------------------
_synth = {}


def _synthetic(ep, waveform):
    """(dictionary of synth.ek80_numpy as the file holds it, file bytes), made once per waveform."""
    if waveform not in _synth:
        from echopype_amd import synth

        d = synth.ek80_numpy(C=2, P=4, S=300, B=4, waveform=waveform)
        d["backscatter_r"] = d["backscatter_r"].astype(np.float32)
        d["backscatter_i"] = d["backscatter_i"].astype(np.float32)
        d["tau"] = d["tau"].astype(np.float32).astype(np.float64)  # the reference stores the pulse duration as float32
        d["beam_type"] = np.ones(2, np.int64)
        _synth[waveform] = (d, R.synth_file(d, synth.ek80_filters(), waveform))
    return _synth[waveform]


def _same(a, b, what):
    a, b = np.asarray(a.values), np.asarray(b.values)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, a.shape, b.dtype, b.shape)
    assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("waveform,cal", [("BB", "Sv"), ("BB", "TS"), ("CW", "Sv"), ("CW", "TS")])
def test_calibration_of_open_raw_ek80_equals_that_of_the_same_arrays(ep, tmp_path, waveform, cal):
    from echopype_amd import synth
    from echopype_amd.xr_lite import is_device

    d, data = _synthetic(ep, waveform)
    ed = ep.open_raw_ek80(_write(tmp_path, f"{waveform}.raw", data))
    ref = ep.echodata.from_ek80_arrays(d, synth.ek80_filters())
    beam = ed["Sonar/Beam_group1"]
    assert ed.sonar_model == "EK80" and list(beam["channel"].values) == list(d["channel"])
    assert list(ed["Sonar"]["waveform_encode_descr"].values) == ["complex_FM" if waveform == "BB" else "complex_CW"]
    assert np.array_equal(beam["ping_time"].values, d["ping_time"]) and list(beam["beam"].values) == ["1", "2", "3", "4"]
    assert is_device(beam["backscatter_r"].data) and is_device(beam["backscatter_i"].data) and is_device(beam["sample_interval"].data)
    for name in ("backscatter_r", "backscatter_i"):
        got = beam[name].values
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(d[name]))
    for name in ("sample_interval", "transmit_duration_nominal", "transmit_power", "slope"):
        _same(beam[name], ref["Sonar/Beam_group1"][name], name)
    fn = ep.calibrate.compute_Sv if cal == "Sv" else ep.calibrate.compute_TS
    got, want = fn(ed, waveform_mode=waveform, encode_mode="complex"), fn(ref, waveform_mode=waveform, encode_mode="complex")
    _same(got[cal], want[cal], cal)
    _same(got["echo_range"], want["echo_range"], "echo_range")
    assert np.isfinite(np.asarray(got[cal].values)).any()
    if (waveform, cal) == ("BB", "Sv"):  # from a file on disk to MVBS, no float64 sample plane on the way up
        mv = ep.commongrid.compute_MVBS(got, range_bin="1m", ping_time_bin="2s")
        mv_ref = ep.commongrid.compute_MVBS(want, range_bin="1m", ping_time_bin="2s")
        _same(mv["Sv"], mv_ref["Sv"], "MVBS")


def test_splitbeam_angles_of_open_raw_ek80_equal_those_of_the_same_arrays(ep, tmp_path):
    from echopype_amd import synth

    d, data = _synthetic(ep, "BB")
    ed = ep.open_raw_ek80(_write(tmp_path, "BB.raw", data))
    ref = ep.echodata.from_ek80_arrays(d, synth.ek80_filters())
    out = []
    for e in (ed, ref):
        sv = ep.calibrate.compute_Sv(e, waveform_mode="BB", encode_mode="complex")
        out.append(ep.consolidate.add_splitbeam_angle(sv, e, "BB", "complex", pulse_compression=True, to_disk=False))
    for name in ("angle_alongship", "angle_athwartship"):
        _same(out[0][name], out[1][name], name)
        assert np.isfinite(np.asarray(out[0][name].values)).any()


def _power_reference(ep):
    """An EK80 EchoData with the power group of ``mixed`` from the REFERENCE-parsed arrays and dicts of the fixture."""
    from echopype_amd.echodata import EchoData
    from echopype_amd.xr_lite import Dataset

    e, cfg, env_j = R.expected_groups("mixed")["power"], R.golden_json("mixed", "config"), R.golden_json("mixed", "environment")
    ch, cp = e["channel"], ("channel", "ping_time")
    num = lambda key: np.array([[np.nan if v is None else float(v) for v in row] for row in e["params"][key]])  # noqa: E731
    beam = Dataset(coords={"channel": ch, "ping_time": e["ping_time"], "range_sample": np.arange(e["S"])})
    beam["backscatter_r"] = (cp + ("range_sample",), e["power"])
    beam["angle_athwartship"] = (cp + ("range_sample",), e["athw"])
    beam["angle_alongship"] = (cp + ("range_sample",), e["along"])
    beam["sample_interval"] = (cp, num("sample_interval"))
    beam["transmit_power"] = (cp, num("transmit_power"))
    beam["slope"] = (cp, num("slope"))
    beam["transmit_duration_nominal"] = (cp, num("pulse_duration").astype(np.float32).astype(np.float64))
    beam["transmit_type"] = (cp, np.full((e["C"], e["P"]), "CW"))
    one = lambda key, src=cfg: np.array([src[c][key] for c in ch], dtype=np.float64)  # noqa: E731
    beam["frequency_nominal"] = (("channel",), one("transducer_frequency"))
    beam["transmit_frequency_start"] = (("channel",), one("transducer_frequency"))
    beam["transmit_frequency_stop"] = (("channel",), one("transducer_frequency"))
    beam["beam_type"] = (("channel",), np.array([cfg[c]["transducer_beam_type"] for c in ch], dtype=np.int64))
    for out, src in (("equivalent_beam_angle",) * 2, ("angle_offset_alongship",) * 2, ("angle_offset_athwartship",) * 2,
                     ("angle_sensitivity_alongship",) * 2, ("angle_sensitivity_athwartship",) * 2,
                     ("beamwidth_twoway_alongship", "beam_width_alongship"), ("beamwidth_twoway_athwartship", "beam_width_athwartship")):
        beam[out] = (("channel",), one(src))
    allc = sorted(cfg)
    vend = Dataset(coords={"channel": allc, "pulse_length_bin": np.arange(5)})
    every = lambda key, dt=np.float64: np.array([cfg[c][key] for c in allc], dtype=dt)  # noqa: E731
    vend["frequency_nominal"] = (("channel",), every("transducer_frequency"))
    for out, src in (("sa_correction", "sa_correction"), ("gain_correction", "gain"), ("pulse_length", "pulse_duration")):
        vend[out] = (("channel", "pulse_length_bin"), every(src))
    vend["impedance_transceiver"] = (("channel",), every("impedance"))
    vend["receiver_sampling_frequency"] = (("channel",), every("rx_sample_frequency"))
    vend["transceiver_type"] = (("channel",), every("transceiver_type", str))
    env = Dataset(coords={"time1": np.array([env_j["timestamp"]], dtype="datetime64[ns]")})
    for out, src in (("sound_speed_indicative", "sound_speed"), ("temperature",) * 2, ("salinity",) * 2, ("depth",) * 2,
                     ("acidity",) * 2):
        env[out] = (("time1",), np.array([env_j[src]], dtype=np.float64))
    sonar = Dataset(coords={"beam_group": ["Beam_group1"]})
    sonar["waveform_encode_descr"] = (("beam_group",), np.array(["power"]))
    return EchoData("EK80", {"Sonar": sonar, "Sonar/Beam_group1": beam, "Vendor_specific": vend, "Environment": env},
                    source_file="mixed.raw")


def test_the_power_group_of_mixed_calibrates_like_the_reference_parse(ep, tmp_path):
    ed = ep.open_raw_ek80(_write(tmp_path, "mixed.raw", R.file_bytes("mixed")))
    ref = _power_reference(ep)
    # the filters and the environment are compared with the reference's parse below; here both sides share them, so that the
    # two calls differ in the samples and the per-ping parameters alone
    ref["Vendor_specific"], ref["Environment"] = ed["Vendor_specific"], ed["Environment"]
    assert ep.calibrate.calibrate_ek.retrieve_correct_beam_group(ed, "CW", "power") == "Sonar/Beam_group3"
    got = ep.calibrate.compute_Sv(ed, waveform_mode="CW", encode_mode="power")
    want = ep.calibrate.compute_Sv(ref, waveform_mode="CW", encode_mode="power")
    _same(got["Sv"], want["Sv"], "Sv")
    _same(got["echo_range"], want["echo_range"], "echo_range")
    assert np.isfinite(np.asarray(got["Sv"].values)).any()
    # the groups beside the samples: what the reference's parse holds
    env, env_j = ed["Environment"], R.golden_json("mixed", "environment")
    assert env["sound_speed_indicative"].values[0] == env_j["sound_speed"] and env["temperature"].values[0] == env_j["temperature"]
    mru, plat = R.golden_json("mixed", "mru0"), ed["Platform"]
    for name, key in (("pitch", "pitch"), ("roll", "roll"), ("vertical_offset", "heave"), ("heading", "heading")):
        assert np.array_equal(plat[name].values, np.array(mru[key], np.float64)), name
    assert np.array_equal(plat["time2"].values.astype(np.int64), np.array(mru["timestamp"], np.int64))
    assert float(plat["water_level"].values) == env_j["water_level_draft"]
    vend = ed["Vendor_specific"]
    assert list(vend["channel"].values) == sorted(R.golden_json("mixed", "config")) and vend["filter_time"].values.size == 1
    fil = R.golden_json("mixed", "fil")
    for f in fil:
        i, j = list(vend["channel"].values).index(f["channel_id"]), int(np.searchsorted(vend["filter_time"].values.astype(np.int64), f["time_ns"]))
        name = "WBT" if f["stage"] == 1 else "PC"
        row = vend[f"{name}_coeffs_real"].values[i, j]
        assert np.array_equal(row[:len(f["real"])], np.array(f["real"], np.float32).astype(np.float64)) and np.isnan(row[len(f["real"]):]).all()
        assert vend[f"{name}_deci_fac"].values[i, j] == f["decimation_factor"]
    assert str(vend["config_xml"].values).startswith("<?xml") and ed["Top-level"].attrs["keywords"] == "EK80"
    assert ed["Sonar"].attrs["sonar_model"] == "EK80" and list(ed["Provenance"]["source_filenames"].values) == ["mixed.raw"]


def test_fm_groups_carry_the_broadband_tables_and_the_sweep(ep, tmp_path):
    ed = ep.open_raw_ek80(_write(tmp_path, "fm.raw", R.file_bytes("fm")))
    beam, e = ed["Sonar/Beam_group1"], R.expected_groups("fm")["complex_FM"]
    _check("fm", beam["backscatter_r"].values, beam["backscatter_i"].values, e["real"], e["imag"])
    for name, key in (("transmit_frequency_start", "frequency_start"), ("transmit_frequency_stop", "frequency_end")):
        want = np.array([[float(v) for v in row] for row in e["params"][key]])
        assert np.array_equal(beam[name].values, want), name
    assert set(np.asarray(beam["transmit_type"].values).ravel()) == {"LFM"}
    off = np.array([[float(v) for v in row] for row in e["params"]["offset"]])
    si = np.array([[float(v) for v in row] for row in e["params"]["sample_interval"]])
    assert np.array_equal(beam["sample_time_offset"].values, off * si)
    tau = np.array([[float(v) for v in row] for row in e["params"]["pulse_duration"]])
    assert np.array_equal(beam["transmit_duration_nominal"].values, tau.astype(np.float32).astype(np.float64))
    vend, cal = ed["Vendor_specific"], R.golden_json("fm", "config")[R.CH120]["calibration"]
    assert list(vend["cal_channel_id"].values) == [R.CH120] and np.array_equal(vend["cal_frequency"].values, cal["frequency"])
    assert np.array_equal(vend["gain"].values[0], cal["gain"]) and np.array_equal(vend["impedance_transducer"].values[0], cal["impedance"])
    cfg = R.golden_json("fm", "config")
    assert np.array_equal(beam["transducer_offset_z"].values, [cfg[c]["transducer_offset_z"] for c in e["channel"]])
    assert list(beam["transceiver_software_version"].values) == [cfg[c]["transceiver_software_version"] for c in e["channel"]]


def test_positions_equal_the_host_rules_and_add_location_runs(ep, tmp_path):
    from echopype_amd.convert import parse_nmea

    ed = ep.open_raw_ek80(_write(tmp_path, "fm.raw", R.file_bytes("fm")))
    text, times = list(R.golden()["fm/nmea_text"]), R.golden()["fm/nmea_time"]
    sel = [i for i, s in enumerate(text) if len(s) >= 6 and s[3:6] in parse_nmea.TYPES]
    lat, lon, kind = parse_nmea.positions_host([text[i] for i in sel])
    plat = ed["Platform"]
    assert len(sel) >= 3 and np.array_equal(plat["time1"].values, times[sel])
    assert np.array_equal(plat["latitude"].values, lat, equal_nan=True) and np.array_equal(plat["longitude"].values, lon, equal_nan=True)
    assert list(plat["sentence_type"].values) == list(kind)
    assert list(ed["Platform/NMEA"]["NMEA_datagram"].values) == text
    sv = ep.calibrate.compute_Sv(ed, waveform_mode="BB", encode_mode="complex")
    out = ep.consolidate.add_location(sv, ed)
    # (the fixture's first GGA sentence has a one-digit checksum: its fix is NaN, and so is what is interpolated from it)
    assert np.asarray(out["latitude"].values).shape == (3,) and np.asarray(out["longitude"].values).shape == (3,)


def test_broken_and_cut_files_through_the_public_call(ep, tmp_path, caplog):
    for name, (data, exc, text) in R.bad_variants().items():
        with pytest.raises(exc, match=text):
            ep.open_raw_ek80(_write(tmp_path, f"{name}.raw", data))
    e = R.expected_groups("fm")["complex_FM"]
    for name, (data, _) in R.cut_variants().items():
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="echopype_amd.convert.api_ek80"):
            ed = ep.open_raw_ek80(_write(tmp_path, f"{name}.raw", data))
        assert any("ends inside a datagram" in r.getMessage() for r in caplog.records)
        want_re, want_im = e["real"].copy(), e["imag"].copy()
        want_re[1, 2], want_im[1, 2] = np.nan, np.nan  # the last RAW3: the 120 kHz channel's ping 2
        beam = ed["Sonar/Beam_group1"]
        _check(name, beam["backscatter_r"].values, beam["backscatter_i"].values, want_re, want_im)
        assert np.isnan(beam["sample_interval"].values[1, 2]) and np.isfinite(beam["sample_interval"].values[0]).all()
