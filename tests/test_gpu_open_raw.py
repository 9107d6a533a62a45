"""``open_raw`` (EK60) on a real MI355X: the unpack kernel alone, bit-equal to what the REFERENCE's parsers read and padded
from the same bytes (tests/golden/open_raw_ek60.npz); every output element written exactly once and nothing behind the
outputs touched; the product (``compute_Sv``, ``add_splitbeam_angle``, ``combine_echodata`` on what ``open_raw`` returns)
bit-equal to the same calls on an EchoData built from the reference-parsed arrays; cut and broken files.

There is no tolerance anywhere: power is ``float32(int16) * float32(10 log10(2) / 256)`` compared as int32 words, NaN is
NumPy's 0x7FC00000 exactly where the reference padded, angles are whole numbers."""
import logging

import numpy as np
import pytest

import raw_cases as R

pytestmark = pytest.mark.gpu

KERNELS = {None: "raw0_unpack_kernel<power>", "int8": "raw0_unpack_kernel<power, int8 angles>",
           "float32": "raw0_unpack_kernel<power, float32 angles>"}
NAN_BITS = np.int32(0x7FC00000)
SENTINEL_BITS = -559038737  # 0xDEADBEEF: no product of an int16 and no canonical NaN
GUARD = 64


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


def _plan(case):
    from echopype_amd.convert import parse_ek60

    return parse_ek60.plan(R.file_bytes(case))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_planes(case, angles, power, athw, along):
    e = R.expected(case)
    assert power.dtype == np.float32 and power.shape == (e["C"], e["P"], e["S"])
    bad = np.flatnonzero(_bits(power).ravel() != _bits(e["power"]).ravel())
    assert bad.size == 0, f"{case}: {bad.size} power words differ, first at {np.unravel_index(bad[0], power.shape)}"
    assert np.array_equal(_bits(power) == NAN_BITS, np.isnan(e["power"]))
    if angles is None:
        assert athw is None and along is None
        return
    for got, want in ((athw, e["athw"]), (along, e["along"])):
        assert got.shape == want.shape
        if angles == "int8":
            assert got.dtype == np.int8 and np.array_equal(got.astype(np.float32), want)
        else:
            assert got.dtype == np.float32 and np.array_equal(_bits(got) == NAN_BITS, np.isnan(want))
            assert np.array_equal(_bits(got), _bits(want))  # (whole numbers and one NaN pattern: words are comparable)


FORMS = [("aligned", "int8"), ("aligned", "float32"), ("aligned", None), ("ragged", "float32"), ("ragged", None),
         ("long", "float32"), ("long", None)]


@pytest.mark.parametrize("case,angles", FORMS)
def test_kernel_alone_is_bit_equal_to_the_reference_parse(ep, case, angles):
    from echopype_amd import _lib

    pl = _plan(case)
    dev, n = ep.ops.upload_file_bytes(R.file_bytes(case))
    assert dev.numel() % 16 == 0 and n == R.file_bytes(case).size
    with _lib.launch_trace() as tr:
        power, athw, along = ep.ops.raw0_unpack(dev, pl.table, pl.C, pl.P, pl.S, angles=angles, n_bytes=n)
    assert tr.kernels == [KERNELS[angles]], tr.kernels
    _check_planes(case, angles, power.cpu().numpy(), None if athw is None else athw.cpu().numpy(),
                  None if along is None else along.cpu().numpy())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_long_rows_at_every_byte_offset(ep, shift):
    """The ``long`` file moved ``shift`` bytes back in its buffer: sample blocks at every offset mod 4 in rows where a lane
    takes several (unrolled) steps -- both rows with float32 planes, and the first ping alone, which is full, with int8
    planes (16 samples per store: the only case whose int8 rows are longer than one step of a wavefront)."""
    pl, e = _plan("long"), R.expected("long")
    dev, n = ep.ops.upload_file_bytes(np.concatenate([np.zeros(shift, np.uint8), R.file_bytes("long")]))
    tab = pl.table.copy()
    tab[:, :2] += shift
    assert {int(v) % 4 for v in tab[:, 0]} == {shift % 4, (shift + 2) % 4} and int(tab[0, 2]) == pl.S == 5000
    power, athw, along = ep.ops.raw0_unpack(dev, tab, pl.C, pl.P, pl.S, angles="float32", n_bytes=n)
    _check_planes("long", "float32", power.cpu().numpy(), athw.cpu().numpy(), along.cpu().numpy())
    p8, a8, l8 = ep.ops.raw0_unpack(dev, tab[:1], 1, 1, pl.S, angles="int8", n_bytes=n)
    assert np.array_equal(_bits(p8.cpu().numpy()), _bits(e["power"][:, :1]))
    assert a8.dtype == __import__("torch").int8
    assert np.array_equal(a8.cpu().numpy().astype(np.float32), e["athw"][:, :1])
    assert np.array_equal(l8.cpu().numpy().astype(np.float32), e["along"][:, :1])


@pytest.mark.parametrize("case,angles", [("aligned", "int8"), ("ragged", "float32"), ("long", "float32")])
def test_every_element_is_written_and_nothing_behind_the_outputs(ep, case, angles):
    import torch

    pl = _plan(case)
    dev, n = ep.ops.upload_file_bytes(R.file_bytes(case))
    count = pl.C * pl.P * pl.S
    results = []
    for fill8 in (0x5A, -0x5B):  # two sentinels: an int8 element that nobody writes cannot equal the golden under both
        flats, outs = [], []
        for dt in (torch.float32,) + ((torch.int8,) * 2 if angles == "int8" else (torch.float32,) * 2):
            flat = torch.full((count + GUARD,), SENTINEL_BITS if dt == torch.float32 else fill8,
                              dtype=torch.int32 if dt == torch.float32 else torch.int8, device=dev.device)
            flats.append(flat)
            outs.append(flat[:count].view(dt).view(pl.C, pl.P, pl.S))
        ep.ops.raw0_unpack(dev, pl.table, pl.C, pl.P, pl.S, angles=angles, n_bytes=n, out=tuple(outs))
        host = [f.cpu().numpy() for f in flats]
        for h in host:
            guard = h[count:]
            assert (guard == (SENTINEL_BITS if h.dtype == np.int32 else fill8)).all(), "the guard behind an output was written"
            if h.dtype == np.int32:
                assert not (h[:count] == SENTINEL_BITS).any(), "an output element was never written"
        planes = [h[:count].view(np.float32 if h.dtype == np.int32 else np.int8).reshape(pl.C, pl.P, pl.S) for h in host]
        _check_planes(case, angles, *planes)
        results.append(planes)
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()


def test_arguments_are_checked_before_anything_is_launched(ep):
    import torch

    from echopype_amd import _lib

    pl = _plan("ragged")
    dev, n = ep.ops.upload_file_bytes(R.file_bytes("ragged"))
    with _lib.launch_trace() as tr:
        with pytest.raises(ValueError, match="int8 angle planes need"):
            ep.ops.raw0_unpack(dev, pl.table, pl.C, pl.P, pl.S, angles="int8", n_bytes=n)
        t = pl.table.copy()
        t[0, 0] = n - 1  # a block that leaves the file
        t[0, 2] = 2
        with pytest.raises(ValueError, match="leaves the"):
            ep.ops.raw0_unpack(dev, t, pl.C, pl.P, pl.S, angles=None, n_bytes=n)
        t = pl.table.copy()
        t[0, 2] = pl.S + 1
        with pytest.raises(ValueError, match="count="):
            ep.ops.raw0_unpack(dev, t, pl.C, pl.P, pl.S, angles=None, n_bytes=n)
        with pytest.raises(ValueError, match="padded to a multiple of 16"):
            ep.ops.raw0_unpack(dev[:-8], pl.table, pl.C, pl.P, pl.S, angles=None, n_bytes=n - 16)
        with pytest.raises(ValueError, match="angles must be"):
            ep.ops.raw0_unpack(dev, pl.table, pl.C, pl.P, pl.S, angles="float64")
    assert tr.kernels == []
    torch.cuda.synchronize()


# ---- the product ------------------------------------------------------------------------------------------------------
def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(np.asarray(data, np.uint8).tobytes())
    return str(path)


def _reference_echodata(ep, case):
    """An EchoData from the REFERENCE-parsed arrays of the fixture, through the package's existing builder."""
    e, cfg = R.expected(case), R.config(case)
    tx = [cfg["transceivers"][str(k)] for k in e["transceivers"]]
    d = {"channel": e["channel"], "ping_time": e["ping_time"], "backscatter_r": e["power"],
         "sample_interval": e["hdr"]["sample_interval"], "transmit_duration_nominal": e["hdr"]["pulse_length"],
         "transmit_power": e["hdr"]["transmit_power"], "sound_speed_indicative": e["hdr"]["sound_velocity"],
         "absorption_indicative": e["hdr"]["absorption_coefficient"],
         "frequency_nominal": [t["frequency"] for t in tx], "equivalent_beam_angle": [t["equivalent_beam_angle"] for t in tx],
         "pulse_length": np.array([t["pulse_length_table"] for t in tx]), "gain_correction": np.array([t["gain_table"] for t in tx]),
         "sa_correction": np.array([t["sa_correction_table"] for t in tx]),
         "beam_type": [t["beam_type"] for t in tx]}
    for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship", "angle_offset_athwartship"):
        d[k] = [t[k] for t in tx]
    if e["athw"] is not None:
        cast = (lambda a: a.astype(np.int8)) if e["angles_int8"] else (lambda a: a)
        d["angle_athwartship"], d["angle_alongship"] = cast(e["athw"]), cast(e["along"])
    return ep.echodata.from_ek60_arrays(d, source_file=f"{case}.raw")


def _same(a, b, what):
    a, b = np.asarray(a.values), np.asarray(b.values)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, a.shape, b.dtype, b.shape)
    assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("case", ["aligned", "ragged"])
def test_compute_sv_of_open_raw_equals_compute_sv_of_the_reference_parse(ep, tmp_path, case):
    from echopype_amd.xr_lite import is_device

    e = R.expected(case)
    ed = ep.open_raw(_write(tmp_path, f"{case}.raw", R.file_bytes(case)), "EK60")
    beam = ed["Sonar/Beam_group1"]
    assert ed.sonar_model == "EK60" and list(beam["channel"].values) == e["channel"]
    assert np.array_equal(beam["ping_time"].values, e["ping_time"]) and np.array_equal(beam["range_sample"].values, np.arange(e["S"]))
    assert is_device(beam["backscatter_r"].data) and is_device(beam["sample_interval"].data)
    _check_planes(case, "int8" if e["angles_int8"] else "float32", beam["backscatter_r"].values,
                  beam["angle_athwartship"].values, beam["angle_alongship"].values)
    for name, field in (("sample_interval", "sample_interval"), ("transmit_bandwidth", "bandwidth"),
                        ("transmit_duration_nominal", "pulse_length"), ("transmit_power", "transmit_power")):
        got = beam[name].values
        assert got.dtype == np.float64 and np.array_equal(got, e["hdr"][field], equal_nan=True), name
    assert np.array_equal(beam["sample_time_offset"].values, e["hdr"]["offset"] * e["hdr"]["sample_interval"], equal_nan=True)
    assert beam["data_type"].values.dtype == (np.int8 if case == "aligned" else np.float32)
    for g in ("Top-level", "Environment", "Platform", "Platform/NMEA", "Provenance", "Sonar", "Vendor_specific"):
        assert g in ed
    assert list(ed["Platform/NMEA"]["NMEA_datagram"].values) == list(R.golden()[f"{case}/nmea_text"]) or case == "aligned"
    assert list(ed["Provenance"]["source_filenames"].values) == [f"{case}.raw"]
    ref = _reference_echodata(ep, case)
    got_sv, want_sv = ep.calibrate.compute_Sv(ed), ep.calibrate.compute_Sv(ref)
    _same(got_sv["Sv"], want_sv["Sv"], "Sv")
    _same(got_sv["echo_range"], want_sv["echo_range"], "echo_range")
    assert np.isfinite(np.asarray(got_sv["Sv"].values)).any()


def test_splitbeam_angles_of_open_raw_equal_those_of_the_reference_parse(ep, tmp_path):
    ed = ep.open_raw(_write(tmp_path, "aligned.raw", R.file_bytes("aligned")), "ek60")
    ref = _reference_echodata(ep, "aligned")
    out = []
    for e in (ed, ref):
        sv = ep.calibrate.compute_Sv(e)
        out.append(ep.consolidate.add_splitbeam_angle(sv, e, waveform_mode="CW", encode_mode="power", to_disk=False))
    for name in ("angle_alongship", "angle_athwartship"):
        _same(out[0][name], out[1][name], name)
        assert np.isfinite(np.asarray(out[0][name].values)).all()


def test_combine_of_two_halves_equals_open_raw_of_the_whole(ep, tmp_path):
    b = R.file_bytes("aligned")
    off, size = R.frames("aligned")
    con_end = int(off[0]) + int(size[0]) + 4
    mid = int(off[5]) - 4  # CON0, then 8 RAW0: the first four are pings 0 and 1
    whole = ep.open_raw(_write(tmp_path, "whole.raw", b), "EK60")
    a = ep.open_raw(_write(tmp_path, "a.raw", b[:mid]), "EK60")
    c = ep.open_raw(_write(tmp_path, "b.raw", np.concatenate([b[:con_end], b[mid:]])), "EK60")
    both = ep.combine_echodata([a, c])
    bw, bb = whole["Sonar/Beam_group1"], both["Sonar/Beam_group1"]
    assert np.array_equal(bw["ping_time"].values, bb["ping_time"].values)
    for name in ("backscatter_r", "angle_athwartship", "angle_alongship", "sample_interval", "transmit_power", "data_type"):
        _same(bb[name], bw[name], name)
    _same(both["Environment"]["sound_speed_indicative"], whole["Environment"]["sound_speed_indicative"], "sound speed")


@pytest.mark.parametrize("name", sorted(R.cut_variants()))
def test_a_cut_file_keeps_its_pings_and_warns(ep, tmp_path, caplog, name):
    data, n_dgram = R.cut_variants()[name]
    path = _write(tmp_path, "cut.raw", data)
    if n_dgram == 1:
        with pytest.raises(ValueError, match="no RAW0 datagram with power"):
            ep.open_raw(path, "EK60")
        return
    with caplog.at_level(logging.WARNING, logger="echopype_amd.convert.api"):
        ed = ep.open_raw(path, "EK60")
    assert any("ends inside a datagram" in r.getMessage() for r in caplog.records)
    e = R.expected("aligned")
    want = e["power"].copy()
    want[0, 3] = np.nan  # the last datagram: transceiver 2 (first by id), ping 3
    got = ed["Sonar/Beam_group1"]["backscatter_r"].values
    assert np.array_equal(_bits(got), _bits(want))
    athw = ed["Sonar/Beam_group1"]["angle_athwartship"].values
    assert athw.dtype == np.float32 and np.isnan(athw[0, 3]).all() and np.array_equal(athw[1], e["athw"][1])


def test_broken_files_raise_the_named_exceptions(ep, tmp_path):
    for name, (data, where, _) in R.bad_variants().items():
        with pytest.raises(ValueError, match=f"byte offset {where}"):
            ep.open_raw(_write(tmp_path, f"{name}.raw", data), "EK60")
    with pytest.raises(ValueError, match="starts with a CON0 datagram"):
        ep.open_raw(_write(tmp_path, "nocon.raw", R.file_bytes("nocon")), "EK60")
    with pytest.raises(NotImplementedError, match="mode 2"):
        ep.open_raw(_write(tmp_path, "mode2.raw", R.file_bytes("mode2")), "EK60")
