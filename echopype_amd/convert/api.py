"""``open_raw`` for EK60: a Simrad ``.raw`` file read into an :class:`~echopype_amd.echodata.EchoData` whose sample
volumes are unpacked ON the device (echopype convert/api.py:346-546 with parse_ek60 / set_groups_ek60).

The file goes over PCIe once, as it is on disk -- int16 power and int8 angle pairs, 4 B per sample for both --, the
``(channel, ping_time, range_sample)`` volumes are written in HBM by one kernel (``ops.raw0_unpack``), and the only host
work is the walk over the datagram framing (``epa_raw_index``), one gather of the 84-byte ``RAW0`` headers and the
``CON0`` configuration.  The GGA / GLL / RMC sentences of the ``NME0`` datagrams are parsed into positions by a second
kernel on the same bytes (``ops.nmea_positions``, 17 bytes back per fix): ``Platform`` carries ``latitude``, ``longitude``
and ``sentence_type`` on ``time1``, which is what ``consolidate.add_location`` reads.  The rules are restated in
``parse_nmea`` (the reference calls ``pynmea2``, which has never been run against them); a sentence outside the plain
form the kernel decides goes through ``parse_nmea.parse_sentence`` on the host.  ``Platform/NMEA`` keeps every sentence.

Scope: EK60 (``CON0`` / ``RAW0`` / ``NME0``).  EK80 files are read by ``open_raw_ek80`` (:mod:`.api_ek80`), a function of
its own: ``open_raw(..., "EK80")`` raises ``NotImplementedError``.  AZFP, ``.bot`` / ``.idx`` files, ``use_swap`` and the
positions of ``MRU1`` / ``IDX`` datagrams are not built.

Deviations from the reference, all on purpose:

* ``sentence_type`` of a sentence that does not parse is ``""`` (the reference: a float NaN among strings), so the
  variable has one string dtype; its fix is NaN, NaN as there.  A file without a GGA / GLL / RMC sentence has one entry at
  the earliest ping time: NaN, NaN, ``""``;
* no resynchronisation -- a trailing datagram size that differs from the leading one, or a size below 16, raises
  ``ValueError`` with the byte offset (the reference searches for the next datagram).  A file that ends inside a
  datagram (cut while recording) keeps the complete datagrams in front and logs a warning, as there;
* ``backscatter_r`` is ``float32(int16) * float32(10 log10(2) / 256)``, rounded once.  Under NumPy 2 the reference's
  ``astype("float32") * INDEX2POWER`` promotes to float64 because ``INDEX2POWER`` is an ``np.float64``; the float32 product
  is what it stored under NumPy 1 and what its files hold;
* the angle planes are int8 when every row of every channel is present, full length and has angles, otherwise float32
  with NaN (the reference: float64 there; the values are whole numbers);
* ``data_type`` / ``channel_mode`` become float32 with NaN when a channel lacks a ping (xarray's promotion of int8);
* pings of mode 2 (angle only) raise ``NotImplementedError``.

No real instrument file has been read yet: the test fixtures are written by the reference's own datagram packers."""
import logging
import os

import numpy as np

from .. import ops
from ..echodata import BEAM1, EchoData
from ..utils.prov import echopype_prov_attrs
from ..xr_lite import DataArray, Dataset, DeviceArray
from . import parse_ek60, parse_nmea

logger = logging.getLogger(__name__)

BEAM_GROUP_DESCR = ("contains backscatter power (uncalibrated) and other beam or channel-specific data, including "
                    "split-beam angle data when they exist.")
_CP = ("channel", "ping_time")
_CPS = ("channel", "ping_time", "range_sample")
_CH = ("channel",)


def _check_args(sonar_model, xml_path, include_bot, include_idx, storage_options, use_swap):
    if not isinstance(sonar_model, str) or sonar_model.upper() != "EK60":
        raise NotImplementedError(f"open_raw reads EK60 files; sonar_model={sonar_model!r} is not built")
    for name, value, is_default in (("xml_path", xml_path, xml_path is None), ("include_bot", include_bot, include_bot is False),
                                    ("include_idx", include_idx, include_idx is False),
                                    ("storage_options", storage_options, storage_options is None or storage_options == {}),
                                    ("use_swap", use_swap, use_swap is False)):
        if not is_default:
            raise NotImplementedError(f"open_raw: {name}={value!r} is not built, only its default")


def read_file(raw_file):
    """-> (uint8 array whose length is a multiple of 16, zero behind the file's bytes; the file's length)."""
    n = os.path.getsize(raw_file)
    buf = np.zeros(max(16, -(-n // 16) * 16), dtype=np.uint8)
    with open(raw_file, "rb") as f:
        got = f.readinto(memoryview(buf)[:n]) if n else 0
    if got != n:
        raise OSError(f"{raw_file}: read {got} of {n} bytes")
    return buf, n


def host_plan(buf, n_bytes, raw_file="<memory>"):
    """``parse_ek60.plan`` with the warnings of ``open_raw``: a cut file, datagrams with the time stamp (0, 0)."""
    pl = parse_ek60.plan(buf, n_bytes)
    if pl.n_consumed < n_bytes:
        logger.warning("%s ends inside a datagram: %d of %d bytes hold complete datagrams, the rest is dropped", raw_file,
                       pl.n_consumed, n_bytes)
    if pl.skipped_zero_time:
        logger.warning("%s: skipped %d datagram(s) with the time stamp (0, 0)", raw_file, pl.skipped_zero_time)
    return pl


def _channel_vars(pl, name, dtype=np.float64):
    tx = pl.config["transceivers"]
    return np.array([tx[k][name] for k in pl.transceivers], dtype=dtype)


def launch_positions(pl, file_dev, n_bytes):
    """The positions kernel over the selected sentences of the plan, on the file's bytes in HBM -> one uint8 device tensor
    of 17 bytes per sentence (all latitudes, all longitudes, all status bytes: ONE download), None without a sentence."""
    import torch

    sel = pl.nmea_selected
    if sel.size == 0:
        return None
    n = int(sel.size)
    packed = torch.empty(17 * n, dtype=torch.uint8, device=file_dev.device)
    out = (packed[:8 * n].view(torch.float64), packed[8 * n:16 * n].view(torch.float64), packed[16 * n:])
    ops.nmea_positions(file_dev, np.stack([pl.nmea_offset[sel], pl.nmea_length[sel]], axis=1), n_bytes=n_bytes, out=out)
    return packed


def positions(pl, packed, raw_file="<memory>"):
    """(time1, latitude, longitude, sentence_type) of the Platform group from what ``launch_positions`` left: the kernel's
    answers, ``parse_nmea.parse_sentence`` for the sentences it did not decide, the reference's warning once per file
    and coordinate for a field that is no ``DDDMM.MMM`` (set_groups_base.py:204-215), the placeholder of a file without
    a selected sentence."""
    from .._lib import NMEA_INVALID, NMEA_LAT_FAILED, NMEA_LON_FAILED, NMEA_TYPE_MASK, NMEA_TYPE_SHIFT, NMEA_UNDECIDED

    if packed is None:
        return parse_nmea.placeholder(pl.ping_time)
    sel = pl.nmea_selected
    n = int(sel.size)
    host = packed.cpu().numpy()
    lat, lon, code = host[:8 * n].view(np.float64).copy(), host[8 * n:16 * n].view(np.float64).copy(), host[16 * n:]
    kind = np.where((code == NMEA_INVALID) | (code == NMEA_UNDECIDED), len(parse_nmea.TYPES),
                    (code & NMEA_TYPE_MASK) >> NMEA_TYPE_SHIFT)
    stype = np.array(parse_nmea.TYPES + ("",), dtype="<U3")[kind]
    lat_bad, lon_bad = (code & NMEA_LAT_FAILED) != 0, (code & NMEA_LON_FAILED) != 0
    decided = code != NMEA_UNDECIDED
    lat_bad &= decided
    lon_bad &= decided
    for i in np.flatnonzero(~decided):
        lat[i], lon[i], stype[i] = parse_nmea.parse_sentence(pl.nmea[sel[i]])
        if stype[i]:
            lat_bad[i], lon_bad[i] = np.isnan(lat[i]), np.isnan(lon[i])
    for name, bad, field in (("latitude", lat_bad, "lat"), ("longitude", lon_bad, "lon")):
        if bad.any():
            first = getattr(parse_nmea.split_sentence(pl.nmea[sel[int(np.flatnonzero(bad)[0])]]), field)
            logger.warning("%s: " + parse_nmea.WARNING[name], raw_file,
                           f"Geographic coordinate value '{first}' is not valid DDDMM.MMM")
    return pl.nmea_time[sel], lat, lon, stype


def build_groups(pl, power, athw, along, source_file):
    """The groups of the EchoData from the plan and the three device planes (names, dims and dtypes of
    set_groups_ek60.py and set_groups_base.set_nmea).  ``Platform`` gets its fixes from ``set_fixes``."""
    cfg, ch, pt, S = pl.config, list(pl.channel), pl.ping_time, pl.S
    freq = _channel_vars(pl, "frequency")
    fattrs = {"units": "Hz", "long_name": "Transducer frequency", "valid_min": 0.0, "standard_name": "sound_frequency"}

    beam = Dataset(coords={"channel": ch, "ping_time": pt, "range_sample": np.arange(S)},
                   attrs={"beam_mode": "vertical", "conversion_equation_t": "type_3"})
    beam["frequency_nominal"] = (_CH, freq, fattrs)
    beam["beam_type"] = (_CH, _channel_vars(pl, "beam_type", np.int64), {"long_name": "type of transducer (0-single, 1-split)"})
    for out, src in (("beamwidth_twoway_alongship", "beamwidth_alongship"), ("beamwidth_twoway_athwartship", "beamwidth_athwartship"),
                     ("angle_offset_alongship",) * 2, ("angle_offset_athwartship",) * 2,
                     ("angle_sensitivity_alongship",) * 2, ("angle_sensitivity_athwartship",) * 2,
                     ("equivalent_beam_angle",) * 2, ("gain_correction", "gain")):
        beam[out] = (_CH, _channel_vars(pl, src))
    d = np.stack([_channel_vars(pl, k) for k in ("dir_x", "dir_y", "dir_z")])
    d[:, np.all(np.isclose(d, 0.0), axis=0)] = np.nan  # (0, 0, 0): no direction recorded (set_groups_ek60.py:368-376)
    for i, k in enumerate(("beam_direction_x", "beam_direction_y", "beam_direction_z")):
        beam[k] = (_CH, d[i])
    beam["gpt_software_version"] = (_CH, _channel_vars(pl, "gpt_software_version", str))
    beam["transmit_frequency_start"] = (_CH, freq.copy())
    beam["transmit_frequency_stop"] = (_CH, freq.copy())
    beam["transmit_type"] = ((), np.array("CW"))
    beam["beam_stabilisation"] = ((), np.array(0, np.byte))
    beam["non_quantitative_processing"] = ((), np.array(0, np.int16))
    for out, src in (("sample_interval", "sample_interval"), ("transmit_bandwidth", "bandwidth"),
                     ("transmit_duration_nominal", "pulse_length"), ("transmit_power", "transmit_power")):
        beam[out] = (_CP, parse_ek60.per_ping(pl, src))
    beam["data_type"] = (_CP, parse_ek60.per_ping(pl, "mode", np.int8))
    beam["channel_mode"] = (_CP, parse_ek60.per_ping(pl, "transmit_mode", np.int8))
    beam["sample_time_offset"] = (_CP, parse_ek60.per_ping(pl, "offset") * parse_ek60.per_ping(pl, "sample_interval"))
    beam["backscatter_r"] = DataArray(DeviceArray(power), _CPS, attrs={"long_name": "Raw backscatter measurements (real part)",
                                                                        "units": "dB"})
    if athw is not None:
        beam["angle_athwartship"] = DataArray(DeviceArray(athw), _CPS, attrs={"long_name": "electrical athwartship angle"})
        beam["angle_alongship"] = DataArray(DeviceArray(along), _CPS, attrs={"long_name": "electrical alongship angle"})

    env = Dataset(coords={"channel": ch, "time1": pt})
    env["absorption_indicative"] = (("channel", "time1"), parse_ek60.per_ping(pl, "absorption_coefficient"),
                                    {"long_name": "Indicative acoustic absorption", "units": "dB/m", "valid_min": 0.0})
    env["sound_speed_indicative"] = (("channel", "time1"), parse_ek60.per_ping(pl, "sound_velocity"),
                                     {"long_name": "Indicative sound speed", "standard_name": "speed_of_sound_in_sea_water",
                                      "units": "m/s", "valid_min": 0.0})
    env["frequency_nominal"] = (_CH, freq.copy(), fattrs)

    vend = Dataset(coords={"channel": ch, "pulse_length_bin": np.arange(5)})
    vend["frequency_nominal"] = (_CH, freq.copy(), fattrs)
    tx = cfg["transceivers"]
    for out, src in (("sa_correction", "sa_correction_table"), ("gain_correction", "gain_table"),
                     ("pulse_length", "pulse_length_table")):
        vend[out] = (("channel", "pulse_length_bin"), np.array([tx[k][src] for k in pl.transceivers], dtype=np.float64))

    # Platform: motion of the first channel's pings on time2, in file order (set_groups_ek60.py:189-266)
    first = pl.header_row // pl.P == 0
    h0 = pl.headers[first]
    plat = Dataset(coords={"channel": ch, "time2": pl.header_time[first]},
                   attrs={"platform_name": "", "platform_type": "", "platform_code_ICES": ""})
    for out, src in (("pitch", "pitch"), ("roll", "roll"), ("vertical_offset", "heave")):
        plat[out] = (("time2",), h0[src].astype(np.float64))
    plat["water_level"] = ((), np.float64(h0["transducer_depth"][0]))
    for k in ("MRU_offset_x", "MRU_offset_y", "MRU_offset_z", "MRU_rotation_x", "MRU_rotation_y", "MRU_rotation_z",
              "position_offset_x", "position_offset_y", "position_offset_z"):
        plat[k] = ((), np.float64(np.nan))
    for out, src in (("transducer_offset_x", "pos_x"), ("transducer_offset_y", "pos_y"), ("transducer_offset_z", "pos_z")):
        plat[out] = (_CH, _channel_vars(pl, src))
    plat["frequency_nominal"] = (_CH, freq.copy(), fattrs)

    if len(pl.nmea):
        nmea = Dataset(coords={"nmea_time": pl.nmea_time}, attrs={"description": "All NMEA sensor datagrams"})
        nmea["NMEA_datagram"] = (("nmea_time",), np.array(pl.nmea, dtype=str), {"long_name": "NMEA datagram"})
    else:  # (the reference: one NaN entry)
        nmea = Dataset(coords={"nmea_time": np.array(["NaT"], dtype="datetime64[ns]")},
                       attrs={"description": "All NMEA sensor datagrams"})
        nmea["NMEA_datagram"] = (("nmea_time",), np.array([np.nan]), {"long_name": "NMEA datagram"})

    sonar = Dataset(coords={"beam_group": ["Beam_group1"]},
                    attrs={"sonar_manufacturer": "Simrad", "sonar_model": "EK60", "sonar_serial_number": "",
                           "sonar_software_name": cfg["sounder_name"], "sonar_software_version": cfg["version"],
                           "sonar_type": "echosounder"})
    sonar["beam_group_descr"] = (("beam_group",), np.array([BEAM_GROUP_DESCR]))

    name = os.path.basename(str(source_file))
    prov = Dataset(coords={"filenames": np.arange(1)}, attrs=echopype_prov_attrs("conversion"))
    prov["source_filenames"] = (("filenames",), np.array([name]))
    top = Dataset(attrs={"conventions": "CF-1.7, SONAR-netCDF4-1.0, ACDD-1.3", "keywords": "EK60",
                         "sonar_convention_authority": "ICES", "sonar_convention_name": "SONAR-netCDF4",
                         "sonar_convention_version": "1.0", "summary": "", "title": "",
                         "survey_name": cfg["survey_name"]})
    return {"Top-level": top, "Environment": env, "Platform": plat, "Platform/NMEA": nmea, "Provenance": prov,
            "Sonar": sonar, BEAM1: beam, "Vendor_specific": vend}


def set_fixes(plat, fixes):
    """``latitude``, ``longitude`` and ``sentence_type`` on ``time1`` into the Platform group: the fixes of the GGA / GLL / RMC
    sentences (set_groups_ek60.py:182-210; the attributes are those of the convention's ``platform_var_default`` and
    ``platform_coord_default``, restated)."""
    time1, lat, lon, sentence_type = fixes
    plat.coords["time1"] = DataArray(np.asarray(time1, dtype="datetime64[ns]"), ("time1",), name="time1",
                                     attrs={"axis": "T", "long_name": "Timestamps for NMEA datagrams", "standard_name": "time",
                                            "comment": "Time coordinate corresponding to NMEA position data."})
    plat["latitude"] = (("time1",), np.asarray(lat, dtype=np.float64),
                        {"long_name": "Platform latitude", "standard_name": "latitude", "units": "degrees_north",
                         "valid_range": (-90.0, 90.0)})
    plat["longitude"] = (("time1",), np.asarray(lon, dtype=np.float64),
                         {"long_name": "Platform longitude", "standard_name": "longitude", "units": "degrees_east",
                          "valid_range": (-180.0, 180.0)})
    plat["sentence_type"] = (("time1",), np.asarray(sentence_type, dtype=str), {"long_name": "NMEA sentence type"})


def open_raw(raw_file, sonar_model, xml_path=None, include_bot=False, include_idx=False, convert_params=None,
             storage_options=None, use_swap=False, max_chunk_size="100MB"):
    """Read the EK60 file ``raw_file`` into an :class:`EchoData` whose sample variables are resident in HBM, as after
    ``EchoData.to_device()``: ``backscatter_r`` and the angle planes are written there by one kernel from the file's
    own bytes, the per-ping parameters are uploaded beside them.  The signature is the reference's; anything but
    ``sonar_model="EK60"`` (any letter case) and the defaults of ``xml_path``, ``include_bot``, ``include_idx``,
    ``storage_options`` and ``use_swap`` raises ``NotImplementedError``; ``convert_params`` and ``max_chunk_size`` have
    nothing to act on and are ignored.  See the module docstring for the scope and the deviations.

    EK80 files are NOT read through this function: ``sonar_model="EK80"`` raises ``NotImplementedError`` like every other
    model, and ``open_raw_ek80`` is the entry point for them.  Routing ``open_raw`` there is a later change.

    ``ValueError``: the file does not start with ``CON0``, holds no ping with power, or its framing is broken (no
    resynchronisation).  A file cut inside a datagram keeps the pings in front and logs a warning."""
    import torch

    _check_args(sonar_model, xml_path, include_bot, include_idx, storage_options, use_swap)
    if raw_file is None:
        raise FileNotFoundError("Please specify the path to the raw data file.")
    raw_file = os.fspath(raw_file)
    if not os.path.isfile(raw_file):
        raise FileNotFoundError(f"There is no file named {os.path.basename(raw_file)}")
    buf, n_bytes = read_file(raw_file)
    pl = host_plan(buf, n_bytes, raw_file)
    file_dev = ops.to_device(buf)  # the file as it is on disk, once
    power, athw, along = ops.raw0_unpack(file_dev, pl.table, pl.C, pl.P, pl.S, angles=pl.angles, n_bytes=n_bytes)
    packed = launch_positions(pl, file_dev, n_bytes)  # the NMEA sentences, read where they lie between the sample blocks
    # the file's bytes are not needed behind the kernels: the allocator may hand the block out again once the stream has
    # passed this point
    file_dev.record_stream(torch.cuda.current_stream(file_dev.device))
    del file_dev
    ed = EchoData("EK60", build_groups(pl, power, athw, along, raw_file), source_file=raw_file)
    ed = ed.to_device(power.device)
    # the fixes last: their download waits for the file's upload and both kernels, which the host work above overlaps
    set_fixes(ed["Platform"], positions(pl, packed, raw_file))
    return ed
