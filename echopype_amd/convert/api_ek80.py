"""``open_raw_ek80``: a Simrad EK80 ``.raw`` file read into an :class:`~echopype_amd.echodata.EchoData` whose sample
volumes are unpacked ON the device (echopype convert/api.py:346-546 with parse_ek80 / set_groups_ek80).

The file goes over PCIe once, as it is on disk.  The complex samples of the ``RAW3`` datagrams -- float32 pairs, sector
by sector -- are written into the ``(channel, ping_time, range_sample, beam)`` volumes ``backscatter_r`` /
``backscatter_i`` of each complex beam group by one launch of ``epa_raw3_unpack`` (``convert.raw3_unpack``); the int16
power and int8 angle blocks of the power group go through ``ops.raw0_unpack``, the kernel of the EK60 reader, unchanged;
the positions come from the ``NME0`` sentences by ``ops.nmea_positions``, exactly the EK60 route.  The host work is the
framing walk, one gather of the ``RAW3`` headers and one parse per DISTINCT ``XML0`` text (``parse_ek80.plan``).

The entry point is a function of its own: ``open_raw(..., "EK80")`` keeps raising ``NotImplementedError`` (a test holds it
to that); routing ``open_raw`` here is a later change.

Beam groups, as set_groups_ek80.py:1124-1232: ``complex_FM`` (the pings of complex channels whose ``pulse_form`` is 1),
``complex_CW`` (``pulse_form`` 0; 5 falls in neither, as in the reference) and ``power`` (all pings of channels with a power
block), numbered ``Beam_group1..3`` in that order over those that exist; ``Sonar`` carries ``beam_group``,
``beam_group_descr`` and ``waveform_encode_descr``.  ``range_sample`` of a group runs to the largest count among the
group's own pings.

``Platform`` carries ``pitch``, ``roll``, ``vertical_offset`` and ``heading`` from ``MRU0`` on ``time2``, the fixes on
``time1``, ``water_level``, ``drop_keel_offset``, ``drop_keel_offset_is_manual``, ``water_level_draft_is_manual``, the
transducer offsets and ``frequency_nominal``.  Of set_groups_ek80.py:310-535 these are left out, nothing here reads
them: ``MRU_offset_*`` / ``MRU_rotation_*`` / ``position_offset_*`` (NaN there), the ``time3`` variables of ``MRU1``
(``latitude_mru1`` / ``longitude_mru1``) and ``sentence_type`` of ``IDX`` positions.  ``Environment`` leaves out
``sound_velocity_profile``; ``Vendor_specific`` is complete.

Deviations from the reference, all on purpose:

* the sample planes are float32, the values the file holds (the reference widens them to float64); an imaginary part
  equal to 0.0 is NaN, as there;
* no resynchronisation (see ``convert.api``); a file cut inside a datagram keeps the complete datagrams and warns;
* a ``RAW3`` without a parameter datagram in front raises ``ValueError`` (the reference: ``NameError``);
* float16 complex samples (``data_type & 4``; the reference cannot read them either), the transmit pulse of ``RAW4``,
  ``MRU1``, ``.bot`` / ``.idx`` files and ``use_swap`` are not built: ``RAW4`` and ``MRU1`` datagrams are skipped with one
  log line per file;
* ``sentence_type`` and the angle planes as in ``convert.api``.

No instrument-written EK80 file has been read yet: the test fixtures are packed by this project's own ``struct`` code
(tests/raw3_cases.py) and parsed back by the reference's parsers."""
import logging
import os

import numpy as np

from .. import ops
from ..utils.prov import echopype_prov_attrs
from ..xr_lite import DataArray, Dataset, DeviceArray
from ..echodata import EchoData
from . import parse_ek80
from .api import launch_positions, positions, read_file, set_fixes
from .raw3_unpack import raw3_unpack

logger = logging.getLogger(__name__)

BEAM_GROUP_DESCR = {
    "complex_FM": "contains FM-only complex backscatter data and other beam or channel-specific data.",
    "complex_CW": "contains CW-only complex backscatter data and other beam or channel-specific data.",
    "power": ("contains backscatter power (uncalibrated) and other beam or channel-specific data, including split-beam "
              "angle data when they exist."),
}
_CP = ("channel", "ping_time")
_CH = ("channel",)
_FATTRS = {"units": "Hz", "long_name": "Transducer frequency", "valid_min": 0.0, "standard_name": "sound_frequency"}


def _check_args(include_bot, include_idx, storage_options, use_swap):
    for name, value, is_default in (("include_bot", include_bot, include_bot is False), ("include_idx", include_idx, include_idx is False),
                                    ("storage_options", storage_options, storage_options is None or storage_options == {}),
                                    ("use_swap", use_swap, use_swap is False)):
        if not is_default:
            raise NotImplementedError(f"open_raw_ek80: {name}={value!r} is not built, only its default")


def host_plan(buf, n_bytes, raw_file="<memory>"):
    """``parse_ek80.plan`` with the log lines of ``open_raw_ek80``: a cut file, datagrams with the time stamp (0, 0), the
    ``RAW4`` and ``MRU1`` datagrams that are skipped."""
    pl = parse_ek80.plan(buf, n_bytes)
    if pl.n_consumed < n_bytes:
        logger.warning("%s ends inside a datagram: %d of %d bytes hold complete datagrams, the rest is dropped", raw_file,
                       pl.n_consumed, n_bytes)
    if pl.skipped_zero_time:
        logger.warning("%s: skipped %d datagram(s) with the time stamp (0, 0)", raw_file, pl.skipped_zero_time)
    if pl.raw4_count:
        logger.info("%s: skipped %d RAW4 datagram(s): the transmit pulse is not built", raw_file, pl.raw4_count)
    if pl.mru1_count:
        logger.info("%s: skipped %d MRU1 datagram(s): their positions are not built", raw_file, pl.mru1_count)
    return pl


def _config(pl, channels, key, dtype=np.float64, default=np.nan):
    return np.array([pl.config[c].get(key, default) for c in channels], dtype=dtype)


def _beam_group(pl, g, planes):
    """One beam group from the plan and its device planes (set_groups_ek80.py:536-750, 967-1068, 1124-1232)."""
    ch = g.channel
    coords = {"channel": ch, "ping_time": g.ping_time, "range_sample": np.arange(g.S)}
    if g.descr != "power":
        coords["beam"] = np.arange(1, g.B + 1).astype(str)
    beam = Dataset(coords=coords, attrs={"beam_mode": "vertical", "conversion_equation_t": "type_3"})
    freq = _config(pl, ch, "transducer_frequency")
    beam["frequency_nominal"] = (_CH, freq, _FATTRS)
    beam["beam_type"] = (_CH, _config(pl, ch, "transducer_beam_type", np.int64, 0), {"long_name": "type of transducer (0-single, 1-split)"})
    for out, src in (("beamwidth_twoway_alongship", "beam_width_alongship"), ("beamwidth_twoway_athwartship", "beam_width_athwartship"),
                     ("angle_offset_alongship",) * 2, ("angle_offset_athwartship",) * 2, ("angle_sensitivity_alongship",) * 2,
                     ("angle_sensitivity_athwartship",) * 2, ("equivalent_beam_angle",) * 2, ("transducer_offset_x",) * 2,
                     ("transducer_offset_y",) * 2, ("transducer_offset_z",) * 2):
        beam[out] = (_CH, _config(pl, ch, src))
    d = np.stack([_config(pl, ch, k) for k in ("transducer_alpha_x", "transducer_alpha_y", "transducer_alpha_z")])
    d[:, np.all(np.isclose(d, 0.0), axis=0)] = np.nan  # (0, 0, 0): no direction recorded (set_groups_ek80.py:560-568)
    for i, k in enumerate(("beam_direction_x", "beam_direction_y", "beam_direction_z")):
        beam[k] = (_CH, d[i])
    beam["transceiver_software_version"] = (_CH, _config(pl, ch, "transceiver_software_version", str, ""))
    beam["beam_stabilisation"] = ((), np.array(0, np.byte))
    beam["non_quantitative_processing"] = ((), np.array(0, np.int16))

    field = lambda key, dt=np.float64: parse_ek80.param_field(pl, key, dt)  # noqa: E731
    si = field("sample_interval")
    beam["sample_interval"] = (_CP, parse_ek80.per_ping(pl, g, si))
    beam["transmit_power"] = (_CP, parse_ek80.per_ping(pl, g, field("transmit_power")))
    beam["slope"] = (_CP, parse_ek80.per_ping(pl, g, field("slope")))
    # the pulse duration may be named pulse_length; the reference stores it as float32 (set_groups_ek80.py:970-977)
    tau = field("pulse_length") if any("pulse_length" in p for p in pl.params) else field("pulse_duration")
    beam["transmit_duration_nominal"] = (_CP, parse_ek80.per_ping(pl, g, tau.astype(np.float32).astype(np.float64)))
    beam["channel_mode"] = (_CP, parse_ek80.per_ping(pl, g, field("channel_mode").astype(np.int8), np.int8))
    form = field("pulse_form")
    name = np.where(np.isfinite(form) & (form >= 0) & (form < parse_ek80.PULSE_FORM_NAMES.size),
                    parse_ek80.PULSE_FORM_NAMES[np.clip(np.nan_to_num(form), 0, 5).astype(np.int64)], "")
    beam["transmit_type"] = (_CP, parse_ek80.per_ping(pl, g, name, np.dtype("U3")))
    beam["sample_time_offset"] = (_CP, parse_ek80.per_ping(pl, g, pl.headers["offset"].astype(np.float64) * si))
    if g.descr == "complex_FM":
        beam["transmit_frequency_start"] = (_CP, parse_ek80.per_ping(pl, g, field("frequency_start")))
        beam["transmit_frequency_stop"] = (_CP, parse_ek80.per_ping(pl, g, field("frequency_end")))
    elif g.descr == "power":
        beam["transmit_frequency_start"] = (_CH, freq.copy())
        beam["transmit_frequency_stop"] = (_CH, freq.copy())
    if g.descr == "power":
        power, athw, along = planes
        dims = ("channel", "ping_time", "range_sample")
        beam["backscatter_r"] = DataArray(DeviceArray(power), dims, attrs={"long_name": "Raw backscatter measurements (real part)",
                                                                            "units": "dB"})
        if athw is not None:
            beam["angle_athwartship"] = DataArray(DeviceArray(athw), dims, attrs={"long_name": "electrical athwartship angle"})
            beam["angle_alongship"] = DataArray(DeviceArray(along), dims, attrs={"long_name": "electrical alongship angle"})
    else:
        dims = ("channel", "ping_time", "range_sample", "beam")
        beam["backscatter_r"] = DataArray(DeviceArray(planes[0]), dims, attrs={"long_name": "Raw backscatter measurements (real part)",
                                                                                "units": "dB"})
        beam["backscatter_i"] = DataArray(DeviceArray(planes[1]), dims,
                                          attrs={"long_name": "Raw backscatter measurements (imaginary part)", "units": "dB"})
    return beam


def _vendor(pl):
    """``Vendor_specific`` (set_groups_ek80.py:1234-1518) over every channel of the configuration, sorted by id."""
    ch = sorted(pl.config)
    tables = {k: np.array([pl.config[c][k] for c in ch], dtype=np.float64) for k in ("pulse_duration", "sa_correction", "gain")}
    if not tables["pulse_duration"].shape == tables["sa_correction"].shape == tables["gain"].shape or tables["gain"].ndim != 2:
        raise ValueError("Narrowband calibration parameters dimension mismatch!")
    vend = Dataset(coords={"channel": ch, "pulse_length_bin": np.arange(tables["gain"].shape[1])})
    vend["frequency_nominal"] = (_CH, _config(pl, ch, "transducer_frequency"), _FATTRS)
    for out, src in (("sa_correction", "sa_correction"), ("gain_correction", "gain"), ("pulse_length", "pulse_duration")):
        vend[out] = (("channel", "pulse_length_bin"), tables[src])
    if all("impedance" in pl.config[c] for c in ch):
        vend["impedance_transceiver"] = (_CH, _config(pl, ch, "impedance"), {"units": "ohm", "long_name": "Transceiver impedance"})
    if all("rx_sample_frequency" in pl.config[c] for c in ch):
        vend["receiver_sampling_frequency"] = (_CH, np.array([float(pl.config[c]["rx_sample_frequency"]) for c in ch]),
                                               {"units": "Hz", "long_name": "Receiver sampling frequency"})
    if all("transceiver_type" in pl.config[c] for c in ch):
        vend["transceiver_type"] = (_CH, _config(pl, ch, "transceiver_type", str), {"long_name": "Transceiver type"})
    cal_ch = [c for c in ch if "calibration" in pl.config[c]]
    if cal_ch:  # the broadband tables over the union of their frequencies, NaN where a channel lacks one (an outer join)
        cal_f = np.unique(np.concatenate([pl.config[c]["calibration"]["frequency"] for c in cal_ch]))
        vend.coords["cal_channel_id"] = DataArray(np.array(cal_ch), ("cal_channel_id",), name="cal_channel_id")
        vend.coords["cal_frequency"] = DataArray(cal_f, ("cal_frequency",), name="cal_frequency",
                                                 attrs={"long_name": "Frequency of calibration parameter", "units": "Hz"})
        for key, _ in parse_ek80.CAL_FIELDS:
            a = np.full((len(cal_ch), cal_f.size), np.nan)
            for i, c in enumerate(cal_ch):
                cal = pl.config[c]["calibration"]
                a[i, np.searchsorted(cal_f, cal["frequency"])] = cal[key]
            vend["impedance_transducer" if key == "impedance" else key] = (("cal_channel_id", "cal_frequency"), a)
    # the filters over filter_time, NaN-padded to the longest (set_groups_ek80.py:1411-1518)
    ft = pl.filter_time
    vend.coords["filter_time"] = DataArray(ft, ("filter_time",), name="filter_time")
    for stage, name in ((1, "WBT"), (2, "PC")):
        n = max([c.size for (cid, st), sets in pl.fil.items() if st == stage for _, c, _ in sets], default=0)
        re, im = np.full((len(ch), ft.size, n), np.nan), np.full((len(ch), ft.size, n), np.nan)
        deci = np.full((len(ch), ft.size), np.nan)
        for (cid, st), sets in pl.fil.items():
            if st != stage or cid not in ch:
                continue
            for t, c, d in sets:
                i, j = ch.index(cid), int(np.searchsorted(ft, t))
                re[i, j], im[i, j] = np.nan, np.nan
                re[i, j, :c.size], im[i, j, :c.size], deci[i, j] = c.real, c.imag, d
        dims = ("channel", "filter_time", f"{name}_filter_n")
        vend[f"{name}_coeffs_real"] = (dims, re)
        vend[f"{name}_coeffs_imag"] = (dims, im)
        vend[f"{name}_deci_fac"] = (("channel", "filter_time"), deci)
    vend["config_xml"] = ((), np.array(pl.config_xml))
    return vend


def build_groups(pl, planes, source_file):
    """The groups of the EchoData from the plan and the device planes of every beam group (``planes[i]`` belongs to
    ``pl.groups[i]``); names, dims and dtypes of set_groups_ek80.py.  ``Platform`` gets its fixes from ``set_fixes``."""
    groups = {}
    for i, (g, p) in enumerate(zip(pl.groups, planes)):
        groups[f"Sonar/Beam_group{i + 1}"] = _beam_group(pl, g, p)

    env_t = np.array([pl.environment_time if pl.environment_time is not None else np.datetime64("NaT")], dtype="datetime64[ns]")
    env = Dataset(coords={"time1": env_t})
    for out, src in (("temperature",) * 2, ("depth",) * 2, ("acidity",) * 2, ("salinity",) * 2, ("sound_speed_indicative", "sound_speed"),
                     ("transducer_sound_speed",) * 2):
        if src in pl.environment:
            env[out] = (("time1",), np.array([pl.environment[src]], dtype=np.float64))
    for k in ("sound_velocity_source", "transducer_name"):
        if k in pl.environment:
            env[k] = (("time1",), np.array([pl.environment[k]]))

    ch = sorted(pl.config)
    plat = Dataset(coords={"channel": ch, "time2": pl.mru0_time if pl.mru0.size else np.array(["NaT"], dtype="datetime64[ns]")},
                   attrs={"platform_name": "", "platform_type": "", "platform_code_ICES": ""})
    for out, src in (("pitch", "pitch"), ("roll", "roll"), ("vertical_offset", "heave"), ("heading", "heading")):
        plat[out] = (("time2",), pl.mru0[src].astype(np.float64) if pl.mru0.size else np.array([np.nan]))
    plat["water_level"] = ((), np.float64(pl.environment.get("water_level_draft", np.nan)))
    for k in ("drop_keel_offset", "drop_keel_offset_is_manual", "water_level_draft_is_manual"):
        plat[k] = ((), np.float64(pl.environment.get(k, np.nan)))
    for k in ("transducer_offset_x", "transducer_offset_y", "transducer_offset_z"):
        plat[k] = (_CH, _config(pl, ch, k))
    plat["frequency_nominal"] = (_CH, _config(pl, ch, "transducer_frequency"), _FATTRS)

    if len(pl.nmea):
        nmea = Dataset(coords={"nmea_time": pl.nmea_time}, attrs={"description": "All NMEA sensor datagrams"})
        nmea["NMEA_datagram"] = (("nmea_time",), np.array(pl.nmea, dtype=str), {"long_name": "NMEA datagram"})
    else:  # (the reference: one NaN entry)
        nmea = Dataset(coords={"nmea_time": np.array(["NaT"], dtype="datetime64[ns]")},
                       attrs={"description": "All NMEA sensor datagrams"})
        nmea["NMEA_datagram"] = (("nmea_time",), np.array([np.nan]), {"long_name": "NMEA datagram"})

    any_cfg = pl.config[ch[0]] if ch else {}
    names = [f"Beam_group{i + 1}" for i in range(len(pl.groups))]
    sonar = Dataset(coords={"beam_group": names},
                    attrs={"sonar_manufacturer": "Simrad", "sonar_model": "EK80", "sonar_serial_number": "",
                           "sonar_software_name": "EK80", "sonar_software_version": any_cfg.get("application_version", ""),
                           "sonar_type": "echosounder"})
    sonar["beam_group_descr"] = (("beam_group",), np.array([BEAM_GROUP_DESCR[g.descr] for g in pl.groups]))
    sonar["waveform_encode_descr"] = (("beam_group",), np.array([g.descr for g in pl.groups]))

    name = os.path.basename(str(source_file))
    prov = Dataset(coords={"filenames": np.arange(1)}, attrs=echopype_prov_attrs("conversion"))
    prov["source_filenames"] = (("filenames",), np.array([name]))
    top = Dataset(attrs={"conventions": "CF-1.7, SONAR-netCDF4-1.0, ACDD-1.3", "keywords": "EK80",
                         "sonar_convention_authority": "ICES", "sonar_convention_name": "SONAR-netCDF4",
                         "sonar_convention_version": "1.0", "summary": "", "title": "", "survey_name": ""})
    groups.update({"Top-level": top, "Environment": env, "Platform": plat, "Platform/NMEA": nmea, "Provenance": prov,
                   "Sonar": sonar, "Vendor_specific": _vendor(pl)})
    return groups


def open_raw_ek80(raw_file, include_bot=False, include_idx=False, convert_params=None, storage_options=None, use_swap=False,
                  max_chunk_size="100MB"):
    """Read the EK80 file ``raw_file`` into an :class:`EchoData` whose sample variables are resident in HBM, as after
    ``EchoData.to_device()``: the complex planes of every complex beam group are written there by one launch each from the
    file's own bytes, the power group's planes by the kernel of the EK60 reader, the per-ping parameters are uploaded
    beside them.  The arguments are those of the reference's ``open_raw`` without ``sonar_model`` and ``xml_path``; anything
    but the defaults of ``include_bot``, ``include_idx``, ``storage_options`` and ``use_swap`` raises
    ``NotImplementedError``; ``convert_params`` and ``max_chunk_size`` have nothing to act on and are ignored.

    This is NOT reached through ``open_raw(..., "EK80")``, which keeps raising ``NotImplementedError``: routing ``open_raw``
    here is a later change.  See the module docstring for the scope and the deviations.

    ``ValueError``: the file does not start with an ``XML0`` Configuration datagram, holds no ping, a sample block leaves its
    datagram, a ping has no or another channel's parameter datagram in front, or the framing is broken (no
    resynchronisation).  ``NotImplementedError``: float16 complex samples.  A file cut inside a datagram keeps the pings in
    front and logs a warning."""
    import torch

    _check_args(include_bot, include_idx, storage_options, use_swap)
    if raw_file is None:
        raise FileNotFoundError("Please specify the path to the raw data file.")
    raw_file = os.fspath(raw_file)
    if not os.path.isfile(raw_file):
        raise FileNotFoundError(f"There is no file named {os.path.basename(raw_file)}")
    buf, n_bytes = read_file(raw_file)
    pl = host_plan(buf, n_bytes, raw_file)
    file_dev = ops.to_device(buf)  # the file as it is on disk, once
    planes = []
    for g in pl.groups:
        if g.descr == "power":
            planes.append(ops.raw0_unpack(file_dev, g.table, g.C, g.P, g.S, angles=g.angles, n_bytes=n_bytes))
        else:
            planes.append(raw3_unpack(file_dev, g.table, g.C, g.P, g.S, g.B, n_bytes=n_bytes))
    packed = launch_positions(pl, file_dev, n_bytes)  # the NMEA sentences, read where they lie between the sample blocks
    # the file's bytes are not needed behind the kernels: the allocator may hand the block out again once the stream has
    # passed this point
    file_dev.record_stream(torch.cuda.current_stream(file_dev.device))
    dev = file_dev.device
    del file_dev
    groups = build_groups(pl, planes, raw_file)
    ed = EchoData("EK80", groups, source_file=raw_file)
    ed = ed.to_device(dev, groups=tuple(k for k in groups if k.startswith("Sonar/Beam_group")) + ("Environment",))
    # the fixes last: their download waits for the file's upload and the kernels, which the host work above overlaps
    set_fixes(ed["Platform"], positions(pl, packed, raw_file))
    return ed
