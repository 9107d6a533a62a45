"""Everything of ``open_raw_ek80`` that needs no device: the framing walk (``parse_ek60.raw_index``), the ``XML0``
configuration, parameter and environment datagrams, the ``RAW3`` headers of all pings in one gather, the ``FIL1`` filters,
the ``MRU0`` motion records, the beam groups and the row tables the unpack kernels read (echopype
convert/utils/ek_raw_parsers.py:764-1064,1135-1203,1653-1769, parse_base.py:360-650, set_groups_ek80.py:1124-1232).

Nothing here loops over pings in Python.  The records come from the C walk as one structured array; the 152-byte ``RAW3``
headers and the 28-byte ``MRU0`` bodies are gathered with one fancy index each and viewed through a structured dtype; the
``XML0`` parameter datagrams -- one in front of every ping, byte-identical for thousands of pings of a channel -- are
gathered by size, reduced with ``np.unique`` and parsed once per distinct text (``parse_xml_text``)."""
import logging
import re
import xml.etree.ElementTree as ET
from collections import Counter

import numpy as np

from .. import _lib
from . import parse_nmea
from .parse_ek60 import nmea_sentences, nt_to_ns, raw_index

logger = logging.getLogger(__name__)

RAW3_DTYPE = np.dtype([("type", "S4"), ("low_date", "<u4"), ("high_date", "<u4"), ("channel_id", "S128"), ("data_type", "<i2"),
                       ("spare", "S2"), ("offset", "<i4"), ("count", "<i4")])
RAW3_HEADER = 152
FIL1_DTYPE = np.dtype([("type", "S4"), ("low_date", "<u4"), ("high_date", "<u4"), ("stage", "<i2"), ("spare", "S2"),
                       ("channel_id", "S128"), ("n_coefficients", "<i2"), ("decimation_factor", "<i2")])
FIL1_HEADER = 148
MRU0_DTYPE = np.dtype([("type", "S4"), ("low_date", "<u4"), ("high_date", "<u4"), ("heave", "<f4"), ("roll", "<f4"),
                       ("pitch", "<f4"), ("heading", "<f4")])
MRU0_SIZE = 28
assert RAW3_DTYPE.itemsize == RAW3_HEADER and FIL1_DTYPE.itemsize == FIL1_HEADER and MRU0_DTYPE.itemsize == MRU0_SIZE
XML_HEADER = 12
MAX_BEAMS = 8  # kMaxBeams of csrc/ek80_complex.hip: what the calibrators take

# XML attribute -> (type, key or "" for the snake-case form of the attribute, separator of a list or "")
# (ek_raw_parsers.py:764-836, restated)
CHANNEL_OPTIONS = {"MaxTxPowerTransceiver": (int, "", ""), "PulseDuration": (float, "", ";"),
                   "PulseDurationFM": (float, "pulse_duration_fm", ";"), "SampleInterval": (float, "", ";"),
                   "ChannelID": (str, "channel_id", ""), "HWChannelConfiguration": (str, "hw_channel_configuration", "")}
TRANSCEIVER_OPTIONS = {"TransceiverNumber": (int, "", ""), "Version": (str, "transceiver_version", ""),
                       "IPAddress": (str, "ip_address", ""), "Impedance": (int, "", "")}
TRANSDUCER_OPTIONS = {"SerialNumber": (str, "transducer_serial_number", ""), "Frequency": (float, "transducer_frequency", ""),
                      "FrequencyMinimum": (float, "transducer_frequency_minimum", ""),
                      "FrequencyMaximum": (float, "transducer_frequency_maximum", ""), "BeamType": (int, "transducer_beam_type", ""),
                      "Gain": (float, "", ";"), "SaCorrection": (float, "", ";"), "MaxTxPowerTransducer": (float, "", ""),
                      "EquivalentBeamAngle": (float, "", ""), "BeamWidthAlongship": (float, "", ""),
                      "BeamWidthAthwartship": (float, "", ""), "AngleSensitivityAlongship": (float, "", ""),
                      "AngleSensitivityAthwartship": (float, "", ""), "AngleOffsetAlongship": (float, "", ""),
                      "AngleOffsetAthwartship": (float, "", ""),
                      "DirectivityDropAt2XBeamWidth": (float, "directivity_drop_at_2x_beam_width", ""),
                      "TransducerOffsetX": (float, "", ""), "TransducerOffsetY": (float, "", ""), "TransducerOffsetZ": (float, "", ""),
                      "TransducerAlphaX": (float, "", ""), "TransducerAlphaY": (float, "", ""), "TransducerAlphaZ": (float, "", "")}
HEADER_OPTIONS = {"Version": (str, "application_version", "")}
ENV_TRANSDUCER_OPTIONS = {"SoundSpeed": (float, "transducer_sound_speed", "")}
ENVIRONMENT_OPTIONS = {"Depth": (float, "", ""), "Acidity": (float, "", ""), "Salinity": (float, "", ""), "SoundSpeed": (float, "", ""),
                       "Temperature": (float, "", ""), "Latitude": (float, "", ""), "SoundVelocityProfile": (float, "", ";"),
                       "DropKeelOffset": (float, "", ""), "DropKeelOffsetIsManual": (int, "", ""),
                       "WaterLevelDraft": (float, "", ""), "WaterLevelDraftIsManual": (int, "", "")}
PARAMETER_OPTIONS = {"ChannelID": (str, "channel_id", ""), "ChannelMode": (int, "", ""), "PulseForm": (int, "", ""),
                     "Frequency": (float, "", ""), "PulseDuration": (float, "", ""), "SampleInterval": (float, "", ""),
                     "TransmitPower": (float, "", ""), "Slope": (float, "", "")}
CAL_FIELDS = (("gain", "Gain"), ("impedance", "Impedance"), ("phase", "Phase"), ("beamwidth_alongship", "BeamWidthAlongship"),
              ("beamwidth_athwartship", "BeamWidthAthwartship"), ("angle_offset_alongship", "AngleOffsetAlongship"),
              ("angle_offset_athwartship", "AngleOffsetAthwartship"))
# the transceiver's number inside a channel id (ek_raw_parsers.py:22)
CHANNEL_NUMBER = re.compile(r"\d{6}-\w{1,2}|\w{12}-\w{1,2}")
DROP_KEEL_ONLY = {"drop_keel_offset", "drop_keel_offset_is_manual"}
GROUP_ORDER = ("complex_FM", "complex_CW", "power")
PULSE_FORM_NAMES = np.array(["CW", "LFM", "", "", "", "FMD"])


def snake_case(name):
    """``TransducerAlphaX`` -> ``transducer_alpha_x``: an underscore in front of every capital but the first letter
    (utils/misc.py:9-21, so ``ChannelID`` gives ``channel_i_d``)."""
    return "".join("_" + c if c.isupper() and i else c for i, c in enumerate(name)).lower()


def _add(attrib, out, options):
    """The attributes of one XML element into ``out`` by the rules of ``options`` (ek_raw_parsers.py:852-896): a value with
    a separator becomes a list whose entries are converted where they convert; one without is converted or raises."""
    for k, v in attrib.items():
        if k not in options:
            out[snake_case(k)] = v
            continue
        kind, key, sep = options[k]
        if sep:
            val = []
            for item in v.split(sep):
                try:
                    val.append(kind(item))
                except (TypeError, ValueError):
                    val.append(item)
        else:
            val = kind(v)
        out[key or snake_case(k)] = val


def parse_configuration(root):
    """The ``Configuration`` element -> {channel id: dict}, as ``SimradXMLParser`` gives it (ek_raw_parsers.py:935-1064)."""
    out = {}
    xducers = root.find("Transducers")
    header = root.find("Header")
    for tcvr in root.iter("Transceiver"):
        for ch in tcvr.iter("Channel"):
            cid = ch.attrib["ChannelID"]
            d = out[cid] = {}
            _add(tcvr.attrib, d, TRANSCEIVER_OPTIONS)
            _add(ch.attrib, d, CHANNEL_OPTIONS)
            if len(list(ch)) > 1:  # (the reference builds a ValueError here and does not raise it: the channel gets no transducer)
                continue
            x = ch.find("Transducer")
            fpar = x.findall("FrequencyPar")
            if fpar:
                cal = {"frequency": np.array([int(f.attrib["Frequency"]) for f in fpar])}
                for key, attr in CAL_FIELDS:
                    cal[key] = np.array([float(f.attrib[attr]) for f in fpar])
                d["calibration"] = cal
            _add(x.attrib, d, TRANSDUCER_OPTIONS)
            if xducers is not None:  # the mounting of the transducer this channel drives
                m = CHANNEL_NUMBER.search(cid)
                if m is None:
                    raise ValueError(f"channel id {cid!r} holds no transceiver number to match the Transducers section with")
                names = Counter(t.attrib["TransducerName"] for t in xducers.iter("Transducer"))
                for t in xducers.iter("Transducer"):
                    a = t.attrib
                    by_name = a["TransducerName"] == x.attrib["TransducerName"]
                    by_sn = a["TransducerSerialNumber"] != "" and a["TransducerSerialNumber"] == x.attrib["SerialNumber"]
                    by_number = m[0] in a["TransducerCustomName"]
                    if (by_sn or by_number) if names[a["TransducerName"]] > 1 else (by_name or by_sn or by_number):
                        _add(a, d, TRANSDUCER_OPTIONS)
                        break
            _add(header.attrib, d, HEADER_OPTIONS)
    return out


def parse_xml_text(raw):
    """The text of one ``XML0`` datagram (the bytes behind its 12-byte header) -> (subtype, dict, text).  ``subtype`` is the
    root tag in lower case; the dict is filled for ``configuration``, ``parameter`` and ``environment`` and empty for every
    other subtype.  ``plan`` calls this once per DISTINCT text of a file."""
    text = str(bytes(raw).strip(b"\x00"), "ascii", errors="replace")
    root = ET.fromstring(text)
    subtype, d = root.tag.lower(), {}
    if subtype == "configuration":
        d = parse_configuration(root)
    elif subtype == "parameter":
        for ch in root.iter("Channel"):
            _add(ch.attrib, d, PARAMETER_OPTIONS)
    elif subtype == "environment":
        for e in root.iter("Environment"):
            _add(e.attrib, d, ENVIRONMENT_OPTIONS)
        for t in root.iter("Transducer"):
            _add(t.attrib, d, ENV_TRANSDUCER_OPTIONS)
    return subtype, d, text


def _gather(buf, offsets, width):
    """``width`` bytes at each of ``offsets`` -> uint8 (n, width): one fancy index over every window of the file."""
    if len(offsets) == 0:
        return np.zeros((0, width), np.uint8)
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(buf, width)[np.asarray(offsets, dtype=np.int64)])


def _headers(buf, records, dtype, what):
    short = records["size"] < dtype.itemsize
    if np.any(short):
        bad = records[short][0]
        raise ValueError(f"{what} datagram at byte offset {int(bad['offset'])} has {int(bad['size'])} bytes, fewer than its "
                         f"{dtype.itemsize}-byte header")
    return _gather(buf, records["offset"], dtype.itemsize).view(dtype).reshape(-1)


def unique_xml(buf, records):
    """The ``XML0`` datagrams ``records`` -> (uid int64 per record, list of parsed distinct texts): the records are grouped
    by size, each group gathered with one fancy index and reduced with ``np.unique(axis=0)``; ``parse_xml_text`` runs once
    per distinct text."""
    uid = np.empty(records.size, dtype=np.int64)
    parsed = []
    width = records["size"].astype(np.int64) - XML_HEADER
    if np.any(width < 0):
        raise ValueError(f"XML0 datagram at byte offset {int(records['offset'][width < 0][0])} is shorter than its header")
    for w in np.unique(width).tolist():  # (distinct sizes, not datagrams)
        sel = np.flatnonzero(width == w)
        if w == 0:
            raise ValueError(f"XML0 datagram at byte offset {int(records['offset'][sel[0]])} holds no text")
        texts, first, inv = np.unique(_gather(buf, records["offset"][sel] + XML_HEADER, w), axis=0, return_index=True,
                                      return_inverse=True)
        uid[sel] = len(parsed) + np.asarray(inv).reshape(-1)
        for t, i in zip(texts, sel[first].tolist()):
            try:
                parsed.append(parse_xml_text(t.tobytes()))
            except ET.ParseError as e:
                raise ValueError(f"XML0 datagram at byte offset {int(records['offset'][i])} does not parse: {e}") from None
    return uid, parsed


def _clean_ids(raw_ids):
    """S128 channel id fields -> (index of each into the distinct ids, the distinct ids as text): NULs stripped, ``"\\x00t"``
    removed (ek_raw_parsers.py:1721, parse_base.py:506)."""
    distinct, inv = np.unique(raw_ids, return_inverse=True)
    text = [bytes(b).decode("latin_1").strip("\x00").replace("\x00t", "") for b in distinct.tolist()]
    return np.asarray(inv).reshape(-1), text


class Ek80Group:
    """One beam group of the plan: ``descr`` (``complex_FM`` / ``complex_CW`` / ``power``), ``channel`` (ids, sorted),
    ``ping_time``, ``C, P, S`` and ``B`` (complex), ``ping`` (indices into the plan's pings, file order), ``row`` (their
    row ``c * P + p``), ``table`` and, for the power group, ``angles`` (see ``plan``)."""


class Ek80Plan:
    """What ``plan`` found: the attributes are documented there."""


def plan(buf, n_bytes=None):
    """The host half of ``open_raw_ek80``: ``buf`` (uint8 array, the file) -> an :class:`Ek80Plan` with

    ``n_consumed``       bytes of complete datagrams (less than the file: it was cut there)
    ``records``          every datagram's record; ``skipped_zero_time``: how many carried the time stamp (0, 0)
    ``config``           {channel id: dict} of the configuration datagram (``parse_configuration``), ``EC150`` channels
                         dropped; ``config_xml`` its text, ``config_time`` its time stamp
    ``environment``      the dict of the last environment datagram whose keys are not just the two drop-keel fields ({}
                         without one), ``environment_time`` its time stamp
    ``xml_texts``        how many distinct ``XML0`` texts were parsed; ``xml_count``: how many such datagrams there are
    ``headers``          the ``RAW3`` headers that count (EC150 dropped), file order; ``ping_channel`` (their channel id),
                         ``ping_time_all``, ``ping_param`` (index of each ping's parameter text into ``params``) and
                         ``params`` (the distinct parameter dicts)
    ``count, n_complex, has_power, has_angle``   per ping, from the header
    ``off_power, off_angle, off_complex``        per ping: byte offset of the block, -1 without one
    ``groups``           the beam groups that exist, in the order complex_FM, complex_CW, power (:class:`Ek80Group`).  A
                         complex group's ``table`` is int64 (C * P, 3): byte offset of the complex block (-1: no datagram,
                         or one without complex samples), count, sectors of the ping.  The power group's is the table of
                         ``ops.raw0_unpack`` (offset of the power block, of the angle block, count) with the angle rule of
                         ``parse_ek60.plan``, and ``angles`` is None, "int8" or "float32" as there
    ``fil``              {(channel id, stage): [(time, complex64 coefficients, decimation factor), ...]}, ``filter_time``
    ``mru0``             structured array of the MRU0 bodies, ``mru0_time``
    ``raw4_count, mru1_count``   datagrams skipped
    ``nmea_time, nmea, nmea_offset, nmea_length, nmea_selected``   as ``parse_ek60.plan``

    ``ValueError``: no configuration ``XML0`` in front, no ping, a block that leaves its datagram (with the byte offset), a
    ping without a parameter datagram in front, a parameter datagram of another channel in front of a ping ("Parameter ID
    does not match RAW"), a ping time twice in one channel; ``NotImplementedError``: float16 complex samples."""
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    out = Ek80Plan()
    rec, out.n_consumed = raw_index(buf, n_bytes)
    out.records = rec
    if rec.size == 0 or rec["type"][0] != b"XML0":
        got = rec["type"][0].decode("latin_1") if rec.size else "nothing"
        raise ValueError(f"an EK80 .raw file starts with an XML0 Configuration datagram, this one with {got}")
    zero = (rec["flags"] & _lib.RAW_ZERO_TIME) != 0
    out.skipped_zero_time = int(zero[1:].sum())
    live_idx = np.concatenate([[0], 1 + np.flatnonzero(~zero[1:])])
    live = rec[live_idx]
    rtime = nt_to_ns(live["low_date"], live["high_date"])

    # ---- XML0: configuration, parameter, environment ----
    is_xml = np.flatnonzero(live["type"] == b"XML0")
    uid, parsed = unique_xml(buf, live[is_xml])
    out.xml_texts, out.xml_count = len(parsed), int(is_xml.size)
    subtype = np.array([p[0] for p in parsed])
    first = parsed[uid[0]]
    if first[0] != "configuration":
        raise ValueError(f"an EK80 .raw file starts with an XML0 Configuration datagram, this one with an XML0 <{first[0]}>")
    out.config = {k: v for k, v in first[1].items() if "EC150" not in k}
    for v in out.config.values():  # (parse_base.py:376-380)
        if "pulse_duration" not in v and "pulse_length" in v:
            v["pulse_duration"] = [float(x) for x in v["pulse_length"].split(";")]
    out.config_xml, out.config_time = first[2], rtime[0]
    xsub = subtype[uid]
    env = [i for i in np.flatnonzero(xsub == "environment").tolist() if set(parsed[uid[i]][1]) != DROP_KEEL_ONLY]
    out.environment, out.environment_time, out.environment_xml = {}, None, None
    if env:  # (a handful per file)
        out.environment = dict(parsed[uid[env[-1]]][1])
        out.environment_xml, out.environment_time = parsed[uid[env[-1]]][2], rtime[is_xml[env[-1]]]
    # the parameter datagrams that count: those of channels that are not EC150 (parse_base.py:528-534)
    is_param = np.array([p[0] == "parameter" and "EC150" not in p[1].get("channel_id", "") for p in parsed], dtype=bool)
    par_sel = np.flatnonzero(is_param[uid])
    par_rec, par_uid = is_xml[par_sel], uid[par_sel]  # index into ``live`` / into ``parsed``

    # ---- RAW3 ----
    raw_idx = np.flatnonzero(live["type"] == b"RAW3")
    raw = live[raw_idx]
    hdr = _headers(buf, raw, RAW3_DTYPE, "RAW3")
    id_of, ids = _clean_ids(hdr["channel_id"])
    keep = np.array(["EC150" not in s for s in ids], dtype=bool)[id_of] if raw.size else np.zeros(0, bool)
    raw_idx, raw, hdr, id_of = raw_idx[keep], raw[keep], hdr[keep], id_of[keep]
    if raw.size == 0:
        raise ValueError("the file holds no RAW3 datagram")
    dt, count = hdr["data_type"].astype(np.int64) & 0xFFFF, hdr["count"].astype(np.int64)
    n_cplx = dt >> 8
    if np.any(count < 0):
        i = int(np.flatnonzero(count < 0)[0])
        raise ValueError(f"RAW3 datagram at byte offset {int(raw['offset'][i])} has count={int(count[i])}")
    half = (count > 0) & (n_cplx > 0) & ((dt & 8) == 0)
    if np.any(half):
        i = int(np.flatnonzero(half)[0])
        raise NotImplementedError(f"RAW3 datagram at byte offset {int(raw['offset'][i])} holds float16 complex samples "
                                  f"(data_type {int(dt[i]):#06x}), which are not built")
    has_p, has_a = ((dt & 1) != 0) & (count > 0), ((dt & 2) != 0) & (count > 0)
    n_cplx = np.where(count > 0, n_cplx, 0)
    body = raw["offset"].astype(np.int64) + RAW3_HEADER
    off_p = np.where(has_p, body, -1)
    off_a = np.where(has_a, body + 2 * count * has_p, -1)
    off_c = np.where(n_cplx > 0, body + 2 * count * (has_p.astype(np.int64) + has_a), -1)
    need = RAW3_HEADER + 2 * count * (has_p.astype(np.int64) + has_a) + 8 * count * n_cplx
    if np.any(need > raw["size"]):
        i = int(np.flatnonzero(need > raw["size"])[0])
        raise ValueError(f"RAW3 datagram at byte offset {int(raw['offset'][i])}: {int(raw['size'][i])} bytes do not hold "
                         f"count={int(count[i])} samples of data_type {int(dt[i]):#06x} ({int(need[i])} bytes)")
    if np.any(n_cplx > MAX_BEAMS):
        i = int(np.flatnonzero(n_cplx > MAX_BEAMS)[0])
        raise ValueError(f"RAW3 datagram at byte offset {int(raw['offset'][i])} has {int(n_cplx[i])} sectors, at most "
                         f"{MAX_BEAMS} are served")
    # each ping's parameter datagram: the last one in front of it
    k = np.searchsorted(par_rec, raw_idx) - 1
    if np.any(k < 0):
        i = int(np.flatnonzero(k < 0)[0])
        raise ValueError(f"RAW3 datagram at byte offset {int(raw['offset'][i])} has no parameter datagram in front")
    p_uid, p_inv = np.unique(par_uid[k], return_inverse=True)
    out.params = [parsed[u][1] for u in p_uid.tolist()]  # (distinct texts)
    out.ping_param = np.asarray(p_inv).reshape(-1)
    param_id = np.array([ids.index(p["channel_id"]) if p.get("channel_id") in ids else -1 for p in out.params], dtype=np.int64)
    if np.any(param_id[out.ping_param] != id_of):
        raise ValueError("Parameter ID does not match RAW")
    out.headers, out.channel_ids, out.ping_id = hdr, ids, id_of
    out.ping_channel = np.array(ids, dtype=object)[id_of]
    out.ping_time_all = nt_to_ns(hdr["low_date"], hdr["high_date"])
    out.count, out.n_complex, out.has_power, out.has_angle = count, n_cplx, has_p, has_a
    out.off_power, out.off_angle, out.off_complex = off_p, off_a, off_c
    out.raw_offset = raw["offset"].astype(np.int64)

    # ---- the beam groups (set_groups_ek80.py:1124-1232) ----
    n_ids = len(ids)
    complex_ch = np.bincount(id_of[n_cplx > 0], minlength=n_ids) > 0
    power_ch = np.bincount(id_of[has_p], minlength=n_ids) > 0
    form = param_field(out, "pulse_form", np.float64)
    members = {"complex_FM": complex_ch[id_of] & (form == 1), "complex_CW": complex_ch[id_of] & (form == 0),
               "power": power_ch[id_of]}
    out.groups = []
    for descr in GROUP_ORDER:
        sel = np.flatnonzero(members[descr])
        if sel.size == 0:
            continue
        g = Ek80Group()
        g.descr, g.ping = descr, sel
        used = np.unique(id_of[sel])
        order = sorted((ids[i], i) for i in used.tolist())
        g.channel = [cid for cid, _ in order]
        c_of = np.full(n_ids, -1, dtype=np.int64)
        c_of[[i for _, i in order]] = np.arange(len(order))
        c, t = c_of[id_of[sel]], out.ping_time_all[sel]
        g.ping_time = np.unique(t)
        g.C, g.P, g.S = len(order), int(g.ping_time.size), int(max(1, count[sel].max()))
        g.row = c * g.P + np.searchsorted(g.ping_time, t)
        if np.unique(g.row).size != g.row.size:
            raise ValueError("a channel holds two pings with one time stamp")
        g.rows_present = int(g.row.size)
        table = np.empty((g.C * g.P, 3), dtype=np.int64)
        if descr == "power":
            g.B = None
            chan_angles = np.bincount(c[~has_a[sel]], minlength=g.C) == 0
            use_a = has_a[sel] & chan_angles[c]
            table[:, :2], table[:, 2] = -1, 0
            table[g.row, 0] = off_p[sel]
            table[g.row, 1] = np.where(use_a, off_a[sel], -1)
            table[g.row, 2] = np.where(has_p[sel] | use_a, count[sel], 0)
            if not chan_angles.any():
                g.angles = None
            elif g.row.size == g.C * g.P and bool(np.all(use_a & (count[sel] == g.S))):
                g.angles = "int8"
            else:
                g.angles = "float32"
        else:
            g.B, g.angles = int(max(1, n_cplx[sel].max())), None
            table[:, 0], table[:, 1:] = -1, 0
            table[g.row, 0] = off_c[sel]
            table[g.row, 1] = np.where(off_c[sel] >= 0, count[sel], 0)
            table[g.row, 2] = n_cplx[sel]
        g.table = table
        out.groups.append(g)
    if not out.groups:
        raise ValueError("the file holds no RAW3 datagram with samples of a pulse form that is served (CW or LFM)")

    # ---- RAW4, FIL1, MRU0 / MRU1, NME0 ----
    out.raw4_count = int((live["type"] == b"RAW4").sum())
    out.mru1_count = int((live["type"] == b"MRU1").sum())
    fil_rec = live[live["type"] == b"FIL1"]
    fh = _headers(buf, fil_rec, FIL1_DTYPE, "FIL1")
    fid_of, fids = _clean_ids(fh["channel_id"]) if fil_rec.size else (np.zeros(0, np.int64), [])
    ftime = nt_to_ns(fh["low_date"], fh["high_date"])
    out.fil, kept_times = {}, []
    for i in range(fil_rec.size):  # (filters, a few per channel, not pings)
        cid, n = fids[fid_of[i]], int(fh["n_coefficients"][i])
        if "EC150" in cid:
            continue
        a = int(fil_rec["offset"][i]) + FIL1_HEADER
        if n < 0 or FIL1_HEADER + 8 * n > int(fil_rec["size"][i]):
            raise ValueError(f"FIL1 datagram at byte offset {int(fil_rec['offset'][i])}: {int(fil_rec['size'][i])} bytes do not "
                             f"hold its {n} coefficients")
        coeffs = buf[a:a + 8 * n].copy().view("<c8")
        out.fil.setdefault((cid, int(fh["stage"][i])), []).append((ftime[i], coeffs, int(fh["decimation_factor"][i])))
        kept_times.append(ftime[i])
    out.filter_time = np.unique(np.array(kept_times, dtype="datetime64[ns]"))
    mru_rec = live[live["type"] == b"MRU0"]
    out.mru0 = _headers(buf, mru_rec, MRU0_DTYPE, "MRU0")
    out.mru0_time = nt_to_ns(out.mru0["low_date"], out.mru0["high_date"])
    out.nmea_time, out.nmea, out.nmea_offset, out.nmea_length = nmea_sentences(buf, live[live["type"] == b"NME0"])
    out.nmea_selected = np.flatnonzero(parse_nmea.select(buf, out.nmea_offset, out.nmea_length))
    out.ping_time = np.unique(out.ping_time_all)  # (every ping of the file: the placeholder of a file without a fix)
    return out


def param_field(pl, key, dtype=np.float64, missing=np.nan):
    """A field of the parameter datagrams per ping (file order): looked up once per distinct text, then indexed."""
    per_text = np.array([dtype(p[key]) if key in p else missing for p in pl.params], dtype=dtype)
    return per_text[pl.ping_param]


def per_ping(pl, g, values, dtype=np.float64):
    """Per-ping ``values`` (aligned with the plan's pings) on the (channel, ping_time) grid of group ``g``: NaN where a
    channel lacks a ping; an integer ``dtype`` is kept when no row is missing, else the variable becomes float32 with NaN
    (as ``parse_ek60.per_ping``)."""
    v = np.asarray(values)[g.ping]
    dt = np.dtype(dtype)
    full = g.rows_present == g.C * g.P
    if dt.kind == "U":
        a = np.full(g.C * g.P, "", dtype=v.dtype if v.dtype.kind == "U" else dt)
    elif dt.kind == "i" and full:
        a = np.empty(g.C * g.P, dtype=dt)
    else:
        a = np.full(g.C * g.P, np.nan, dtype=np.float32 if dt.kind == "i" else dt)
    a[g.row] = v
    return a.reshape(g.C, g.P)
