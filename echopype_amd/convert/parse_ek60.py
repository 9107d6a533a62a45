"""Everything of ``open_raw`` (EK60) that needs no device: the framing walk (``epa_raw_index``), the ``CON0``
configuration, the ``RAW0`` headers of all pings in one gather, ``ping_time``, the channel order and the row table the
unpack kernel reads (echopype convert/utils/ek_raw_io.py, ek_raw_parsers.py, parse_base.py, set_groups_ek60.py).

Nothing here loops over pings in Python: the records come from the C walk as one structured array, the 84-byte ``RAW0``
headers are gathered with one fancy index and viewed through a structured dtype."""
import ctypes
import struct

import numpy as np

from .. import _lib
from . import parse_nmea

RECORD_DTYPE = np.dtype([("offset", "<i8"), ("size", "<i4"), ("type", "S4"), ("low_date", "<u4"), ("high_date", "<u4"),
                         ("flags", "<u4"), ("reserved", "<u4")])
assert RECORD_DTYPE.itemsize == _lib.RAW_RECORD_BYTES

# SimradRawParser version 0 (ek_raw_parsers.py:1629-1652), "=" packing: 84 bytes
RAW0_FLOATS = ("transducer_depth", "frequency", "transmit_power", "pulse_length", "bandwidth", "sample_interval",
               "sound_velocity", "absorption_coefficient", "heave", "roll", "pitch", "temperature", "heading")
RAW0_DTYPE = np.dtype([("type", "S4"), ("low_date", "<u4"), ("high_date", "<u4"), ("channel", "<i2"), ("mode", "<i2")] +
                      [(k, "<f4") for k in RAW0_FLOATS] +
                      [("transmit_mode", "<i2"), ("spare0", "S6"), ("offset", "<i4"), ("count", "<i4")])
RAW0_HEADER = 84
assert RAW0_DTYPE.itemsize == RAW0_HEADER

# SimradConfigParser version 0 (ek_raw_parsers.py:1311-1351): 528 bytes, then 320 per transceiver
CON0_HEADER_FMT = "<4sLL128s128s128s30s98sl"
CON0_HEADER_FIELDS = ("type", "low_date", "high_date", "survey_name", "transect_name", "sounder_name", "version", "spare0",
                      "transceiver_count")
CON0_TXCVR_FMT = "<128sl15f5f8s5f8s5f8s16s28s"
CON0_TXCVR_SCALARS = ("channel_id", "beam_type", "frequency", "gain", "equivalent_beam_angle", "beamwidth_alongship",
                      "beamwidth_athwartship", "angle_sensitivity_alongship", "angle_sensitivity_athwartship",
                      "angle_offset_alongship", "angle_offset_athwartship", "pos_x", "pos_y", "pos_z", "dir_x", "dir_y", "dir_z")
CON0_HEADER_SIZE = struct.calcsize(CON0_HEADER_FMT)
CON0_TXCVR_SIZE = struct.calcsize(CON0_TXCVR_FMT)
assert CON0_HEADER_SIZE == 528 and CON0_TXCVR_SIZE == 320

NT_EPOCH_US = -11644473600 * 1000000  # 1601-01-01 in microseconds since 1970-01-01


def raw_index(buf, n_bytes=None):
    """``buf``: the file's bytes (C-contiguous uint8 array; ``n_bytes`` of it, default all) -> (records, n_consumed).
    ``records`` is a structured array (``RECORD_DTYPE``), one entry per complete datagram; ``n_consumed < n_bytes`` says
    the file was cut there.  ``ValueError`` (with the byte offset) for a size below 16 and for a trailing size that
    differs from the leading one: unlike the reference this reader does not search for the next datagram."""
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    n = int(buf.size if n_bytes is None else n_bytes)
    if n > buf.size:
        raise ValueError(f"raw_index: n_bytes={n} is more than the {buf.size} bytes given")
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    count, used = ctypes.c_longlong(), ctypes.c_longlong()
    _lib.call("epa_raw_index", ptr, n, None, 0, ctypes.byref(count), ctypes.byref(used))
    rec = np.zeros(count.value, dtype=RECORD_DTYPE)
    _lib.call("epa_raw_index", ptr, n, rec.ctypes.data_as(ctypes.c_void_p), rec.size, ctypes.byref(count), ctypes.byref(used))
    return rec, int(used.value)


def _text(b):
    return b.decode("latin_1").strip("\x00")


def parse_con0(buf, rec):
    """The ``CON0`` datagram at record ``rec`` -> the dict ``SimradConfigParser`` gives (version 0, the ER60 / ES60 / ES70
    transceiver layout, which the reference also falls back to for an unknown sounder name), the three 5-entry tables
    rounded to 6 digits as there.  ``transceivers`` is keyed 1 .. transceiver_count."""
    off, size = int(rec["offset"]), int(rec["size"])
    if size < CON0_HEADER_SIZE:
        raise ValueError(f"CON0 datagram of {size} bytes is shorter than its {CON0_HEADER_SIZE}-byte header")
    body = buf[off:off + size].tobytes()
    data = dict(zip(CON0_HEADER_FIELDS, struct.unpack_from(CON0_HEADER_FMT, body, 0)))
    for k in ("type", "survey_name", "transect_name", "sounder_name", "version", "spare0"):
        data[k] = _text(data[k]) if k != "type" else data[k].decode("latin_1")
    if data["sounder_name"] == "MBES":
        raise NotImplementedError("ME70 (MBES) configuration datagrams are not served")
    n = int(data["transceiver_count"])
    if n < 0 or CON0_HEADER_SIZE + n * CON0_TXCVR_SIZE > size:
        raise ValueError(f"CON0 datagram of {size} bytes cannot hold its {n} transceivers")
    data["transceivers"] = {}
    for i in range(n):  # (channels, not pings)
        v = struct.unpack_from(CON0_TXCVR_FMT, body, CON0_HEADER_SIZE + i * CON0_TXCVR_SIZE)
        t = dict(zip(CON0_TXCVR_SCALARS, v[:17]))
        t["pulse_length_table"] = np.array([round(x, 6) for x in v[17:22]], dtype=float)
        t["spare1"] = _text(v[22])
        t["gain_table"] = np.array([round(x, 6) for x in v[23:28]], dtype=float)
        t["spare2"] = _text(v[28])
        t["sa_correction_table"] = np.array([round(x, 6) for x in v[29:34]], dtype=float)
        t["spare3"] = _text(v[34])
        t["gpt_software_version"] = _text(v[35])
        t["spare4"] = _text(v[36])
        t["channel_id"] = _text(t["channel_id"])
        data["transceivers"][i + 1] = t
    return data


def nt_to_ns(low_date, high_date):
    """NT time pairs -> datetime64[ns], bit for bit what ``np.datetime64(nt_to_unix((low, high)), "ns")`` gives
    (ek_date_conversion.py:48-52): ``((high << 32) + low) * 1e-7`` seconds in float64, added to 1601-01-01 as a
    ``datetime.timedelta`` -- which splits the float into whole seconds and a fraction and rounds the fraction to whole
    microseconds, ties to even."""
    ticks = (np.asarray(high_date, dtype=np.uint64) << np.uint64(32)) + np.asarray(low_date, dtype=np.uint64)
    sec = ticks.astype(np.float64) * 1.0e-7
    frac, whole = np.modf(sec)
    us = whole.astype(np.int64) * 1000000 + np.rint(frac * 1.0e6).astype(np.int64) + NT_EPOCH_US
    return (us * 1000).view("datetime64[ns]")


def gather_raw0(buf, records):
    """The 84-byte headers of the ``RAW0`` datagrams ``records`` (a structured array) as one structured array
    (``RAW0_DTYPE``): a single fancy index over the record offsets."""
    if np.any(records["size"] < RAW0_HEADER):
        bad = records[records["size"] < RAW0_HEADER][0]
        raise ValueError(f"RAW0 datagram at byte offset {int(bad['offset'])} has {int(bad['size'])} bytes, fewer than its "
                         f"{RAW0_HEADER}-byte header")
    if records.size == 0:
        return np.zeros(0, dtype=RAW0_DTYPE)
    # (every 84-byte window of the file as a view, indexed with the offsets: 84 contiguous bytes copied per datagram)
    windows = np.lib.stride_tricks.sliding_window_view(buf, RAW0_HEADER)
    return np.ascontiguousarray(windows[records["offset"]]).view(RAW0_DTYPE).reshape(-1)


def nmea_sentences(buf, records):
    """(times datetime64[ns], sentences, offsets, lengths) of the ``NME0`` datagrams: the text behind the 12-byte header,
    NULs stripped, decoded as ASCII with replacement (ek_raw_parsers.py:442-446), and where that stripped text lies in
    ``buf`` (int64 byte offset and length: leading NULs move the start).  (One Python step per sentence: they are
    strings.)"""
    times = nt_to_ns(records["low_date"], records["high_date"])
    start = records["offset"].astype(np.int64) + 12
    length = records["size"].astype(np.int64) - 12
    text = [str(buf[a:a + n].tobytes().strip(b"\x00"), "ascii", errors="replace") for a, n in zip(start.tolist(), length.tolist())]
    # where the stripped text lies: the whole body unless its first or last byte is a NUL (few sentences, if any)
    some = np.flatnonzero(length > 0)
    padded = some[(buf[start[some]] == 0) | (buf[start[some] + length[some] - 1] == 0)]
    for i in padded.tolist():
        raw = buf[start[i]:start[i] + length[i]].tobytes()
        tail = raw.lstrip(b"\x00")
        start[i] += len(raw) - len(tail)
        length[i] = len(tail.rstrip(b"\x00"))
    return times, text, start, length


class Ek60Plan:
    """What ``plan`` found: the attributes are documented there."""


def plan(buf, n_bytes=None):
    """The host half of ``open_raw``: ``buf`` (uint8 array, the file) -> an :class:`Ek60Plan` with

    ``n_consumed``      bytes of complete datagrams (less than the file: it was cut there)
    ``config``          the ``CON0`` dict (``parse_con0``)
    ``records``         every datagram's record; ``skipped_zero_time``: how many carried the time stamp (0, 0)
    ``headers``         the ``RAW0`` headers that count (``gather_raw0``), file order, and ``header_time`` / ``header_row``
                        (their ping time and their row ``c * P + p`` in the volumes)
    ``transceivers``    the transceiver numbers (1-based, the ``channel`` field of RAW0) of the output channels, ordered
                        by channel id string, channels without power dropped (set_groups_ek60.py:73-80)
    ``channel``         their id strings
    ``ping_time``       the sorted union of the channels' ping times (the reference's outer join); ``C, P, S``
    ``table``           int64 (C * P, 3): byte offset of the power block, of the angle block (-1: none), count
    ``angles``          None, "int8" or "float32": the angle variables exist when a channel records angles on all its
                        pings (set_groups_ek60.py:678); int8 when every row of every channel is present, full and has
                        angles, else float32 with NaN (the rule of ``ops.concat_rows``)
    ``nmea_time, nmea``  the NME0 sentences; ``nmea_offset, nmea_length``: where each one's stripped text lies in the file;
                        ``nmea_selected``: the indices of those that carry a position (``parse_nmea.select``, rule R1)

    ``ValueError``: no ``CON0`` in front, no ping with power, a RAW0 that does not hold its samples, a channel number
    outside the configuration, a ping time twice in one channel; ``NotImplementedError``: a mode-2 (angle only) ping."""
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    out = Ek60Plan()
    rec, out.n_consumed = raw_index(buf, n_bytes)
    out.records = rec
    if rec.size == 0 or rec["type"][0] != b"CON0":
        got = rec["type"][0].decode("latin_1") if rec.size else "nothing"
        raise ValueError(f"an EK60 .raw file starts with a CON0 datagram, this one with {got}")
    out.config = cfg = parse_con0(buf, rec[0])
    zero = (rec["flags"] & _lib.RAW_ZERO_TIME) != 0
    out.skipped_zero_time = int(zero[1:].sum())
    live = rec[1:][~zero[1:]]
    out.nmea_time, out.nmea, out.nmea_offset, out.nmea_length = nmea_sentences(buf, live[live["type"] == b"NME0"])
    out.nmea_selected = np.flatnonzero(parse_nmea.select(buf, out.nmea_offset, out.nmea_length))
    raw = live[live["type"] == b"RAW0"]
    hdr = gather_raw0(buf, raw)
    mode, count, chan = hdr["mode"].astype(np.int64), hdr["count"].astype(np.int64), hdr["channel"].astype(np.int64)
    if np.any((mode & 3) == 2):
        raise NotImplementedError("RAW0 datagrams of mode 2 (angle only) are not served")
    has_p, has_a = (mode & 1) != 0, (mode & 2) != 0
    need = RAW0_HEADER + 2 * np.maximum(count, 0) * (has_p.astype(np.int64) + has_a.astype(np.int64))
    if np.any(count < 0) or np.any(need > raw["size"]):
        i = int(np.flatnonzero((count < 0) | (need > raw["size"]))[0])
        raise ValueError(f"RAW0 datagram at byte offset {int(raw['offset'][i])}: {int(raw['size'][i])} bytes do not hold "
                         f"count={int(count[i])} samples of mode {int(mode[i])}")
    n_tx = len(cfg["transceivers"])
    if np.any((chan < 1) | (chan > n_tx)):
        raise ValueError(f"a RAW0 datagram names channel {int(chan[(chan < 1) | (chan > n_tx)][0])}, the configuration has "
                         f"{n_tx} transceivers")
    # channels in the order of their id strings; one that never delivers a power sample is dropped
    with_power = np.bincount(chan[has_p & (count > 0)], minlength=n_tx + 1) > 0
    order = sorted((t["channel_id"], k) for k, t in cfg["transceivers"].items() if with_power[k])
    if not order:
        raise ValueError("the file holds no RAW0 datagram with power samples")
    out.transceivers = [k for _, k in order]
    out.channel = [cid for cid, _ in order]
    c_of = np.full(n_tx + 1, -1, dtype=np.int64)
    c_of[out.transceivers] = np.arange(len(order))
    keep = c_of[chan] >= 0
    hdr, raw, mode, count, chan, has_p, has_a = (a[keep] for a in (hdr, raw, mode, count, chan, has_p, has_a))
    t = nt_to_ns(hdr["low_date"], hdr["high_date"])
    c = c_of[chan]
    out.ping_time = np.unique(t)
    p = np.searchsorted(out.ping_time, t)
    out.C, out.P, out.S = C, P, S = len(order), int(out.ping_time.size), int(max(1, count.max()))
    row = c * P + p
    if np.unique(row).size != row.size:
        raise ValueError("a channel holds two pings with one time stamp")
    out.headers, out.header_time, out.header_row = hdr, t, row
    # a channel's angles count when ALL its pings record them (set_groups_ek60.py:678)
    chan_angles = np.bincount(c[~has_a], minlength=C) == 0
    use_a = has_a & chan_angles[c]
    table = np.empty((C * P, 3), dtype=np.int64)
    table[:, :2] = -1
    table[:, 2] = 0
    body = raw["offset"].astype(np.int64) + RAW0_HEADER
    table[row, 0] = np.where(has_p, body, -1)
    table[row, 1] = np.where(use_a, body + np.where(has_p, 2 * count, 0), -1)
    table[row, 2] = count
    out.table = table
    out.rows_present = int(row.size)
    if not chan_angles.any():
        out.angles = None
    elif row.size == C * P and bool(np.all(use_a & (count == S))):
        out.angles = "int8"
    else:
        out.angles = "float32"
    return out


def per_ping(pl, field, dtype=np.float64):
    """A RAW0 header field on (channel, ping_time): float64 with NaN where a channel lacks a ping; an integer ``dtype``
    is kept when no row is missing, else the variable becomes float32 with NaN (xarray's promotion of a small integer)."""
    v = pl.headers[field]
    full = pl.rows_present == pl.C * pl.P
    dt = np.dtype(dtype)
    if dt.kind == "i" and full:
        a = np.empty(pl.C * pl.P, dtype=dt)
    else:
        a = np.full(pl.C * pl.P, np.nan, dtype=np.float32 if dt.kind == "i" else dt)
    a[pl.header_row] = v
    return a.reshape(pl.C, pl.P)
