"""Positions from NMEA sentences: the rules ``open_raw`` applies to the ``NME0`` datagrams of an EK60 file, in plain Python.

The reference parses every selected sentence with ``pynmea2.parse`` and reads ``.latitude`` / ``.longitude`` /
``.sentence_type`` of the result (echopype convert/set_groups_base.py:180-239).  That library is not a dependency here and
has NEVER been run against this module: what follows restates its documented behaviour, and the restatement is the
yardstick the kernel (csrc/nmea.hip, ``ops.nmea_positions``) is held to, bit for bit.  ``parse_sentence`` is also the
host fallback for the sentences the kernel does not decide.

A sentence ``s`` is what ``parse_ek60.nmea_sentences`` gives: the datagram's text, NULs stripped at both ends, decoded as
ASCII with replacement (one character per byte, so character and byte positions agree).

R1  selection   ``s[3:6]`` is exactly ``"GGA"``, ``"GLL"`` or ``"RMC"`` (set_groups_base.py:182-183): case-sensitive, and
                whatever stands in ``s[0:3]`` does not matter.  (``select``)
R2  form        ``s`` matches ``SENTENCE_RE`` (case-insensitive), through its talker branch ``\\w{2}\\w{3},`` and the three
                letters behind the talker, upper-cased, are GGA, GLL or RMC; else the sentence is invalid.
R3  checksum    present: the XOR of the characters of ``nmea_str`` equals ``int(checksum, 16)``, else invalid; absent:
                accepted.
R4  fields      ``data.split(",")``, a missing field is ``""``; (lat, lat_dir, lon, lon_dir) are the fields
                GGA 1 2 3 4, GLL 0 1 2 3, RMC 2 3 4 5.
R5  value       ``""`` or ``"0"`` is 0.0; otherwise the field matches ``^(\\d+)(\\d\\d\\.\\d+)$`` and the value is
                ``float(d) + float(m) / 60``; a field that does not match gives NaN for that coordinate (the caller logs
                the reference's warning once per file).  Sign: ``+`` for N / E, ``-`` for S / W, any other direction
                gives 0.0; ``"0"`` with ``S`` is -0.0.  The value is looked at before the direction.
R6  type        the three letters of a sentence that passed R2 and R3, also when R5 gave NaN; ``""`` with NaN, NaN for an
                invalid one.

Corners where this restatement may differ from the library (none has been compared with it):

* a talker that begins with ``P`` takes the pattern's proprietary branch, a sentence such as ``ccGPQ,GGA`` its query
  branch; what the library makes of them is not known here: both are invalid;
* a sentence that passes R2's pattern with another three letters behind its talker (possible when ``s`` starts with white
  space, which moves ``s[3:6]``) is invalid: the library has no class with positions for it, or raises;
* without a checksum the pattern's ``data`` runs to the end of the string, trailing CR / LF included, so a direction that
  is the last field is then not ``"N"`` but ``"N\\r\\n"`` and gives 0.0;
* ``sentence_type`` of an invalid sentence is ``""``, where the reference holds a float NaN: the variable keeps one
  string dtype, which ``combine_echodata`` concatenates.

``plain_form`` is the kernel's own test, restated: the sentences it decides by itself.  It is a pure function of the bytes."""
import math
import re
from functools import reduce

import numpy as np

SENTENCE_RE = re.compile(r"^\s*\$?(?P<nmea_str>(?P<sentence_type>(P\w{3})|(\w{2}\w{2}Q,\w{3})|(\w{2}\w{3},))(?P<data>[^*]*))"
                         r"(?:[*](?P<checksum>[A-F0-9]{2}))?\s*[\r\n]*$", re.IGNORECASE)
VALUE_RE = re.compile(r"^(\d+)(\d\d\.\d+)$")
TYPES = ("GGA", "GLL", "RMC")  # the order is the kernel's type code
FIELDS = {"GGA": (1, 2, 3, 4), "GLL": (0, 1, 2, 3), "RMC": (2, 3, 4, 5)}  # lat, lat_dir, lon, lon_dir

# the status byte of ``ops.nmea_positions`` (include/echopype_amd.h: EPA_NMEA_*)
INVALID, LAT_FAILED, LON_FAILED, TYPE_SHIFT, TYPE_MASK, UNDECIDED = 1, 2, 4, 3, 0x18, 64
MAX_DIGITS = 15  # of ``d`` and of ``m`` without its point, leading zeros not counted; also of the decimals of ``m``
MAX_FIELD = 64   # bytes of a coordinate field the kernel looks at

WARNING = {"latitude": "At least one latitude entry is problematic and are assigned None in the converted data: %s",
           "longitude": "At least one longitude entry is problematic and are assigned None in the converted data: %s"}
_TRAIL = b"\r\n \t"


class Parsed:
    """What R2 - R4 make of a sentence: ``type`` ("" when invalid) and the four field strings."""

    def __init__(self, type="", lat="", lat_dir="", lon="", lon_dir=""):
        self.type, self.lat, self.lat_dir, self.lon, self.lon_dir = type, lat, lat_dir, lon, lon_dir


def split_sentence(s):
    """R2 - R4 -> :class:`Parsed`."""
    m = SENTENCE_RE.match(s)
    if m is None or m.group(5) is None:  # no match, or the proprietary / query branch
        return Parsed()
    kind = m.group("sentence_type")[2:5].upper()
    if kind not in FIELDS:
        return Parsed()
    if m.group("checksum") is not None and reduce(lambda a, c: a ^ ord(c), m.group("nmea_str"), 0) != int(m.group("checksum"), 16):
        return Parsed()
    f = m.group("data").split(",")
    return Parsed(kind, *(f[i] if i < len(f) else "" for i in FIELDS[kind]))


def value(field):
    """R5 without the sign: degrees from ``DDDMM.MMM``; ``ValueError`` for a field of another form."""
    if not field or field == "0":
        return 0.0
    m = VALUE_RE.match(field)
    if m is None:
        raise ValueError(f"Geographic coordinate value '{field}' is not valid DDDMM.MMM")
    return float(m.group(1)) + float(m.group(2)) / 60


def _signed(field, direction, plus, minus):
    try:
        sd = value(field)
    except ValueError:
        return math.nan
    return sd if direction == plus else -sd if direction == minus else 0.0


def parse_sentence(s):
    """R2 - R6 for one sentence -> (latitude, longitude, sentence type)."""
    p = split_sentence(s)
    if not p.type:
        return math.nan, math.nan, ""
    return _signed(p.lat, p.lat_dir, "N", "S"), _signed(p.lon, p.lon_dir, "E", "W"), p.type


def select(buf, offset, length):
    """R1 on the file's bytes: ``buf`` uint8, ``offset`` / ``length`` of every stripped text -> bool per sentence."""
    offset, length = np.asarray(offset, dtype=np.int64), np.asarray(length, dtype=np.int64)
    keep = np.zeros(offset.size, dtype=bool)
    long_enough = np.flatnonzero(length >= 6)
    if long_enough.size:
        three = buf[offset[long_enough, None] + np.arange(3, 6)]
        hit = np.zeros(long_enough.size, dtype=bool)
        for t in TYPES:
            hit |= (three == np.frombuffer(t.encode(), np.uint8)).all(axis=1)
        keep[long_enough] = hit
    return keep


def _digits_bounded(field):
    """The bound under which the kernel's arithmetic is ``float()`` bit for bit; fields R5 refuses are decided (NaN)."""
    if len(field) > MAX_FIELD:
        return False
    m = VALUE_RE.match(field)
    if m is None:
        return True
    d, mm = m.group(1), m.group(2).replace(".", "")
    return int(d) < 10 ** MAX_DIGITS and int(mm) < 10 ** MAX_DIGITS and len(mm) - 2 <= MAX_DIGITS


def plain_form(raw):
    """The kernel's test on the bytes of a stripped text: True when it decides the sentence itself (status below 64).

    Byte 0 is ``$``; bytes 1-5 are ASCII letters or digits, byte 1 not ``P`` / ``p``, bytes 3-5 ``GGA``, ``GLL`` or ``RMC``;
    byte 6 is ``,``; every byte is in 0x20..0x7E apart from a trailing run of CR / LF / space / tab; at most one ``*``, and
    then exactly two hex digits and only that run behind them; without a ``*`` the four coordinate fields end at a comma or
    the run is empty (else the run belongs to a field); a latitude / longitude field has at most ``MAX_FIELD`` bytes and, where it
    has R5's form, at most ``MAX_DIGITS`` significant digits in ``d`` and in ``m``, and as many decimals."""
    raw = bytes(raw)
    if len(raw) < 7 or raw[0:1] != b"$" or raw[6:7] != b",":
        return False
    head = raw[1:6]
    if not (head.isalnum() and head.isascii()) or head[0:1] in b"Pp" or head[2:5].decode() not in FIELDS:
        return False
    body = raw.rstrip(_TRAIL)
    if any(b < 0x20 or b > 0x7E for b in body) or body.count(b"*") > 1:
        return False
    star = body.find(b"*")
    if star >= 0:
        if len(body) != star + 3 or not all(chr(b) in "0123456789abcdefABCDEF" for b in body[star + 1:]):
            return False
        data = raw[7:star]
    else:
        data = raw[7:]
    f = data.split(b",")
    idx = FIELDS[head[2:5].decode()]
    if star < 0 and len(body) != len(raw) and len(f) <= idx[3] + 1:
        return False
    lat, lon = (f[i].decode() if i < len(f) else "" for i in (idx[0], idx[2]))
    return _digits_bounded(lat) and _digits_bounded(lon)


def placeholder(ping_time):
    """The Platform entry of a file without a selected sentence (the reference's ``_nan_timestamp_handler``): one fix at
    the earliest ping time, NaN, NaN, ""."""
    t = np.asarray(ping_time, dtype="datetime64[ns]")
    return t.min().reshape(1), np.array([np.nan]), np.array([np.nan]), np.array([""], dtype="<U3")


def positions_host(sentences):
    """``parse_sentence`` over a list of sentences -> (lat float64, lon float64, type str array)."""
    out = [parse_sentence(s) for s in sentences]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype="<U3"))
