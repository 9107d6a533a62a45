"""The NMEA sentences of the position tests (TEST INFRASTRUCTURE, data only): sentences with answers worked out by hand,
sentences the kernel must not decide, the shapes of the kernel test, and a few lines of ``struct`` that lay NME0 datagrams
between the pings of the ``aligned`` open_raw fixture.

``HAND``: (name, sentence bytes, latitude, longitude, sentence type, does the kernel decide it?).  The answers are written
as the arithmetic of rule R5 -- ``float(d) + float(m) / 60`` with the literals of the sentence -- or as NaN / 0.0 where a
rule says so; nothing here calls the code under test."""
import struct
from functools import reduce
from operator import xor

import numpy as np

import raw_cases as R

NAN = float("nan")


def ck(body):
    """``$`` + body + ``*`` + the XOR of the body's bytes as two upper-case hex digits."""
    x = reduce(xor, body.encode("latin_1"), 0)
    return f"${body}*{x:02X}".encode("latin_1")


def ckb(body):
    """``ck`` for a body given as bytes: the checksum is the XOR of the RAW bytes."""
    return b"$" + body + b"*%02X" % reduce(xor, body, 0)


def _pad(body, length):
    """``body`` (GGA: free fields at its end) made so long that the sentence with its checksum has ``length`` bytes."""
    need = length - (len(body) + 4)
    assert need >= 0
    return ck(body + "7" * need)


def _wrong(sentence):
    """The sentence with another last hex digit."""
    return sentence[:-1] + (b"0" if sentence[-1:] != b"0" else b"1")


GGA = "GPGGA,234910.00,4704.1234,N,12503.4321,W,1,08,0.9,12.3,M,-20.1,M,,"
GLL = "GPGLL,4704.12,N,12503.43,W,234911,A"
GGA_SHORT = "GPGGA,1,4704.1234,N,12503.4321,W,1,"
RMC = "GPRMC,234912,A,4704.1234,N,12503.4321,W,9.7,254.1,120917,,"
LAT_4, LON_4 = 47 + 4.1234 / 60, -(125 + 3.4321 / 60)  # 4704.1234,N: d = "47", m = "04.1234"; 12503.4321,W
LAT_2, LON_2 = 47 + 4.12 / 60, -(125 + 3.43 / 60)      # 4704.12,N; 12503.43,W
# (a GLL whose checksum has a letter among its hex digits: the last field is free)
_LOWER = next(s for s in (ck(GLL[:-1] + c) for c in "AVBCDEFGH") if s[-2:] != s[-2:].lower())

HAND = [
    # the three types
    ("gga", ck(GGA), LAT_4, LON_4, "GGA", True),
    ("gll", ck(GLL), LAT_2, LON_2, "GLL", True),
    ("rmc", ck(RMC), LAT_4, LON_4, "RMC", True),
    # southern and eastern fixes: 3351.0000,S -> -(33 + 51.0/60); 15112.5000,E -> 151 + 12.5/60
    ("south_east", ck("GPGGA,000000,3351.0000,S,15112.5000,E,1,,,,,,,,"), -(33 + 51.0 / 60), 151 + 12.5 / 60, "GGA", True),
    ("rmc_south_east", ck("GNRMC,1,A,0030.5,S,00015.25,E"), -(0 + 30.5 / 60), 0 + 15.25 / 60, "RMC", True),
    # empty fields: "" is 0.0, and a direction that is neither letter gives 0.0
    ("empty_fields", ck("GPGGA,,,,,,0,,,,,,,,"), 0.0, 0.0, "GGA", True),
    ("no_direction", ck("GPGLL,4704.12,,12503.43,,1,A"), 0.0, 0.0, "GLL", True),
    ("wrong_direction", ck("GPGLL,4704.12,E,12503.43,N,1,A"), 0.0, 0.0, "GLL", True),
    ("long_direction", ck("GPGLL,4704.12,N ,12503.43,WW,1,A"), 0.0, 0.0, "GLL", True),
    # trailing fields cut off: a missing field is ""
    ("cut_after_lat_dir", ck("GPGLL,4704.12,N"), LAT_2, 0.0, "GLL", True),
    ("cut_after_lon", ck("GPGLL,4704.12,S,12503.43"), -LAT_2, 0.0, "GLL", True),
    ("cut_rmc", ck("GPRMC,1,A"), 0.0, 0.0, "RMC", True),
    ("only_the_head", b"$GPGGA,", 0.0, 0.0, "GGA", True),
    # "0": 0.0, and -0.0 with S / W
    ("zero_south_west", ck("GPGLL,0,S,0,W"), -0.0, -0.0, "GLL", True),
    ("zero_north_east", ck("GPGLL,0,N,0,E"), 0.0, 0.0, "GLL", True),
    # R5 fails: NaN for that coordinate, the type stays
    ("lat_fails", ck("GPGLL,04.12,N,12503.43,W"), NAN, -(125 + 3.43 / 60), "GLL", True),
    ("lon_fails", ck("GPGGA,1,4704.12,N,125o3.43,W"), LAT_2, NAN, "GGA", True),
    ("both_fail", ck("GPRMC,1,A,00,N,4704.,W"), NAN, NAN, "RMC", True),
    ("no_decimals", ck("GPGLL,4704,N,12503,W"), NAN, NAN, "GLL", True),
    ("two_points", ck("GPGLL,47.04.12,N,1.2503.43,W"), NAN, NAN, "GLL", True),
    # checksums
    ("no_checksum", b"$" + GLL.encode(), LAT_2, LON_2, "GLL", True),
    ("wrong_checksum", _wrong(ck(GLL)), NAN, NAN, "", True),
    ("lower_case_hex", _LOWER[:-2] + _LOWER[-2:].lower(), LAT_2, LON_2, "GLL", True),
    ("one_hex_digit", R.NMEA[1].encode(), NAN, NAN, "", False),  # (the `aligned` / `ragged` fixtures hold it)
    ("one_hex_digit_gga", R.NMEA[0].encode(), NAN, NAN, "", False),
    ("three_hex_digits", ck(GLL) + b"0", NAN, NAN, "", False),
    ("no_hex_digit", b"$" + GLL.encode() + b"*", NAN, NAN, "", False),
    ("not_hex", b"$" + GLL.encode() + b"*4G", NAN, NAN, "", False),
    ("two_stars", b"$GPGLL,4704.12,N,1*503.43,W*4A", NAN, NAN, "", False),
    # the end of the text
    ("cr_lf", ck(GLL) + b"\r\n", LAT_2, LON_2, "GLL", True),
    ("spaces_tabs_cr_lf", ck(GGA) + b" \t \r\n\n", LAT_4, LON_4, "GGA", True),
    ("no_checksum_cr_lf", b"$" + GLL.encode() + b"\r\n", LAT_2, LON_2, "GLL", True),
    # without a checksum the data run to the end: the direction is "W\r\n", which is no "W"
    ("no_checksum_cr_lf_in_a_field", b"$GPGLL,4704.12,N,12503.43,W\r\n", LAT_2, 0.0, "GLL", False),
    ("cr_in_the_middle", b"$GPGLL,4704.12,N,12503.43,W,1\r,A", LAT_2, LON_2, "GLL", False),
    # a byte outside 0x20..0x7E in the middle AND a trailing CR LF: never decided, with a checksum that matches the raw bytes
    # (the host: valid for the ASCII control bytes; 0xE9 decodes to U+FFFD, whose XOR cannot match) and without one
    ("cr_inside_checked_cr_lf", ckb(b"GPGLL,4704.12,N,12503.43,W,1\r,A") + b"\r\n", LAT_2, LON_2, "GLL", False),
    ("tab_inside_checked_cr_lf", ckb(b"GPGLL,4704.12,N,12503.43,W,1\t,A") + b"\r\n", LAT_2, LON_2, "GLL", False),
    ("soh_inside_checked_cr_lf", ckb(b"GPGLL,4704.12,N,12503.43,W,1\x01,A") + b"\r\n", LAT_2, LON_2, "GLL", False),
    ("high_byte_inside_checked_cr_lf", ckb(b"GPGLL,4704.12,N,12503.43,W,\xe9") + b"\r\n", NAN, NAN, "", False),
    ("cr_inside_cr_lf", b"$GPGLL,4704.12,N,12503.43,W,1\r,A\r\n", LAT_2, LON_2, "GLL", False),
    ("tab_inside_cr_lf", b"$GPGLL,4704.12,N,12503.43,W,1\t,A\r\n", LAT_2, LON_2, "GLL", False),
    ("soh_inside_cr_lf", b"$GPGLL,4704.12,N,12503.43,W,1\x01,A\r\n", LAT_2, LON_2, "GLL", False),
    ("high_byte_inside_cr_lf", b"$GPGLL,4704.12,N,12503.43,W,1\xe9,A\r\n", LAT_2, LON_2, "GLL", False),
    # a line feed at the end of the latitude field: the value pattern's `$` matches in front of it, the host gives the value
    ("lf_in_a_value_checked_cr_lf", ckb(b"GPGLL,4704.12\n,N,12503.43,W") + b"\r\n", LAT_2, LON_2, "GLL", False),
    ("soh_in_a_value_checked_cr_lf", ckb(b"GPGLL,4704.12\x01,N,12503.43,W") + b"\r\n", NAN, LON_2, "GLL", False),
    # the same byte in the second step of a wavefront, the trailing run in the third
    ("soh_in_the_second_step_cr_lf", ckb(b"GPGLL,4704.12,N,12503.43,W," + b"7" * 60 + b"\x01" + b"7" * 50) + b"\r\n", LAT_2, LON_2, "GLL",
     False),
    # the digit bound: m = "59.12345678901234" has 16 digits; the answer is still float(d) + float(m) / 60, from the host
    ("16_digit_minutes", ck("GPGLL,4759.12345678901234,N,12503.43,W"), 47 + 59.12345678901234 / 60, LON_2, "GLL", False),
    ("16_digit_degrees", ck("GPGLL,4704.12,N,123456789012345603.43,W"), LAT_2, -(1234567890123456 + 3.43 / 60), "GLL", False),
    ("16_decimals", ck("GPGLL,4704.0000000000000001,N,12503.43,W"), 47 + 4.0000000000000001 / 60, LON_2, "GLL", False),
    ("16_decimals_of_a_small_number", ck("GPGLL,4700.0000000000000001,N,12503.43,W"), 47 + 0.0000000000000001 / 60, LON_2, "GLL",
     False),
    ("15_digits_each", ck("GPGLL,12345678901234559.1234567890123,N,000.1,E"),
     123456789012345 + 59.1234567890123 / 60, 0 + 0.1 / 60, "GLL", True),
    ("leading_zeros", ck("GPGLL,0000000000000000004704.12,N,012503.43,W"), LAT_2, LON_2, "GLL", True),
    # outside the plain form: decided by the host rules
    ("leading_space", b" " + ck(GGA), LAT_4, LON_4, "GGA", False),
    ("no_dollar", ck(GGA)[1:], LAT_4, LON_4, "GGA", False),
    ("high_byte", b"$GPGGA,1\xff,4704.1234,N,12503.4321,W,1", LAT_4, LON_4, "GGA", False),
    ("high_byte_checked", ck("GPGGA,1,4704.1234,N,12503.4321,W,1")[:-3] + b"\xe9*00", NAN, NAN, "", False),
    ("p_talker", ck("PGGGA,1,4704.1234,N,12503.4321,W,1"), NAN, NAN, "", False),
    ("p_talker_lower", ck("pgGGA,1,4704.1234,N,12503.4321,W,1"), NAN, NAN, "", False),
    ("underscore_talker", ck("G_GGA,1,4704.1234,N,12503.4321,W,1"), LAT_4, LON_4, "GGA", False),
    ("lower_case_talker", ck("gpGGA,1,4704.1234,N,12503.4321,W,1"), LAT_4, LON_4, "GGA", True),
    ("lower_case_type", ck("GPgga,1,4704.1234,N,12503.4321,W,1"), LAT_4, LON_4, "GGA", False),
    ("no_comma", b"$GPGGAX,1,4704.1234,N,12503.4321,W,1", NAN, NAN, "", False),
    ("short", b"$GPGGA", NAN, NAN, "", False),
    ("empty", b"", NAN, NAN, "", False),
    # types outside R1 (never selected; handed to the kernel all the same)
    ("zda", R.NMEA[2].encode(), NAN, NAN, "", False),
    ("vtg", R.NMEA[3].encode(), NAN, NAN, "", False),
    ("gpxx", R.NMEA[4].encode(), NAN, NAN, "", False),
    # lengths around one step of a wavefront: the star in front of, on and behind lane 63, and in the third step
    ("length_63", _pad(GGA_SHORT, 63), LAT_4, LON_4, "GGA", True),
    ("length_64", _pad(GGA_SHORT, 64), LAT_4, LON_4, "GGA", True),
    ("length_65", _pad(GGA_SHORT, 65), LAT_4, LON_4, "GGA", True),
    ("length_66", _pad(GGA_SHORT, 66), LAT_4, LON_4, "GGA", True),
    ("length_67", _pad(GGA_SHORT, 67), LAT_4, LON_4, "GGA", True),
    ("length_130", _pad(GGA_SHORT, 130), LAT_4, LON_4, "GGA", True),
    ("length_130_wrong_checksum", _wrong(_pad(GGA_SHORT, 130)), NAN, NAN, "", True),
    # a field that straddles two steps (the longitude lies across lane 63), and the longest field the kernel looks at
    ("field_across_steps", ck("GPRMC," + "1" * 39 + ",A,4704.1234,N,12503.4321,W"), LAT_4, LON_4, "RMC", True),
    ("field_of_65_bytes", ck("GPGLL," + "0" * 58 + "4704.12,N,12503.43,W"), LAT_2, LON_2, "GLL", False),
    ("field_of_64_bytes", ck("GPGLL," + "0" * 57 + "4704.12,N,12503.43,W"), LAT_2, LON_2, "GLL", True),
]
assert [len(s) for n, s, *_ in HAND if n.startswith("length_")] == [63, 64, 65, 66, 67, 130, 130]
# which of them rule R1 selects (s[3:6], whatever stands in front)
SELECTED = {n: s[3:6] in (b"GGA", b"GLL", b"RMC") for n, s, *_ in HAND}
assert not SELECTED["leading_space"] and not SELECTED["no_dollar"] and not SELECTED["zda"] and SELECTED["p_talker"]
assert SELECTED["lower_case_talker"] and not SELECTED["lower_case_type"]

STATUS_INVALID, STATUS_LAT, STATUS_LON, TYPE_SHIFT, STATUS_UNDECIDED = 1, 2, 4, 3, 64
TYPE_CODE = {"GGA": 0, "GLL": 1, "RMC": 2}


def hand_code(lat, lon, kind, decided):
    """The status byte the kernel must give for a HAND entry."""
    if not decided:
        return STATUS_UNDECIDED
    if not kind:
        return STATUS_INVALID
    return (TYPE_CODE[kind] << TYPE_SHIFT) | (STATUS_LAT if lat != lat else 0) | (STATUS_LON if lon != lon else 0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def lay_out(sentences, gaps=None, lead=5):
    """The sentences in one buffer, ``gaps[i]`` bytes of 0xAA behind sentence i (default: i % 4 + 1, so that the starts
    walk through every byte offset mod 4), none behind the last: it ends on the buffer's final byte.
    -> (uint8 array, int64 table (n, 2))."""
    parts, table, pos = [b"\xaa" * lead], [], lead
    for i, s in enumerate(sentences):
        table.append((pos, len(s)))
        gap = 0 if i == len(sentences) - 1 else (i % 4 + 1 if gaps is None else gaps[i])
        parts.append(bytes(s) + b"\xaa" * gap)
        pos += len(s) + gap
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(table, dtype=np.int64).reshape(-1, 2)


def random_plain(n, seed=20261019):
    """``n`` random sentences of the plain form with valid checksums: random type and talker, 1-15 degree digits, minutes
    of 2 + 1..13 digits, random directions (the four letters, none, a wrong one), random fields behind and CR LF at times."""
    rng = np.random.default_rng(seed)

    def digits(k):
        return str(rng.integers(0, 10 ** k)).zfill(k)

    out = []
    for _ in range(n):
        kind = ("GGA", "GLL", "RMC")[rng.integers(3)]
        talker = ("GP", "GN", "IN", "gp", "G1")[rng.integers(5)]
        f = []
        for dirs in ("NS", "EW"):
            d = digits(int(rng.integers(1, 16)))
            m = digits(2) + "." + digits(int(rng.integers(1, 14)))
            f += [d + m, (dirs[0], dirs[1], dirs[0], dirs[1], "", "X")[rng.integers(6)]]
        front = {"GGA": ["123519.00"], "GLL": [], "RMC": ["123519", "A"]}[kind]
        back = [str(rng.integers(0, 10 ** int(rng.integers(1, 8)))) for _ in range(rng.integers(0, 6))]
        s = ck(",".join([talker + kind] + front + f + back))
        out.append(s + (b"\r\n" if rng.integers(4) == 0 else b""))
    return out


# ---- NME0 datagrams between the pings of the `aligned` fixture ------------------------------------------------------------
def nme0_frame(ticks, text, nuls=(0, 0)):
    body = struct.pack("<4sLL", b"NME0", ticks & 0xFFFFFFFF, ticks >> 32) + b"\x00" * nuls[0] + bytes(text) + b"\x00" * nuls[1]
    return struct.pack("<l", len(body)) + body + struct.pack("<l", len(body))


def _dm(value, width):
    """Degrees -> the DDMM.MMMM text of its magnitude."""
    deg = int(abs(value))
    return f"{deg:0{width}d}{(abs(value) - deg) * 60:07.4f}"


def track_sentence(i, lat, lon):
    """Fix i of a track as a sentence: the types rotate, every fifth has no checksum."""
    la, lo = _dm(lat, 2) + "," + ("N" if lat >= 0 else "S"), _dm(lon, 3) + "," + ("E" if lon >= 0 else "W")
    body = (f"GPGGA,1,{la},{lo},1,08", f"GPGLL,{la},{lo},1,A", f"GPRMC,1,A,{la},{lo},9.7")[i % 3]
    return b"$" + body.encode() if i % 5 == 4 else ck(body)


def file_with_track(per_ping=3, extra=()):
    """The ``aligned`` file (2 channels x 4 pings) with ``per_ping`` fixes behind every ping's datagrams, a sentence without
    a position (ZDA) among them, and the ``extra`` (ticks offset, text, nuls) sentences behind the first ping.
    -> (uint8 file bytes, [every sentence's text in file order])."""
    b = R.file_bytes("aligned").tobytes()
    off, size = R.frames("aligned")
    cuts = [int(off[k]) + int(size[k]) + 4 for k in (2, 4, 6, 8)]  # behind the two RAW0 of ping 0, 1, 2, 3
    parts, texts, last, n = [b[:cuts[0]]], [], cuts[0], 0
    for p in range(4):
        if p:
            parts.append(b[last:cuts[p]])
            last = cuts[p]
        t0 = R._ping_ticks(p)
        for j in range(per_ping):
            s = track_sentence(n, 47.0 + 0.00031 * n, -125.0 - 0.00017 * n)
            parts.append(nme0_frame(t0 + 1_000_000 * (j + 1), s))
            texts.append(s)
            n += 1
        parts.append(nme0_frame(t0 + 1_000_000 * (per_ping + 1), R.NMEA[2].encode()))
        texts.append(R.NMEA[2].encode())
        if p == 0:
            for k, (dt, s, nuls) in enumerate(extra):
                parts.append(nme0_frame(t0 + dt, s, nuls))
                texts.append(bytes(s))
    assert last == len(b)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), texts
