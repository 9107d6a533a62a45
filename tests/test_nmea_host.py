"""The rules that turn NMEA sentences into positions (``convert.parse_nmea``), without a device: ``parse_sentence`` against
answers worked out by hand (tests/nmea_cases.py), bit for bit; the plain form the kernel decides; the selection of rule R1
on the file's bytes, leading NULs included; the entry of a file without a fix; the new symbol declared and bound."""
import math
import os
import re

import numpy as np
import pytest

import nmea_cases as C
import raw_cases as R


def _text(s):
    return str(bytes(s), "ascii", errors="replace")


@pytest.mark.parametrize("name,sentence,lat,lon,kind,decided", C.HAND, ids=[h[0] for h in C.HAND])
def test_parse_sentence_gives_the_hand_values_bit_for_bit(name, sentence, lat, lon, kind, decided):
    from echopype_amd.convert import parse_nmea

    got = parse_nmea.parse_sentence(_text(sentence))
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert C.bits([got[0]])[0] == C.bits([lat])[0], (got[0], lat)  # (-0.0 is not 0.0 here, and NaN is math.nan's word)
    assert C.bits([got[1]])[0] == C.bits([lon])[0], (got[1], lon)
    assert got[2] == kind
    assert parse_nmea.plain_form(sentence) is decided


def test_the_hand_values_are_what_they_are_meant_to_be():
    by_name = {h[0]: h for h in C.HAND}
    assert by_name["gga"][2] == 47.06872333333333 and by_name["gga"][3] == -125.05720166666667
    assert math.copysign(1.0, by_name["zero_south_west"][2]) == -1.0 and math.copysign(1.0, by_name["zero_north_east"][2]) == 1.0
    assert C.bits([math.nan])[0] == 0x7FF8000000000000
    assert by_name["one_hex_digit"][1] == R.NMEA[1].encode() and by_name["one_hex_digit"][4] == ""
    decided = [h[5] for h in C.HAND]
    assert 20 < sum(decided) < len(decided) - 20  # both sides are well represented


def test_random_plain_sentences_are_plain_and_valid():
    from echopype_amd.convert import parse_nmea

    for s in C.random_plain(300, seed=3):
        assert parse_nmea.plain_form(s)
        lat, lon, kind = parse_nmea.parse_sentence(_text(s))
        assert kind in parse_nmea.TYPES and lat == lat and lon == lon


def test_value_arithmetic_is_the_integer_division_the_kernel_does():
    """Under the digit bound ``float(m)`` equals (digits of m as an integer) / 10^k in float64: what the kernel computes."""
    from echopype_amd.convert import parse_nmea

    rng = np.random.default_rng(11)
    for _ in range(3000):
        k = int(rng.integers(1, 14))
        m = str(rng.integers(0, 100)).zfill(2) + "." + str(rng.integers(0, 10 ** k)).zfill(k)
        d = str(rng.integers(0, 10 ** int(rng.integers(1, 16))))
        want = float(int(d)) + (float(int(m.replace(".", ""))) / float(10 ** k)) / 60.0
        assert parse_nmea.value(d + m) == want


def test_selection_on_the_bytes_with_leading_nuls():
    from echopype_amd.convert import parse_ek60, parse_nmea

    extra = [(77, b"$GPGLL,4704.12,N,12503.43,W\r\n", (3, 2)), (78, C.ck(C.GGA), (1, 0)), (79, b"  $GGAXQ,RMC", (0, 4)),
             (80, b"xyzRMC", (2, 2)), (81, b"$GPGG", (0, 0)), (82, b"", (4, 0))]
    data, texts = C.file_with_track(extra=extra)
    pl = parse_ek60.plan(data)
    assert pl.nmea == [_text(t) for t in texts]
    # the offsets and lengths are those of the stripped text: leading NULs move the start
    for t, o, n in zip(texts, pl.nmea_offset, pl.nmea_length):
        assert bytes(data[int(o):int(o) + int(n)]) == bytes(t)
    assert pl.nmea_offset.dtype == np.int64 and pl.nmea_length.dtype == np.int64
    want = [i for i, t in enumerate(pl.nmea) if t[3:6] in ("GGA", "GLL", "RMC")]
    assert list(pl.nmea_selected) == want
    assert _text(b"  $GGAXQ,RMC") in [pl.nmea[i] for i in want] and "xyzRMC" in [pl.nmea[i] for i in want]
    assert not any(pl.nmea[i].startswith("$GPZDA") for i in want)
    # the same through the function alone, and on the HAND sentences
    buf, table = C.lay_out([h[1] for h in C.HAND])
    got = parse_nmea.select(buf, table[:, 0], table[:, 1])
    assert list(got) == [C.SELECTED[h[0]] for h in C.HAND]
    assert parse_nmea.select(buf, np.zeros(0, np.int64), np.zeros(0, np.int64)).size == 0


def test_a_file_without_fixes_gets_the_placeholder_entry():
    from echopype_amd.convert import api, parse_ek60, parse_nmea

    pl = parse_ek60.plan(R.file_bytes("aligned"))
    assert pl.nmea_selected.size == 0
    t, lat, lon, kind = api.positions(pl, None)
    assert t.dtype == np.dtype("datetime64[ns]") and list(t) == [pl.ping_time.min()]
    assert np.isnan(lat).all() and np.isnan(lon).all() and lat.shape == lon.shape == (1,) and lat.dtype == np.float64
    assert list(kind) == [""] and kind.dtype.kind == "U"
    t2, *_ = parse_nmea.placeholder(pl.ping_time[::-1])
    assert t2[0] == pl.ping_time[0]
    # the ragged fixture: its GGA / GLL sentences have one hex digit, they are selected and do not parse
    pl = parse_ek60.plan(R.file_bytes("ragged"))
    assert pl.nmea_selected.size == 10
    assert all(parse_nmea.parse_sentence(pl.nmea[i])[2] == "" for i in pl.nmea_selected)


def test_the_symbol_is_declared_and_bound():
    from echopype_amd import _lib, ops

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "echopype_amd.h")).read()
    assert re.search(r"\bint epa_nmea_positions\(", header)
    assert len(_lib.SIGNATURES["epa_nmea_positions"]) == 10 and hasattr(_lib.lib, "epa_nmea_positions")
    for name, value in (("EPA_NMEA_INVALID", _lib.NMEA_INVALID), ("EPA_NMEA_LAT_FAILED", _lib.NMEA_LAT_FAILED),
                        ("EPA_NMEA_LON_FAILED", _lib.NMEA_LON_FAILED), ("EPA_NMEA_UNDECIDED", _lib.NMEA_UNDECIDED),
                        ("EPA_NMEA_TYPE_SHIFT", _lib.NMEA_TYPE_SHIFT)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert re.search(r"#define EPA_NMEA_TYPE_MASK 0x18\b", header) and _lib.NMEA_TYPE_MASK == 0x18
    assert (C.STATUS_INVALID, C.STATUS_LAT, C.STATUS_LON, C.TYPE_SHIFT, C.STATUS_UNDECIDED) == (1, 2, 4, 3, 64)
    assert "nmea.hip" in __import__("echopype_amd.build", fromlist=["SOURCES"]).SOURCES and callable(ops.nmea_positions)
    assert _lib.lib.epa_version() == 104


def test_arguments_are_refused_without_a_device():
    """The entry point's own checks run before any HIP call."""
    import ctypes

    from echopype_amd import _lib

    tab = np.array([[0, 17]], dtype=np.int64)
    p = tab.ctypes.data_as(ctypes.c_void_p)
    with pytest.raises(ValueError, match="leaves the 16 file bytes"):
        _lib.call("epa_nmea_positions", p, 16, 16, p, p, 1, p, p, p, None)
    with pytest.raises(ValueError, match="padded to a multiple of 16"):
        _lib.call("epa_nmea_positions", p, 16, 24, p, p, 1, p, p, p, None)
    with pytest.raises(ValueError, match="NULL array argument"):
        _lib.call("epa_nmea_positions", p, 16, 16, p, p, 1, None, p, p, None)
    with pytest.raises(ValueError, match="not served"):
        _lib.call("epa_nmea_positions", p, 16, 16, p, p, -1, p, p, p, None)
    _lib.call("epa_nmea_positions", None, 0, 0, None, None, 0, None, None, None, None)  # n == 0: nothing to do
