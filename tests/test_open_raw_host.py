"""Everything of ``open_raw`` that needs no device -- the CON0 fields, the vectorised RAW0 header gather, ``ping_time``,
the channel order and the row table -- against what the REFERENCE's parsers read from the same bytes
(tests/golden/open_raw_ek60.npz, scripts/gen_open_raw_goldens.py); the argument errors; the signature."""
import inspect
import json

import numpy as np
import pytest

import raw_cases as R


def _plan(case):
    from echopype_amd.convert import parse_ek60

    return parse_ek60.plan(R.file_bytes(case))


@pytest.mark.parametrize("case", R.GOOD)
def test_con0_fields_equal_the_reference_parser(case):
    cfg, ref = _plan(case).config, R.config(case)
    for k in ("survey_name", "transect_name", "sounder_name", "version", "spare0", "transceiver_count", "low_date", "high_date"):
        assert cfg[k] == ref[k], k
    assert sorted(cfg["transceivers"]) == sorted(int(k) for k in ref["transceivers"])
    for k, t in cfg["transceivers"].items():
        rt = ref["transceivers"][str(k)]
        assert sorted(t) == sorted(rt)
        for f, v in t.items():
            if isinstance(v, np.ndarray):  # the three tables, round(x, 6) included
                assert v.dtype == np.float64 and v.tolist() == rt[f], (k, f)
            else:
                assert v == rt[f] and type(v) is type(rt[f]), (k, f)


@pytest.mark.parametrize("case", R.GOOD)
def test_header_gather_times_order_and_table(case):
    from echopype_amd.convert import parse_ek60

    pl, e, g = _plan(case), R.expected(case), R.golden()
    assert pl.transceivers == e["transceivers"] and pl.channel == e["channel"]
    assert (pl.C, pl.P, pl.S) == (e["C"], e["P"], e["S"])
    assert pl.ping_time.dtype == np.dtype("datetime64[ns]") and np.array_equal(pl.ping_time, e["ping_time"])
    assert pl.n_consumed == R.file_bytes(case).size
    assert pl.angles == (None if e["athw"] is None else "int8" if e["angles_int8"] else "float32")
    # per-ping header fields on (channel, ping_time), NaN where a channel lacks a ping
    for f in R.RAW0_FLOATS + ("offset",):
        got = parse_ek60.per_ping(pl, f)
        assert got.dtype == np.float64 and np.array_equal(got, e["hdr"][f], equal_nan=True), f
    for f in ("mode", "transmit_mode"):
        got = parse_ek60.per_ping(pl, f, np.int8)
        full = not np.isnan(e["hdr"][f]).any()
        assert got.dtype == (np.int8 if full else np.float32)
        assert np.array_equal(got.astype(np.float64), e["hdr"][f], equal_nan=True)
    # the row table: offsets and counts point at the samples the reference parsed
    tab, data = pl.table.reshape(pl.C, pl.P, 3), R.file_bytes(case)
    count = np.where(np.isnan(e["hdr"]["count"]), 0, e["hdr"]["count"]).astype(np.int64)
    assert np.array_equal(tab[:, :, 2], count)
    assert np.array_equal(tab[:, :, 0] < 0, np.isnan(e["hdr"]["count"]))
    for c in range(pl.C):
        for p in range(pl.P):
            off_p, off_a, n = (int(v) for v in tab[c, p])
            if off_p >= 0:
                pw = data[off_p:off_p + 2 * n].view("<i2").astype(np.float32) * R.INDEX2POWER
                assert np.array_equal(pw.view(np.int32), e["power"][c, p, :n].view(np.int32))
                assert np.isnan(e["power"][c, p, n:]).all()
            else:
                assert np.isnan(e["power"][c, p]).all()
            if e["athw"] is not None:
                if off_a >= 0:
                    an = data[off_a:off_a + 2 * n].view(np.int8).reshape(-1, 2).astype(np.float32)
                    assert np.array_equal(an[:, 0], e["athw"][c, p, :n]) and np.array_equal(an[:, 1], e["along"][c, p, :n])
                else:
                    assert np.isnan(e["athw"][c, p]).all()
    # NME0 sentences and their times
    assert np.array_equal(pl.nmea_time, g[f"{case}/nmea_time"]) and list(pl.nmea) == list(g[f"{case}/nmea_text"])


def test_ragged_case_exercises_what_it_is_there_for():
    pl = _plan("ragged")
    assert pl.transceivers == [2, 3, 1] and pl.skipped_zero_time == 1
    assert pl.rows_present == pl.C * pl.P - 1 and pl.angles == "float32"
    tab = pl.table.reshape(pl.C, pl.P, 3)
    assert (tab[1, :, 1] == -1).all() and (tab[1, :, 0] >= 0).all()  # the mode-1 channel: power, no angles
    assert {int(v) % 4 for v in tab[:, :, 0].ravel() if v >= 0} == {0, 1, 2, 3}
    assert {int(v) % 4 for v in tab[:, :, 1].ravel() if v >= 0} == {0, 1, 2, 3}
    assert sorted(set(tab[:, :, 2].ravel())) == sorted(R.RAGGED_COUNTS)


def test_nt_to_ns_rounds_like_timedelta():
    """Half a microsecond goes to the even neighbour of what the float64 product gives, as datetime.timedelta rounds."""
    import datetime

    from echopype_amd.convert.parse_ek60 import nt_to_ns

    rng = np.random.default_rng(5)
    ticks = np.concatenate([R.NT_BASE + rng.integers(0, 10**10, 2000), R.NT_BASE + 10 * rng.integers(0, 10**9, 500) + 5,
                            np.array([1, 5, 15, 25, 10**17])])
    low, high = (ticks & 0xFFFFFFFF).astype(np.uint32), (ticks >> 32).astype(np.uint32)
    epoch = datetime.datetime(1601, 1, 1)
    want = np.array([np.datetime64(epoch + datetime.timedelta(seconds=((int(h) << 32) + int(lo)) * 1.0e-7), "ns")
                     for lo, h in zip(low, high)])
    assert np.array_equal(nt_to_ns(low, high), want)


@pytest.mark.parametrize("name", sorted(R.cut_variants()))
def test_plan_of_a_cut_file(name):
    from echopype_amd.convert import parse_ek60

    data, n_dgram = R.cut_variants()[name]
    if n_dgram == 1:
        with pytest.raises(ValueError, match="no RAW0 datagram with power"):
            parse_ek60.plan(data)
        return
    pl, e = parse_ek60.plan(data), R.expected("aligned")
    assert pl.n_consumed < data.size and pl.rows_present == n_dgram - 1 == pl.C * pl.P - 1
    assert np.array_equal(pl.ping_time, e["ping_time"]) and pl.angles == "float32"
    assert tuple(pl.table.reshape(pl.C, pl.P, 3)[0, 3]) == (-1, -1, 0)  # transceiver 2 sorts first and lost its last ping


def test_bad_files_raise_the_named_exceptions():
    from echopype_amd.convert import parse_ek60

    with pytest.raises(ValueError, match="starts with a CON0 datagram, this one with RAW0"):
        parse_ek60.plan(R.file_bytes("nocon"))
    with pytest.raises(NotImplementedError, match="mode 2"):
        parse_ek60.plan(R.file_bytes("mode2"))
    for name, (data, where, _) in R.bad_variants().items():
        with pytest.raises(ValueError, match=f"byte offset {where}"):
            parse_ek60.plan(data)
    with pytest.raises(ValueError, match="this one with nothing"):
        parse_ek60.plan(np.zeros(0, np.uint8))


def test_argument_errors_come_before_any_file_or_device_access():
    import echopype_amd as ep

    assert ep.open_raw is ep.convert.open_raw
    for model in ("EK80", "AZFP", "ES70", None):
        with pytest.raises(NotImplementedError, match="sonar_model"):
            ep.open_raw("no_such_file.raw", model)
    for kw in ({"xml_path": "a.xml"}, {"include_bot": True}, {"include_idx": True}, {"storage_options": {"anon": True}},
               {"use_swap": True}, {"use_swap": "auto"}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            ep.open_raw("no_such_file.raw", "ek60", **kw)
    with pytest.raises(FileNotFoundError):
        ep.open_raw("no_such_file.raw", "ek60")


def test_signature_equals_the_reference():
    import echopype_amd as ep

    ref = json.load(open(R.SIGNATURE))["convert.open_raw"]["params"]
    got = list(inspect.signature(ep.convert.open_raw).parameters.values())
    assert [p.name for p in got] == [r[0] for r in ref]
    for p, (name, kind, src) in zip(got, ref):
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and kind == "positional_or_keyword"
        if src is None:
            assert p.default is inspect.Parameter.empty
        else:
            want = eval(src, {})  # noqa: S307 - literals from the committed fixture
            assert p.default == want and type(p.default) is type(want), name
