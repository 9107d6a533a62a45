"""Positions from NMEA sentences on a real MI355X: the kernel alone, bit-equal to the host restatement of the rules
(``convert.parse_nmea``; the hand-made answers of tests/nmea_cases.py besides); every output element written once and
nothing behind the outputs touched; arguments checked before any launch; and the product -- ``open_raw`` fills
``Platform`` so that ``add_location`` and ``compute_NASC`` run on what it returns.

There is no tolerance anywhere: latitude and longitude are compared as int64 words (-0.0 is not 0.0, NaN is
0x7FF8000000000000), the status byte exactly, and the sentences the kernel leaves to the host are exactly those outside
the plain form, which is a function of the bytes alone."""
import logging

import numpy as np
import pytest

import nmea_cases as C
import raw_cases as R

pytestmark = pytest.mark.gpu

KERNEL = "nmea_positions_kernel"
GUARD = 64
NAN_BITS = 0x7FF8000000000000


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


def _text(s):
    return str(bytes(s), "ascii", errors="replace")


def restated(sentences):
    """What the kernel must give, from the host rules alone -> (lat, lon, code)."""
    from echopype_amd.convert import parse_nmea

    lat, lon, code = np.full(len(sentences), np.nan), np.full(len(sentences), np.nan), np.zeros(len(sentences), np.uint8)
    for i, s in enumerate(sentences):
        if not parse_nmea.plain_form(s):
            code[i] = C.STATUS_UNDECIDED
            continue
        la, lo, kind = parse_nmea.parse_sentence(_text(s))
        code[i] = C.hand_code(la, lo, kind, True)
        if kind:
            lat[i], lon[i] = la, lo
    return lat, lon, code


def _run(ep, sentences, **layout):
    buf, table = C.lay_out(sentences, **layout)
    dev, n = ep.ops.upload_file_bytes(buf)
    assert n == buf.size and int(table[-1].sum()) == n  # the last sentence ends on the file's final byte
    lat, lon, code = ep.ops.nmea_positions(dev, table, n_bytes=n)
    return lat.cpu().numpy(), lon.cpu().numpy(), code.cpu().numpy(), table


def _assert_equal(got, want, sentences):
    for name, g, w in (("latitude", C.bits(got[0]), C.bits(want[0])), ("longitude", C.bits(got[1]), C.bits(want[1])),
                       ("code", got[2], want[2])):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f"{name}: {bad.size} of {len(sentences)} differ, first {sentences[bad[0]]!r}: "
                               f"got {g[bad[0]]}, want {w[bad[0]]}")


@pytest.fixture(scope="module")
def hand():
    sentences = [h[1] for h in C.HAND]
    want = (np.array([h[2] for h in C.HAND]), np.array([h[3] for h in C.HAND]),
            np.array([C.hand_code(*h[2:]) for h in C.HAND], dtype=np.uint8))
    # where the kernel does not decide, or the sentence is invalid, it writes NaN
    silent = (want[2] == C.STATUS_UNDECIDED) | (want[2] == C.STATUS_INVALID)
    return sentences, (np.where(silent, np.nan, want[0]), np.where(silent, np.nan, want[1]), want[2])


def test_kernel_alone_gives_the_hand_values_and_leaves_the_rest_undecided(ep, hand):
    from echopype_amd import _lib

    sentences, want = hand
    buf, table = C.lay_out(sentences)
    assert {int(o) % 4 for o in table[:, 0]} == {0, 1, 2, 3}
    dev, n = ep.ops.upload_file_bytes(buf)
    with _lib.launch_trace() as tr:
        lat, lon, code = ep.ops.nmea_positions(dev, table, n_bytes=n)
    assert tr.kernels == [KERNEL], tr.kernels
    got = (lat.cpu().numpy(), lon.cpu().numpy(), code.cpu().numpy())
    assert got[0].dtype == np.float64 and got[2].dtype == np.uint8
    _assert_equal(got, want, sentences)
    _assert_equal(got, restated(sentences), sentences)  # the restatement says the same
    # the undecided sentences are exactly those designed to be
    assert [h[0] for h, c in zip(C.HAND, got[2]) if c == C.STATUS_UNDECIDED] == [h[0] for h in C.HAND if not h[5]]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_start_offset_and_the_lengths_around_a_step(ep, shift):
    """Sentences of 63 / 64 / 65 / 130 bytes (and the rest of the step cases) starting at every byte offset mod 4."""
    pick = [h for h in C.HAND if h[0].startswith(("length_", "field_"))]
    sentences = [h[1] for h in pick]
    assert {63, 64, 65, 130} <= {len(s) for s in sentences}
    lat, lon, code, table = _run(ep, sentences, gaps=[4 - len(s) % 4 for s in sentences], lead=4 + shift)
    assert {int(o) % 4 for o in table[:, 0]} == {shift}
    _assert_equal((lat, lon, code), restated(sentences), sentences)
    assert list(code) == [C.hand_code(*h[2:]) for h in pick]


@pytest.mark.parametrize("n", [1, 65])
def test_one_sentence_and_more_than_a_block_of_waves(ep, n):
    sentences = [C.HAND[i % len(C.HAND)][1] for i in range(n)] if n > 1 else [C.ck(C.RMC)]
    if n > 1:
        sentences[-1] = C.ck(C.GLL)  # (the last one ends on the final byte: not an empty text)
    lat, lon, code, _ = _run(ep, sentences)
    _assert_equal((lat, lon, code), restated(sentences), sentences)
    if n == 1:
        assert (lat[0], lon[0], code[0]) == (C.LAT_4, C.LON_4, C.TYPE_CODE["RMC"] << C.TYPE_SHIFT)


@pytest.fixture(scope="module")
def random_case():
    sentences = C.random_plain(20000)
    return sentences, restated(sentences)


def test_twenty_thousand_random_plain_sentences_are_all_decided_and_bit_equal(ep, random_case):
    sentences, want = random_case
    assert not np.isnan(want[0]).any() and not np.isnan(want[1]).any()
    types = np.array([C.TYPE_CODE[_text(s)[3:6]] for s in sentences], dtype=np.uint8)
    assert np.array_equal(want[2], types << C.TYPE_SHIFT) and set(types) == {0, 1, 2}  # every status is 0: both values written
    lat, lon, code, _ = _run(ep, sentences)
    _assert_equal((lat, lon, code), want, sentences)
    assert (np.signbit(lat)).any() and (lat == 0).any() and (np.abs(lat) > 1e14).any()


def test_every_element_is_written_once_and_nothing_behind_the_outputs(ep, hand):
    import torch

    sentences, want = hand
    buf, table = C.lay_out(sentences)
    dev, n = ep.ops.upload_file_bytes(buf)
    count = len(sentences)
    results = []
    for fill64, fill8 in ((0x5A5A5A5A5A5A5A5A, 0x5A), (-0x2152411021524111, 0xA5)):  # no result equals either pattern
        flat_lat = torch.full((count + GUARD,), fill64, dtype=torch.int64, device=dev.device)
        flat_lon = torch.full((count + GUARD,), fill64, dtype=torch.int64, device=dev.device)
        flat_code = torch.full((count + GUARD,), fill8, dtype=torch.uint8, device=dev.device)
        out = (flat_lat[:count].view(torch.float64), flat_lon[:count].view(torch.float64), flat_code[:count])
        ep.ops.nmea_positions(dev, table, n_bytes=n, out=out)
        host = [t.cpu().numpy() for t in (flat_lat, flat_lon, flat_code)]
        for h, fill in zip(host, (fill64, fill64, fill8)):
            assert (h[count:] == (fill if h.dtype != np.int64 else np.int64(fill))).all(), "the guard behind an output was written"
            assert not (h[:count] == (fill if h.dtype != np.int64 else np.int64(fill))).any(), "an output element was never written"
        got = (host[0][:count].view(np.float64), host[1][:count].view(np.float64), host[2][:count])
        _assert_equal(got, want, sentences)
        results.append(got)
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()


def test_arguments_are_checked_before_anything_is_launched(ep, hand):
    import torch

    from echopype_amd import _lib

    sentences, _ = hand
    buf, table = C.lay_out(sentences)
    dev, n = ep.ops.upload_file_bytes(buf)
    with _lib.launch_trace() as tr:
        t = table.copy()
        t[3, 1] = n - t[3, 0] + 1  # one byte past the file
        with pytest.raises(ValueError, match="sentence 3 .* leaves the"):
            ep.ops.nmea_positions(dev, t, n_bytes=n)
        t = table.copy()
        t[0, 0] = -1
        with pytest.raises(ValueError, match="leaves the"):
            ep.ops.nmea_positions(dev, t, n_bytes=n)
        with pytest.raises(ValueError, match="padded to a multiple of 16"):
            ep.ops.nmea_positions(dev[:-8], table[:1], n_bytes=int(table[0].sum()))
        with pytest.raises(ValueError, match="padded to a multiple of 16"):
            ep.ops.nmea_positions(dev, table, n_bytes=dev.numel() + 1)
        with pytest.raises(ValueError, match=r"shape \(n, 2\)"):
            ep.ops.nmea_positions(dev, table.reshape(-1, 1), n_bytes=n)
        with pytest.raises(ValueError, match="one-dimensional uint8"):
            ep.ops.nmea_positions(dev.view(torch.int8), table, n_bytes=n)
        with pytest.raises(ValueError, match="out must hold"):
            ep.ops.nmea_positions(dev, table, n_bytes=n, out=(torch.empty(1, dtype=torch.float64, device=dev.device),) * 3)
        count = len(sentences)
        strided = torch.empty(2 * count, dtype=torch.float64, device=dev.device)[::2]
        whole = torch.empty(count, dtype=torch.float64, device=dev.device)
        with pytest.raises(ValueError, match="out must hold contiguous"):
            ep.ops.nmea_positions(dev, table, n_bytes=n, out=(strided, whole, torch.empty(count, dtype=torch.uint8, device=dev.device)))
        with pytest.raises(ValueError, match="on the file's device"):
            ep.ops.nmea_positions(dev, table, n_bytes=n, out=(whole, whole.clone(), torch.empty(count, dtype=torch.uint8)))
        lat, lon, code = ep.ops.nmea_positions(dev, np.zeros((0, 2), np.int64), n_bytes=n)  # n == 0 launches nothing
        assert lat.numel() == lon.numel() == code.numel() == 0
    assert tr.kernels == []
    torch.cuda.synchronize()


# ---- the product ------------------------------------------------------------------------------------------------------
EXTRA = [(5_000_100, b"$GPGLL,4704.12,N,12503.43,W\r\n", (3, 2)),                                # host rules: NULs in front, no checksum
         (5_000_200, b" " + C.ck(C.GGA), (0, 0)),                                                  # not selected (s[3:6] is "PGG")
         (5_000_300, C.ck("GPGLL,4759.12345678901234,N,12503.43,W"), (0, 1))]                      # 16 digits: host rules


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(np.asarray(data, np.uint8).tobytes())
    return str(path)


def _host_platform(ep, texts, times):
    """The Platform group of the reference's rules, on the host alone: R1 on the strings, ``parse_sentence`` on each."""
    from echopype_amd.convert import parse_nmea

    keep = [i for i, t in enumerate(texts) if _text(t)[3:6] in ("GGA", "GLL", "RMC")]
    fixes = [parse_nmea.parse_sentence(_text(texts[i])) for i in keep]
    t = np.asarray(times)[keep]
    plat = ep.Dataset()
    plat["latitude"] = ep.DataArray(np.array([f[0] for f in fixes]), ("time1",), {"time1": t})
    plat["longitude"] = ep.DataArray(np.array([f[1] for f in fixes]), ("time1",), {"time1": t})
    plat["sentence_type"] = ep.DataArray(np.array([f[2] for f in fixes]), ("time1",), {"time1": t})
    return plat


@pytest.fixture(scope="module")
def opened(ep, tmp_path_factory):
    from echopype_amd import _lib

    data, texts = C.file_with_track(extra=EXTRA)
    path = _write(tmp_path_factory.mktemp("nmea"), "track.raw", data)
    with _lib.launch_trace() as tr:
        ed = ep.open_raw(path, "EK60")
    assert tr.kernels.count(KERNEL) == 1, tr.kernels
    return dict(ed=ed, texts=texts, path=path, data=data)


def test_open_raw_fills_platform_and_add_location_equals_the_host_rules(ep, opened):
    ed, texts = opened["ed"], opened["texts"]
    plat, nmea = ed["Platform"], ed["Platform/NMEA"]
    assert list(nmea["NMEA_datagram"].values) == [_text(t) for t in texts]  # Platform/NMEA keeps every sentence
    want = _host_platform(ep, texts, nmea["nmea_time"].values)
    n = len(want["latitude"].values)
    assert n == 12 + 2 and plat["latitude"].dims == ("time1",) and plat["latitude"].dtype == np.float64
    assert np.array_equal(plat["time1"].values, want["time1"].values)
    for v in ("latitude", "longitude"):
        assert np.array_equal(C.bits(plat[v].values), C.bits(want[v].values)), v
        assert plat[v].attrs["standard_name"] == v
    assert list(plat["sentence_type"].values) == list(want["sentence_type"].values)
    assert set(plat["sentence_type"].values) == {"GGA", "GLL", "RMC"} and plat["sentence_type"].values.dtype.kind == "U"
    assert plat["latitude"].attrs["units"] == "degrees_north" and plat["longitude"].attrs["valid_range"] == (-180.0, 180.0)
    # add_location on what open_raw returned equals add_location on the host-parsed Platform, bit for bit
    ds = ep.calibrate.compute_Sv(ed)
    got = ep.consolidate.add_location(ds, ed)
    ref = ep.open_raw(opened["path"], "EK60")
    ref["Platform"] = want
    exp = ep.consolidate.add_location(ep.calibrate.compute_Sv(ref), ref)
    for v in ("latitude", "longitude"):
        a, b = np.asarray(got[v].values), np.asarray(exp[v].values)
        assert a.shape == (4,) and np.isfinite(a).all() and np.array_equal(C.bits(a), C.bits(b)), v
    # one sentence type selects its fixes
    gga = ep.consolidate.add_location(ds, ed, nmea_sentence="GGA")
    gga_ref = ep.consolidate.add_location(ds, ref, nmea_sentence="GGA")
    assert np.array_equal(C.bits(gga["latitude"].values), C.bits(gga_ref["latitude"].values))
    assert not np.array_equal(gga["latitude"].values, got["latitude"].values)


def test_the_chain_from_the_file_to_nasc_runs(ep, opened):
    ed = opened["ed"]
    ds = ep.consolidate.add_depth(ep.calibrate.compute_Sv(ed))
    ds = ep.consolidate.add_location(ds, ed)
    out = ep.commongrid.compute_NASC(ds, range_bin="2m", dist_bin="0.001nmi")
    nasc = np.asarray(out["NASC"].values)
    assert nasc.size > 0 and np.isfinite(nasc).any() and not np.isinf(nasc).any()


def test_combine_of_two_halves_has_the_whole_track(ep, opened, tmp_path):
    data = opened["data"]
    rec_off = []
    pos = 0
    while pos < data.size:  # the framing: [size][body][size]
        size = int(data[pos:pos + 4].view("<i4")[0])
        rec_off.append(pos)
        pos += size + 8
    types = [bytes(data[o + 4:o + 8]) for o in rec_off]
    con_end = rec_off[1]
    # the second half begins with the first RAW0 of ping 2: the fifth RAW0 datagram
    mid = [o for o, t in zip(rec_off, types) if t == b"RAW0"][4]
    a = ep.open_raw(_write(tmp_path, "a.raw", data[:mid]), "EK60")
    b = ep.open_raw(_write(tmp_path, "b.raw", np.concatenate([data[:con_end], data[mid:]])), "EK60")
    both, whole = ep.combine_echodata([a, b]), opened["ed"]
    pw, pb = whole["Platform"], both["Platform"]
    assert np.array_equal(pb["time1"].values, pw["time1"].values)
    for v in ("latitude", "longitude"):
        assert np.array_equal(C.bits(pb[v].values), C.bits(pw[v].values)), v
    assert list(pb["sentence_type"].values) == list(pw["sentence_type"].values)


@pytest.mark.parametrize("case", ["aligned", "ragged"])
def test_the_existing_fixtures_still_open(ep, tmp_path, caplog, case):
    """``aligned`` has no sentence: the placeholder.  ``ragged``'s GGA / GLL sentences have ONE hex digit behind the star:
    they stay invalid -- NaN fixes and "" -- and ``add_location`` refuses the all-NaN track as the reference does."""
    from echopype_amd import _lib

    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING, logger="echopype_amd.convert.api"):
        ed = ep.open_raw(_write(tmp_path, f"{case}.raw", R.file_bytes(case)), "EK60")
    plat = ed["Platform"]
    n = {"aligned": 1, "ragged": 10}[case]
    assert tr.kernels.count(KERNEL) == (0 if case == "aligned" else 1)
    assert plat["latitude"].values.shape == (n,) and np.isnan(plat["latitude"].values).all()
    assert np.isnan(plat["longitude"].values).all() and list(plat["sentence_type"].values) == [""] * n
    assert not any("problematic" in r.getMessage() for r in caplog.records)  # (invalid sentences are not R5 failures)
    if case == "aligned":
        assert plat["time1"].values[0] == ed["Sonar/Beam_group1"]["ping_time"].values.min()
    else:
        texts = list(ed["Platform/NMEA"]["NMEA_datagram"].values)
        assert len(texts) == 23 and sum(t[3:6] in ("GGA", "GLL") for t in texts) == n
    with pytest.raises(ValueError, match="Coordinate variables are all NaN."):
        ep.consolidate.add_location(ep.calibrate.compute_Sv(ed), ed)


def test_a_field_that_is_no_position_warns_once_per_file(ep, tmp_path, caplog):
    extra = [(5_000_100, C.ck("GPGLL,04.12,N,12503.43,W"), (0, 0)), (5_000_200, C.ck("GPGLL,4.12,N,12503.43,W"), (0, 0)),
             (5_000_300, C.ck("GPGGA,1,4704.12,N,125o3.43,W"), (0, 0))]
    data, texts = C.file_with_track(per_ping=1, extra=extra)
    with caplog.at_level(logging.WARNING, logger="echopype_amd.convert.api"):
        ed = ep.open_raw(_write(tmp_path, "warn.raw", data), "EK60")
    said = [r.getMessage() for r in caplog.records if "problematic" in r.getMessage()]
    assert len(said) == 2, said
    assert "At least one latitude entry is problematic and are assigned None in the converted data: " in said[0]
    assert "'04.12'" in said[0] and "At least one longitude entry is problematic" in said[1] and "'125o3.43'" in said[1]
    plat = ed["Platform"]
    kinds, lat, lon = list(plat["sentence_type"].values), plat["latitude"].values, plat["longitude"].values
    assert kinds[1:5] == ["GLL", "GLL", "GGA", "GLL"]  # (the type stays when a value fails)
    assert np.isnan(lat[1]) and np.isnan(lat[2]) and lon[1] == C.LON_2 and lat[3] == C.LAT_2 and np.isnan(lon[3])
