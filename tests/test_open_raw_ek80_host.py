"""The host half of ``open_raw_ek80`` (convert/parse_ek80.py) against what the REFERENCE's parsers read from the same bytes
(tests/golden/open_raw_ek80.npz, made by scripts/gen_open_raw_ek80_goldens.py): the groups and their row tables, the
parameter pairing, the configuration, environment, filters and motion records; the XML texts parsed once per distinct
text; broken and cut files; the entry point's argument checks.  No GPU."""
import inspect
import json
import logging

import numpy as np
import pytest

import raw3_cases as R

GOOD = sorted(R.CASES)


def _plan(case):
    from echopype_amd.convert import parse_ek80

    return parse_ek80.plan(R.file_bytes(case))


@pytest.mark.parametrize("case", GOOD)
def test_the_fixture_holds_the_bytes_the_packers_give(case):
    g = R.golden()
    data, off, size, specs = R.built(case)
    assert np.array_equal(g[f"{case}/bytes"], data) and np.array_equal(g[f"{case}/rec_offset"], off)
    assert np.array_equal(g[f"{case}/rec_size"], size) and [t.decode() for t in g[f"{case}/rec_type"]] == [d["kind"] for d in specs]


def test_the_cases_hold_what_they_are_for():
    res = lambda case: {c % 4 for _, _, _, c in R.block_offsets(case) if c >= 0}  # noqa: E731
    assert res("fm") == {0, 1, 2, 3} and res("edges") == {0, 1, 2, 3}
    fm = R.ref_channel("fm", R.CH70)
    assert np.isnan(fm["imag"][0, 3, 1]) and fm["real"][0, 3, 1] == 1.5          # imaginary part 0.0
    assert np.isnan(fm["imag"][0, 4, 2]) and fm["real"][0, 4, 2] == -2.25        # ... -0.0
    assert np.isnan(fm["real"][0, 5, 0]) and np.isnan(fm["imag"][0, 5, 0])       # a NaN sample
    assert fm["real"][0, 6, 3] == 0.0 and fm["imag"][0, 6, 3] == 3.0             # a real part 0.0 stays
    assert list(R.expected_groups("mixed")) == ["complex_FM", "complex_CW", "power"]
    assert [c for c in R.ref_channels("mixed") if "EC150" in c] == []
    sizes = {int(p["count"]) * b for cid, b in R.EDGE_CHANNELS for p in R.ref_channel("edges", cid)["params"]}
    assert sizes == set(R.EDGE_SIZES)


def _expected_tables(case):
    """{descr: int64 (C * P, 3)} from where the generator laid the blocks and the reference's ping times."""
    _, _, _, specs = R.built(case)
    blocks = {i: b for i, *b in R.block_offsets(case)}
    where, seen = {}, {}
    for i, d in enumerate(specs):
        if d["kind"] != "RAW3" or "EC150" in d["channel_id"]:
            continue
        k = seen.get(d["channel_id"], 0)
        seen[d["channel_id"]] = k + 1
        t = R.ref_channel(case, d["channel_id"])["ping_time"][k]
        where[d["channel_id"], t] = (blocks[i], d)
    out = {}
    for descr, e in R.expected_groups(case).items():
        tab = np.zeros((e["C"], e["P"], 3), np.int64)
        tab[..., 0] = -1
        if descr == "power":
            tab[..., 1] = -1
        for ci, cid in enumerate(e["channel"]):
            for pi, t in enumerate(e["ping_time"]):
                if e["params"]["count"][ci, pi] is None:
                    continue
                (p, a, c), d = where[cid, t]
                if d["count"] == 0:  # an empty block is no block
                    p = a = c = -1
                if descr == "power":
                    tab[ci, pi] = (p, a if e["has_angle"][ci] else -1, d["count"] if p >= 0 else 0)
                else:
                    tab[ci, pi] = (c, d["count"] if c >= 0 else 0, d["data_type"] >> 8 if d["count"] else 0)
        out[descr] = tab.reshape(-1, 3)
    return out


@pytest.mark.parametrize("case", GOOD)
def test_plan_gives_the_groups_and_row_tables_of_the_reference_parse(case):
    pl, want = _plan(case), R.expected_groups(case)
    assert [g.descr for g in pl.groups] == list(want)
    tables = _expected_tables(case)
    for g in pl.groups:
        e = want[g.descr]
        assert g.channel == e["channel"] and g.channel == sorted(g.channel)
        assert np.array_equal(g.ping_time, e["ping_time"]) and g.ping_time.dtype == np.dtype("datetime64[ns]")
        assert (g.C, g.P, g.S) == (e["C"], e["P"], e["S"]) and g.B == e.get("B")
        assert g.table.dtype == np.int64 and np.array_equal(g.table, tables[g.descr]), g.descr
    if case == "mixed":
        power = pl.groups[2]
        assert power.angles == "float32" and (power.table[:power.P, 1] >= 0).all() and (power.table[power.P:, 1] == -1).all()
        cw = pl.groups[1]
        assert tuple(cw.table.reshape(cw.C, cw.P, 3)[1, 2]) == (-1, 0, 0)  # the 3-sector channel lacks ping 2
        assert set(cw.table.reshape(cw.C, cw.P, 3)[1, [0, 1, 3], 2]) == {3} and cw.B == 4
        assert pl.raw4_count == 1 and pl.mru1_count == 1
        assert not any("EC150" in c for c in pl.config) and not any("EC150" in c for c in pl.ping_channel)


@pytest.mark.parametrize("case", GOOD)
def test_every_ping_gets_the_parameters_the_reference_pairs_it_with(case):
    from echopype_amd.convert import parse_ek80

    pl = _plan(case)
    for g in pl.groups:
        e = R.expected_groups(case)[g.descr]["params"]
        for key, dt in (("sample_interval", np.float64), ("transmit_power", np.float64), ("slope", np.float64),
                        ("pulse_duration", np.float64), ("channel_mode", np.float64), ("pulse_form", np.float64),
                        ("frequency", np.float64), ("frequency_start", np.float64), ("frequency_end", np.float64)):
            if key not in e:
                continue
            got = parse_ek80.per_ping(pl, g, parse_ek80.param_field(pl, key, dt))
            want = np.array([[np.nan if v is None else float(v) for v in row] for row in e[key]])
            assert np.array_equal(got, want, equal_nan=True), (g.descr, key)
        for key, src in (("offset", pl.headers["offset"]), ("count", pl.count), ("data_type", pl.headers["data_type"])):
            got = parse_ek80.per_ping(pl, g, src.astype(np.float64))
            want = np.array([[np.nan if v is None else float(v) for v in row] for row in e[key]])
            assert np.array_equal(got, want, equal_nan=True), (g.descr, key)
    ids = [p["channel_id"] for p in pl.params]
    assert list(np.array(ids, dtype=object)[pl.ping_param]) == list(pl.ping_channel)


def _same_json(a, b):
    return json.loads(json.dumps(a, sort_keys=True)) == json.loads(json.dumps(b, sort_keys=True))


@pytest.mark.parametrize("case", GOOD)
def test_configuration_environment_filters_and_motion_equal_the_reference_parse(case):
    pl = _plan(case)
    plain = lambda v: v.tolist() if isinstance(v, np.ndarray) else ({k: plain(x) for k, x in v.items()} if isinstance(v, dict) else v)  # noqa: E731
    want = R.golden_json(case, "config")
    assert sorted(pl.config) == sorted(want)
    for cid in want:
        assert _same_json(plain(pl.config[cid]), want[cid]), cid
    env = R.golden_json(case, "environment")
    t, xml = env.pop("timestamp"), env.pop("xml")
    assert _same_json(pl.environment, env) and pl.environment_xml == xml
    assert int(pl.environment_time.astype("datetime64[ns]").astype(np.int64)) == t
    if case == "mixed":  # the drop-keel datagram behind the real one does not replace it
        assert pl.environment["sound_speed"] == 1492.25 and pl.environment["drop_keel_offset"] == 0.0
    fil = R.golden_json(case, "fil")
    assert sum(len(v) for v in pl.fil.values()) == len(fil)
    for f in fil:
        hits = [(tt, c, d) for tt, c, d in pl.fil[f["channel_id"], f["stage"]] if int(tt.astype(np.int64)) == f["time_ns"]]
        assert len(hits) == 1
        _, c, d = hits[0]
        assert c.dtype == np.complex64 and d == f["decimation_factor"]
        assert np.array_equal(c.real, np.array(f["real"], np.float32)) and np.array_equal(c.imag, np.array(f["imag"], np.float32))
    assert np.array_equal(pl.filter_time.astype(np.int64), np.unique([f["time_ns"] for f in fil]).astype(np.int64))
    mru = R.golden_json(case, "mru0")
    assert pl.mru0.size == len(mru.get("timestamp", []))
    for key in ("heave", "roll", "pitch", "heading"):
        assert np.array_equal(pl.mru0[key].astype(np.float64), np.array(mru.get(key, []), np.float64))
    assert np.array_equal(pl.mru0_time.astype(np.int64), np.array(mru.get("timestamp", []), np.int64))
    assert list(pl.nmea) == list(R.golden()[f"{case}/nmea_text"]) and np.array_equal(pl.nmea_time, R.golden()[f"{case}/nmea_time"])


def test_xml_texts_are_parsed_once_per_distinct_text(monkeypatch):
    from echopype_amd.convert import parse_ek80

    calls = []
    real = parse_ek80.parse_xml_text
    monkeypatch.setattr(parse_ek80, "parse_xml_text", lambda raw: calls.append(bytes(raw)) or real(raw))
    for case in GOOD:
        calls.clear()
        data, off, size, specs = R.built(case)
        pl = parse_ek80.plan(data)
        texts = [data[int(o) + 12:int(o) + int(n)].tobytes() for d, o, n in zip(specs, off, size) if d["kind"] == "XML0"]
        assert len(calls) == len(set(calls)) == len(set(texts)) == pl.xml_texts and pl.xml_count == len(texts)
    assert len(set(texts)) < len(texts)
    # many pings of one channel: still one parse per distinct text
    calls.clear()
    par = R.xml0(R.NT_BASE, R.parameter_xml(R.CH70, 0, 0.000512, 8e-06, 100.0, 0.5, freq=70000.0))
    specs = [R.xml0(R.NT_BASE - 5, R.config_xml([R.channel_config(R.CH70, 1, 70000.0)]))]
    for p in range(200):
        specs += [dict(par, ticks=R.NT_BASE + p * 1000), R.raw3(R.NT_BASE + p * 1000, R.CH70, 2, 4, np.ones((2, 4), np.complex64))]
    pl = parse_ek80.plan(R.assemble(specs)[0])
    assert len(calls) == 2 and pl.groups[0].P == 200 and len(pl.params) == 1


def test_broken_files_raise_the_named_exceptions():
    from echopype_amd.convert import parse_ek80

    for name, (data, exc, text) in R.bad_variants().items():
        with pytest.raises(exc, match=text):
            parse_ek80.plan(data)
    with pytest.raises(ValueError, match="this one with nothing"):
        parse_ek80.plan(np.zeros(0, np.uint8))
    data = R.file_bytes("fm").copy()
    data[4:8] = np.frombuffer(b"RAW3", np.uint8)
    with pytest.raises(ValueError, match="this one with RAW3"):
        parse_ek80.plan(data)
    # two pings of one channel with one time stamp
    specs = R.fm()
    raws = [i for i, d in enumerate(specs) if d["kind"] == "RAW3" and d["channel_id"] == R.CH70]
    specs[raws[1]]["ticks"] = specs[raws[0]]["ticks"]
    with pytest.raises(ValueError, match="two pings with one time stamp"):
        parse_ek80.plan(R.assemble(specs)[0])


@pytest.mark.parametrize("name", sorted(R.cut_variants()))
def test_a_cut_file_keeps_the_pings_in_front_and_warns(name, caplog):
    from echopype_amd.convert import api_ek80

    data, n_dgram = R.cut_variants()[name]
    with caplog.at_level(logging.WARNING, logger="echopype_amd.convert.api_ek80"):
        pl = api_ek80.host_plan(data, data.size, "cut.raw")
    assert any("ends inside a datagram" in r.getMessage() for r in caplog.records)
    assert pl.records.size == n_dgram and pl.n_consumed < data.size
    g, e = pl.groups[0], R.expected_groups("fm")["complex_FM"]
    assert g.rows_present == g.C * g.P - 1 and np.array_equal(g.ping_time, e["ping_time"])
    assert tuple(g.table.reshape(g.C, g.P, 3)[1, 2]) == (-1, 0, 0)  # the last RAW3: channel 120 kHz, ping 2


def test_skipped_datagrams_are_logged_once_per_file(caplog):
    from echopype_amd.convert import api_ek80

    data = R.file_bytes("mixed")
    with caplog.at_level(logging.INFO, logger="echopype_amd.convert.api_ek80"):
        api_ek80.host_plan(data, data.size, "mixed.raw")
    assert sum("RAW4" in r.getMessage() for r in caplog.records) == 1 and sum("MRU1" in r.getMessage() for r in caplog.records) == 1


def test_the_entry_point_is_exported_and_checks_its_arguments_first():
    import echopype_amd as ep

    assert ep.open_raw_ek80 is ep.convert.open_raw_ek80 and "open_raw_ek80" in ep.__all__ and "open_raw_ek80" in ep.convert.__all__
    sig = inspect.signature(ep.open_raw_ek80)
    assert str(sig) == ("(raw_file, include_bot=False, include_idx=False, convert_params=None, storage_options=None, "
                        "use_swap=False, max_chunk_size='100MB')")
    for kw in ({"include_bot": True}, {"include_idx": True}, {"storage_options": {"anon": True}}, {"use_swap": True},
               {"use_swap": "auto"}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            ep.open_raw_ek80("no_such_file.raw", **kw)
    with pytest.raises(FileNotFoundError):
        ep.open_raw_ek80("no_such_file.raw")
    with pytest.raises(FileNotFoundError):
        ep.open_raw_ek80(None)
    assert "open_raw(" in ep.open_raw_ek80.__doc__ and "NotImplementedError" in ep.open_raw_ek80.__doc__
    assert "open_raw_ek80" in ep.open_raw.__doc__


def test_open_raw_still_refuses_ek80():
    import echopype_amd as ep

    with pytest.raises(NotImplementedError, match="sonar_model"):
        ep.open_raw("no_such_file.raw", "EK80")


def test_abi_and_wrapper_are_wired():
    import re

    from echopype_amd import _lib, ops
    from echopype_amd.convert import raw3_unpack

    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib.__file__), "..", "include", "echopype_amd.h")).read()
    assert re.search(r"\bint epa_raw3_unpack\(", header)
    assert len(_lib.SIGNATURES["epa_raw3_unpack"]) == 12 and hasattr(_lib.lib, "epa_raw3_unpack")
    assert not hasattr(ops, "raw3_unpack") and "test_poison_table_host" in raw3_unpack.__doc__
    p = __import__("ctypes").c_void_p(16)
    with pytest.raises(ValueError, match="NULL array"):
        _lib.call("epa_raw3_unpack", None, 16, 16, p, p, 1, 1, 1, 4, p, p, None)
    with pytest.raises(ValueError, match="sectors are served"):
        _lib.call("epa_raw3_unpack", p, 16, 16, p, p, 1, 1, 1, 9, p, p, None)
    with pytest.raises(ValueError, match="padded to a multiple of 16"):
        _lib.call("epa_raw3_unpack", p, 16, 24, p, p, 1, 1, 1, 4, p, p, None)


def test_vendor_group_over_two_filter_times():
    """``fm`` with the filters of one channel stamped later: ``filter_time`` is the sorted union, a channel's row is NaN at
    the time it sent nothing, shorter filters are NaN-padded to the longest (set_groups_ek80.py:1411-1518)."""
    import torch

    from echopype_amd.convert import api_ek80, parse_ek80

    specs = R.fm()
    for d in specs:
        if d["kind"] == "FIL1" and d["channel_id"] == R.CH120:
            d["ticks"] += 1000
    pl = parse_ek80.plan(R.assemble(specs)[0])
    (g,) = pl.groups
    planes = [(torch.zeros((g.C, g.P, g.S, g.B)), torch.zeros((g.C, g.P, g.S, g.B)))]
    vend = api_ek80.build_groups(pl, planes, "fm.raw")["Vendor_specific"]
    ft = vend["filter_time"].values
    assert ft.size == 2 and ft[1] > ft[0] and list(vend["channel"].values) == [R.CH70, R.CH120]
    for name, n70, n120 in (("WBT", 47, 31), ("PC", 91, 63)):
        re, deci = vend[f"{name}_coeffs_real"].values, vend[f"{name}_deci_fac"].values
        assert re.shape == (2, 2, n70) and vend[f"{name}_coeffs_real"].dims == ("channel", "filter_time", f"{name}_filter_n")
        assert np.isfinite(re[0, 0]).all() and np.isnan(re[0, 1]).all() and np.isnan(re[1, 0]).all()
        assert np.isfinite(re[1, 1, :n120]).all() and np.isnan(re[1, 1, n120:]).all()
        assert np.isnan(deci[0, 1]) and np.isnan(deci[1, 0]) and np.isfinite(deci[0, 0]) and np.isfinite(deci[1, 1])
        want = pl.fil[R.CH120, 1 if name == "WBT" else 2][0][1]
        assert np.array_equal(re[1, 1, :n120], want.real.astype(np.float64))
        assert np.array_equal(vend[f"{name}_coeffs_imag"].values[1, 1, :n120], want.imag.astype(np.float64))
