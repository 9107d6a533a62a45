"""``utils.align_to_ping_time`` and ``consolidate.add_location`` without a GPU: the NumPy restatement
(tests/location_ref.py) against what the reference's own functions returned (tests/golden/ref_location_goldens.npz,
scripts/gen_location_goldens.py), the drop-in signatures, every message the reference raised or logged reproduced by the
package on paths that reach no device work, and the argument errors of ``epa_align_to_ping_time``."""
import inspect
import json
import logging
import os

import numpy as np
import pytest

import location_cases as C
import location_ref as R
from test_signatures import ALLOWED_EXTRAS, KIND, _same_default

ALIGN, LOCATION, Z = C.load_fixture()
SIGS = json.load(open(os.path.join(os.path.dirname(C.GOLDEN), "ref_location_signatures.json")))
BY_NAME = {r["name"]: r for r in LOCATION}


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.int64) == want.view(np.int64)
    same |= np.isnan(got) & np.isnan(want)  # (a NaN is a NaN: its payload is not part of the result)
    assert same.all(), (what, int((~same).sum()), got[~same][:4], want[~same][:4])


# ---- the restatement against the reference ------------------------------------------------------------------------------
def test_the_cases_are_the_ones_the_reference_ran():
    assert [r["name"] for r in ALIGN] == [n for n in C.ALIGN_CASES if n not in C.NOT_IN_GOLDENS]
    assert [r["name"] for r in LOCATION] == [n for n in C.LOCATION_CASES if n not in C.ORDER_UNDEFINED]
    for name in (r["name"] for r in ALIGN):
        for k, a in C.align_case(name).items():
            np.testing.assert_array_equal(a, Z[f"align/{name}/in/{k}"], err_msg=f"{name} {k}")


@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("name", [r["name"] for r in ALIGN])
def test_restatement_equals_the_reference_bit_for_bit(name, method):
    c = {k: Z[f"align/{name}/in/{k}"] for k in ("t_ext", "y", "ping_time")}
    want = Z[f"align/{name}/{method}"]
    assert_bits(R.align(c["t_ext"], c["y"], c["ping_time"], method), want, f"{name} {method}")
    for v in range(c["y"].shape[0]):  # through the four branches, one row at a time as the reference takes them
        assert_bits(R.align_to_ping_time(c["t_ext"], c["y"][v], c["ping_time"], method), want[v], f"{name} {method} row {v}")


def test_the_goldens_hold_what_the_cases_are_about():
    lin = Z["align/p257/linear"]
    pt, t = Z["align/p257/in/ping_time"].astype(np.int64), Z["align/p257/in/t_ext"].astype(np.int64)
    y = Z["align/p257/in/y"]
    assert pt.min() < t.min() and pt.max() > t.max()  # both end segments extrapolate
    for fix in (0, 37 // 3, 36):  # a ping on a fix returns the fix
        hit = np.flatnonzero(pt == t[fix])
        assert hit.size == 1 and lin[0, hit[0]] == y[0, fix]
    nan = np.isnan(lin[0])
    assert nan.any() and (nan == ((pt > t[17]) & (pt <= t[19]))).all()  # the NaN fix spoils its two segments, no more
    assert (t[-1] - t[0]) < 2**53 < np.ptp(Z["align/days200/in/t_ext"].astype(np.int64))
    mid_pt, mid_t = Z["align/midway/in/ping_time"].astype(np.int64), Z["align/midway/in/t_ext"].astype(np.int64)
    at = np.flatnonzero(mid_pt == (mid_t[5] + mid_t[6]) // 2)
    assert at.size == 1 and Z["align/midway/nearest"][0, at[0]] == Z["align/midway/in/y"][0, 5]  # a tie: the earlier fix


def test_restatement_turns_a_nat_ping_into_nan():
    c = C.align_case("nat_ping")
    nat = np.isnat(c["ping_time"])
    assert nat.sum() == 3
    for method in C.METHODS:
        out = R.align(c["t_ext"], c["y"], c["ping_time"], method)
        assert np.isnan(out[:, nat]).all()
        keep = ~nat
        assert_bits(out[:, keep], R.align(c["t_ext"], c["y"], c["ping_time"][keep], method), method)


def _restated(name):
    c = C.location_case(name)
    return R.add_location(c["ping_time"], c["platform"], c["model"], c["datagram_type"], c["nmea_sentence"])


@pytest.mark.parametrize("name", list(C.LOCATION_CASES))
def test_restated_add_location_equals_the_reference(name):
    if name in C.ORDER_UNDEFINED:  # (the generator compared the message up to the order of its list)
        with pytest.raises(ValueError, match=r"any of \[None, 'IDX'\]\.$"):
            _restated(name)
        return
    rec = BY_NAME[name]
    if "raised" in rec:
        with pytest.raises(ValueError) as e:
            _restated(name)
        assert [type(e.value).__name__, str(e.value)] == rec["raised"]
        return
    lat, lon, warnings = _restated(name)
    assert warnings == [m for _, m in rec["logged"]]
    assert_bits(lat, Z[f"location/{name}/latitude"], f"{name} latitude")
    assert_bits(lon, Z[f"location/{name}/longitude"], f"{name} longitude")


# ---- the package: signatures and messages (no device work is reached) --------------------------------------------------------
@pytest.mark.parametrize("qual", sorted(SIGS))
def test_signature_equals_the_reference(qual):
    import echopype_amd as ep

    mod, name = qual.split(".")
    fn = getattr(getattr(ep, mod), name)
    got = [(p.name, KIND[p.kind], p.default) for p in inspect.signature(fn).parameters.values()]
    ref = SIGS[qual]["params"]
    core = [g for g in got if not (g[0] in ALLOWED_EXTRAS or g[0].startswith("_"))]
    extras = [g for g in got if g[0] in ALLOWED_EXTRAS or g[0].startswith("_")]
    assert [g[0] for g in core] == [r[0] for r in ref], f"{qual}: parameter names / order"
    for (n, kind, default), (rn, rkind, rsrc) in zip(core, ref):
        assert kind == rkind, f"{qual}: {n} is {kind}, the reference's is {rkind}"
        assert _same_default(default, rsrc), f"{qual}: default of {n} is {default!r}, the reference's is {rsrc}"
    for n, kind, default in extras:
        assert kind == "keyword_only" and default is not inspect.Parameter.empty, f"{qual}: extra parameter {n}"


def test_the_names_are_exported():
    import echopype_amd as ep

    assert "add_location" in ep.consolidate.__all__
    assert ep.utils.align_to_ping_time is ep.utils.align.align_to_ping_time
    from echopype_amd.consolidate import loc_utils

    assert sorted(loc_utils.__all__) == ["check_loc_time_dim_duplicates", "check_loc_vars_validity",
                                         "compute_invalid_check", "sel_nmea"]


def echodata_of(case):
    """The case's Platform group in an ``EchoData`` (item assignment: the container takes a Platform group as it is)."""
    import echopype_amd as ep

    plat = ep.Dataset()
    for name, (dim, t, v) in case["platform"].items():
        plat[name] = ep.DataArray(v, (dim,), {dim: t}, {"long_name": name}, name)
    ed = ep.EchoData(case["model"])
    ed["Platform"] = plat
    return ed


def dataset_of(case, S=2):
    import echopype_amd as ep

    ds = ep.Dataset(coords={"ping_time": case["ping_time"], "range_sample": np.arange(S)})
    ds["Sv"] = (("ping_time", "range_sample"), np.zeros((len(case["ping_time"]), S)))
    return ds


class _NoDevice:
    """Any attribute of ``ops`` that would touch the device fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"ops.{name} reached on a path that must not touch the device")


@pytest.mark.parametrize("name", [n for n in C.LOCATION_CASES if n in C.ORDER_UNDEFINED or "raised" in BY_NAME[n]])
def test_package_raises_the_reference_message(name, monkeypatch):
    import echopype_amd as ep

    monkeypatch.setattr(ep.utils.align, "ops", _NoDevice())
    c = C.location_case(name)
    with pytest.raises(ValueError) as want:
        _restated(name)
    if name not in C.ORDER_UNDEFINED:
        assert [type(want.value).__name__, str(want.value)] == BY_NAME[name]["raised"]
    with pytest.raises(ValueError) as got:
        ep.consolidate.add_location(dataset_of(c), echodata_of(c), datagram_type=c["datagram_type"],
                                    nmea_sentence=c["nmea_sentence"])
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("name", [r["name"] for r in LOCATION if r.get("logged")])
def test_package_logs_the_reference_warnings(name, monkeypatch, caplog):
    """The warnings come before the alignment: it is cut short here (no device on this machine), after they were logged."""
    import echopype_amd as ep
    from echopype_amd.consolidate import api

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached

    monkeypatch.setattr(api, "align_many_to_ping_time", stop)
    c = C.location_case(name)
    with caplog.at_level(logging.WARNING, logger="echopype_amd.consolidate"), pytest.raises(Reached):
        ep.consolidate.add_location(dataset_of(c), echodata_of(c), c["datagram_type"], c["nmea_sentence"])
    got = [[r.levelname, r.getMessage()] for r in caplog.records if r.name == "echopype_amd.consolidate"]
    assert got == BY_NAME[name]["logged"]


@pytest.mark.parametrize("name", ["single_fix", "track_on_ping_time"])
def test_branches_without_a_launch_equal_the_reference(name, monkeypatch):
    """One fix is repeated and a track on ``ping_time`` passes through: host work only, compared with the reference."""
    import echopype_amd as ep

    monkeypatch.setattr(ep.utils.align, "ops", _NoDevice())
    c = C.location_case(name)
    ds = dataset_of(c)
    out = ep.consolidate.add_location(ds, echodata_of(c))
    assert "latitude" not in ds and "time1" not in out
    assert out.attrs["processing_level"] == "Level 2A" and "processing_level" not in ds.attrs  # Sv with valid positions
    for v in ("latitude", "longitude"):
        assert out[v].dims == ("ping_time",) and out[v].dtype == np.float64
        assert_bits(out[v].values, Z[f"location/{name}/{v}"], f"{name} {v}")
        stamp, _, rest = out[v].attrs["history"].partition(". ")
        assert rest == BY_NAME[name]["history"] and sorted(out[v].attrs) == BY_NAME[name]["attrs"]


def test_align_to_ping_time_host_branches_and_errors(monkeypatch):
    import echopype_amd as ep

    monkeypatch.setattr(ep.utils.align, "ops", _NoDevice())
    pt = C.align_case("p255")["ping_time"]
    ping = ep.DataArray(pt, ("ping_time",), {"ping_time": pt})
    attrs = {"units": "m"}

    def ext(t, v):
        return ep.DataArray(np.asarray(v, dtype=np.float32), ("time3",), {"time3": np.asarray(t, "datetime64[ns]")}, attrs, "x")

    same = ep.utils.align_to_ping_time(ext(pt, np.arange(len(pt))), "time3", ping)
    assert same.dims == ("ping_time",) and same.dtype == np.float32 and "time3" not in same.coords and same.attrs == attrs
    np.testing.assert_array_equal(same.values, np.arange(len(pt), dtype=np.float32))
    one = ep.utils.align_to_ping_time(ext(pt[:1], [2.5]), "time3", ping, method="linear")
    assert one.dtype == np.float64 and (one.values == 2.5).all() and one.shape == pt.shape and one.attrs == attrs
    none = ep.utils.align_to_ping_time(ext(pt[:0], []), "time3", ping)
    assert none.dtype == np.float64 and np.isnan(none.values).all() and none.shape == pt.shape
    with pytest.raises(ValueError, match="'linear' or 'nearest'"):
        ep.utils.align_to_ping_time(ext(pt[:3], [1, 2, 3]), "time3", ping, method="cubic")
    with pytest.raises(ValueError, match="NaT"):
        ep.utils.align_to_ping_time(ext([pt[0], np.datetime64("NaT"), pt[2]], [1, 2, 3]), "time3", ping)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_abi_reports_each_argument_error_without_a_gpu():
    from echopype_amd import _lib

    ok = dict(t=8, N=2, y=8, V=1, pt=8, P=1, mode=0, out=8)  # (never launched: every call below fails a check first)

    def call(**kw):
        a = {**ok, **kw}
        _lib.call("epa_align_to_ping_time", a["t"], a["N"], a["y"], a["V"], a["pt"], a["P"], a["mode"], a["out"], None)

    for kw, msg in (({"N": 1}, "N=1 external times"), ({"N": 0}, "N=0"), ({"V": 0}, "V=0 rows"), ({"P": 0}, "P=0 pings"),
                    ({"P": -3}, "P=-3"), ({"t": None}, "NULL array"), ({"y": None}, "NULL array"),
                    ({"pt": None}, "NULL array"), ({"out": None}, "NULL array"), ({"mode": 2}, "bad mode 2"),
                    ({"mode": -1}, "bad mode -1")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
