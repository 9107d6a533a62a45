"""The seeded cases of the alignment / add_location tests, shared by scripts/gen_location_goldens.py (which runs the
reference on them) and the tests (which run the restatement and the package on them).  Everything is a function of the
case's name: two calls give the same arrays."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_location_goldens.npz")
T0 = np.datetime64("2026-03-01T00:00:00", "ns").astype(np.int64)
NAT = np.iinfo(np.int64).min
METHODS = ("linear", "nearest")

# name -> N fixes, P pings, V rows, then what is special about it.  ``gap_s``: mean spacing of the fixes in seconds.
ALIGN_CASES = {
    "n2_p1_v1": dict(N=2, P=1, V=1),
    "n3_v2": dict(N=3, P=17, V=2),
    "p255": dict(N=37, P=255, V=2, nan_at=(18,), zero_at=(7,)),
    "p256": dict(N=37, P=256, V=2, nan_at=(18,), zero_at=(7,)),
    "p257": dict(N=37, P=257, V=2, nan_at=(18,), zero_at=(7,)),
    "v1": dict(N=37, P=200, V=1, nan_at=(18,), zero_at=(7,)),
    "nan_first": dict(N=37, P=200, V=2, nan_at=(0,)),
    "nan_last": dict(N=37, P=200, V=2, nan_at=(36,)),
    "nan_ends_and_middle": dict(N=37, P=200, V=2, nan_at=(0, 20, 36)),
    "shuffled_track": dict(N=37, P=200, V=2, nan_at=(18,), shuffle=True),
    "pings_out_of_order": dict(N=37, P=200, V=2, unordered=True),
    "days200": dict(N=37, P=200, V=2, gap_s=200 * 86400 / 36, nan_at=(18,)),  # 1.7e16 ns > 2**53
    "midway": dict(N=37, P=200, V=2, midway=True),
    "nat_ping": dict(N=37, P=200, V=2, nat_at=(0, 77, 199), nan_at=(18,)),
}
# a NaT ping: the reference over oracle/xr_shim.py turns it into -9.2e18 ns where real xarray makes it NaN, so the
# reference-executed goldens hold no such case; the restatement pins NaT -> NaN
NOT_IN_GOLDENS = ("nat_ping",)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def track(rng, N, gap_s=1.0):
    """N strictly increasing int64-ns times from T0 (even gaps, so that a midpoint is a whole nanosecond) and a
    (2, N) latitude / longitude walk."""
    gaps = 2 * rng.integers(int(0.25e9 * gap_s), int(0.75e9 * gap_s), N - 1, dtype=np.int64)
    t = T0 + np.concatenate([[0], np.cumsum(gaps)])
    lat = 45.0 + np.cumsum(rng.normal(0, 1e-4, N))
    lon = -125.0 + np.cumsum(rng.normal(0, 1e-4, N))
    return t, np.stack([lat, lon])


def align_case(name):
    """-> dict(t_ext datetime64[ns] (N,), y float64 (V, N), ping_time datetime64[ns] (P,))."""
    c = ALIGN_CASES[name]
    rng = _rng(name)
    N, P, V = c["N"], c["P"], c["V"]
    t, y = track(rng, N, c.get("gap_s", 1.0))
    y = y[:V].copy()
    for i in c.get("nan_at", ()):
        y[:, i] = np.nan
    for i in c.get("zero_at", ()):
        y[0, i] = 0.0
    span = int(t[-1] - t[0])
    pt = np.sort(t[0] - span // 20 + rng.integers(0, span + span // 10, P, dtype=np.int64))
    if P >= 8:
        # before the first and after the last fix, and exactly on the first, an inner and the last fix
        pt[0], pt[-1] = t[0] - span // 7, t[-1] + span // 9
        pt[1:4] = np.sort([t[0], t[N // 3], t[-1]])
        if c.get("midway"):
            pt[4:6] = [(t[5] + t[6]) // 2, (t[N - 3] + t[N - 2]) // 2]
        pt = np.sort(pt)
    else:
        pt[:] = t[0] + rng.integers(1, span, P, dtype=np.int64)
    if c.get("unordered"):
        pt = pt[rng.permutation(P)]
    for i in c.get("nat_at", ()):
        pt[i] = NAT
    if c.get("shuffle"):
        perm = rng.permutation(N)
        t, y = t[perm], y[:, perm]
    return {"t_ext": t.astype("datetime64[ns]"), "y": np.ascontiguousarray(y), "ping_time": pt.astype("datetime64[ns]")}


# ---- add_location: Platform groups ----------------------------------------------------------------------------------------
# name -> sonar model, call arguments and what the Platform group holds
LOCATION_CASES = {
    "plain": dict(model="EK60", vars=("nmea",)),
    "some_nan_and_zero": dict(model="EK60", vars=("nmea",), nan_at=(11,), zero_at=(3,)),
    # longitude_idx holds a zero and IDX is recommended all the same: the reference looks at latitude_idx twice
    "some_nan_suggests_idx": dict(model="EK80", vars=("nmea", "idx"), nan_at=(11,), idx_zero_at=(2,)),
    "gga": dict(model="EK60", vars=("nmea",), nmea_sentence="GGA"),
    "mru1": dict(model="EK80", vars=("nmea", "mru1"), datagram_type="MRU1"),
    "idx": dict(model="EK80", vars=("idx",), datagram_type="IDX"),
    "azfp": dict(model="AZFP", vars=("nmea",)),
    "single_fix": dict(model="EK60", vars=("nmea",), N=1),
    "track_on_ping_time": dict(model="EK60", vars=("nmea",), on_ping_time=True),
    "missing_azfp": dict(model="AZFP", vars=()),
    "missing_ek_suggests_mru1": dict(model="EK80", vars=("mru1",)),
    "missing_mru1_suggests_nmea_idx": dict(model="EK80", vars=("nmea", "idx"), datagram_type="MRU1"),
    "all_nan": dict(model="EK60", vars=("nmea",), all_nan=True),
    "all_nan_suggests_idx": dict(model="EK80", vars=("nmea", "idx"), all_nan=True),
    "datagram_type_on_azfp": dict(model="AZFP", vars=("nmea",), datagram_type="MRU1"),
    "sentence_with_datagram_type": dict(model="EK80", vars=("nmea", "mru1"), datagram_type="MRU1", nmea_sentence="GGA"),
    "duplicate_times": dict(model="EK60", vars=("nmea",), duplicate=True),
    "duplicates_outside_the_sentence": dict(model="EK60", vars=("nmea",), duplicate=True, nmea_sentence="RMC"),
}
# two recommendations: the reference lists them in the order of a set of strings, which changes from process to process.
# The generator checks the message up to that order and stores nothing; the package's order is the restatement's.
ORDER_UNDEFINED = ("missing_mru1_suggests_nmea_idx",)
LOC_P, LOC_N = 300, 41
_TIME_DIM = {"nmea": "time1", "mru1": "time3", "idx": "time4"}
_SUFFIX = {"nmea": "", "mru1": "_mru1", "idx": "_idx"}


def location_case(name):
    """-> dict(model, datagram_type, nmea_sentence, ping_time datetime64[ns] (P,),
    platform {variable: (time dimension, times datetime64[ns], values)})."""
    c = LOCATION_CASES[name]
    rng = _rng("loc/" + name)
    N = c.get("N", LOC_N)
    t_nav, _ = track(rng, max(N, 2))
    span = int(t_nav[-1] - t_nav[0]) if N > 1 else 40_000_000_000
    pt = np.sort(t_nav[0] - span // 20 + rng.integers(0, span + span // 10, LOC_P, dtype=np.int64))
    platform = {}
    for kind in c["vars"]:
        n = LOC_P if c.get("on_ping_time") else N
        t, y = track(rng, max(n, 2))
        t, y = t[:n], y[:, :n].copy()
        if c.get("on_ping_time"):
            t = pt.copy()
        if kind == "nmea":
            for i in c.get("nan_at", ()):
                y[1, i] = np.nan
            for i in c.get("zero_at", ()):
                y[0, i] = 0.0
            if c.get("all_nan"):
                y[0, :] = np.nan
            if c.get("duplicate"):
                t[9] = t[8]  # fix 8 is "GGA", fix 9 "RMC": neither sentence's subset holds both
        if kind == "idx":
            for i in c.get("idx_zero_at", ()):
                y[1, i] = 0.0
        dim = _TIME_DIM[kind]
        platform[f"latitude{_SUFFIX[kind]}"] = (dim, t.astype("datetime64[ns]"), y[0])
        platform[f"longitude{_SUFFIX[kind]}"] = (dim, t.astype("datetime64[ns]"), y[1])
        if kind == "nmea":
            i = np.arange(n)
            platform["sentence_type"] = (dim, t.astype("datetime64[ns]"), np.array(["GGA", "RMC", "GLL"])[i % 2 + (i % 7 == 6)])
    return {"model": c["model"], "datagram_type": c.get("datagram_type"), "nmea_sentence": c.get("nmea_sentence"),
            "ping_time": pt.astype("datetime64[ns]"), "platform": platform}


def load_fixture():
    """(records of the align cases, records of the add_location cases, the npz) of the reference-executed goldens."""
    z = np.load(GOLDEN)
    return json.loads(z["align_cases"].item()), json.loads(z["location_cases"].item()), z
