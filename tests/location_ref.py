"""NumPy float64 restatement of ``utils.align.align_to_ping_time`` and ``consolidate.add_location`` -- the judge of the
GPU tests, itself held bit for bit to what the reference's own functions returned (tests/test_location_host.py against
tests/golden/ref_location_goldens.npz).

Linear mode is ``scipy.interpolate.interp1d(kind="linear", fill_value="extrapolate", assume_sorted=False)`` operation for
operation (scipy/interpolate/_interpolate.py, ``_call_linear``), on the float64 nanoseconds from the smallest external
time that xarray's ``interp`` hands to it.  Nearest mode is the rule of ``consolidate/ek_depth_utils.align_to_ping_time``:
the closer neighbour in int64 nanoseconds, the earlier one on a tie -- scipy's ``nearest`` compares float64 midpoints
``x[i] / 2 + x[i+1] / 2`` instead, which is the same thing while those are exact (tracks up to 2**52 ns = 52 days)."""
import numpy as np

NAT = np.iinfo(np.int64).min
DATAGRAM_TYPES = (None, "MRU1", "IDX")  # (the reference iterates a set: the package fixes this order)


def _ns(t):
    return np.asarray(t).astype("datetime64[ns]").astype(np.int64)


def align(t_ext, y, ping_time, method):
    """``y`` (V, N) at the times ``t_ext`` (N >= 2, any order, no NaT) on ``ping_time`` (P,) -> (V, P) float64."""
    t, pt = _ns(t_ext), _ns(ping_time)
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    order = np.argsort(t, kind="stable")
    t, y = t[order], y[:, order]
    nat = pt == NAT
    with np.errstate(over="ignore"):
        x = (t - t[0]).astype(np.float64)
        q = (pt - t[0]).astype(np.float64)
    q[nat] = np.nan  # xarray's datetime_to_numeric: NaT -> NaN
    k = np.clip(np.searchsorted(x, q, side="left"), 1, len(x) - 1)
    if method == "linear":
        with np.errstate(invalid="ignore", divide="ignore"):
            slope = (y[:, k] - y[:, k - 1]) / (x[k] - x[k - 1])
            return slope * (q - x[k - 1]) + y[:, k - 1]
    assert method == "nearest", method
    with np.errstate(over="ignore"):
        earlier = (pt - t[k - 1]) <= (t[k] - pt)
    out = y[:, np.where(earlier, k - 1, k)]
    out[:, nat] = np.nan
    return out


def align_to_ping_time(t_ext, y, ping_time, method="nearest"):
    """The four branches of utils/align.py:33-61 for one row of values -> (P,) float64."""
    t, pt = np.asarray(t_ext).astype("datetime64[ns]"), np.asarray(ping_time).astype("datetime64[ns]")
    y = np.asarray(y, dtype=np.float64)
    if t.shape == pt.shape and np.array_equal(t, pt):
        return y
    if len(t) == 1:
        return y[0] * np.ones(len(pt), dtype=np.float64)
    if len(t) == 0:
        return np.full(len(pt), np.nan)
    return align(t, y, pt, method)[0]


# ---- add_location ----------------------------------------------------------------------------------------------------------
def _invalid(lat, lon, check):
    if check == "missing":
        return lat is None or lon is None
    if lat is None or lon is None:
        return True
    if check == "all_nan":
        return bool(np.isnan(lat).all() or np.isnan(lon).all())
    if check == "some_nan":
        return bool(np.isnan(lat).any() or np.isnan(lon).any())
    return bool((lat == 0).any() or (lon == 0).any())


_MESSAGES = {
    "missing": "Coordinate variables not present.",
    "all_nan": "Coordinate variables are all NaN.",
    "some_nan": "Coordinate variables contain NaN(s). Interpolation may be negatively impacted, "
                "consider handling these values before calling ``add_location``.",
    "some_zero": "Coordinate variables contain zero(s). Interpolation may be negatively impacted, "
                 "consider handling these values before calling ``add_location``.",
}


def add_location(ping_time, platform, sonar_model, datagram_type=None, nmea_sentence=None):
    """``platform``: {variable name: (time dimension name, times, values)}, ``sentence_type`` among them.  Returns
    (latitude, longitude, [warning messages]); raises ValueError with the reference's messages."""
    ek = sonar_model.startswith("EK")
    if ek and datagram_type in ["MRU1", "IDX"]:
        lat_name, lon_name = f"latitude_{datagram_type.lower()}", f"longitude_{datagram_type.lower()}"
    elif not ek and datagram_type:
        raise ValueError("Sonar Model must be EK in order to specify datagram_type.")
    else:
        lat_name, lon_name = "latitude", "longitude"

    def values(name):
        return None if name not in platform else np.asarray(platform[name][2], dtype=np.float64)

    warnings = []
    for check in ("missing", "all_nan", "some_nan", "some_zero"):
        if not _invalid(values(lat_name), values(lon_name), check):
            continue
        msg = _MESSAGES[check]
        if ek:
            good = []
            for cand in (d for d in DATAGRAM_TYPES if d != datagram_type):
                # (the reference reads the latitude_* name for both)
                la = values("latitude" if cand is None else f"latitude_{cand.lower()}")
                lo = values("longitude" if cand is None else f"latitude_{cand.lower()}")
                pair = ("missing", "all_nan") if check in ("missing", "all_nan") else ("some_nan", "some_zero")
                if not (_invalid(la, lo, pair[0]) or _invalid(la, lo, pair[1])):
                    good.append(cand)
            if good:
                msg += f" Consider setting datagram_type to any of {good}."
        if check in ("missing", "all_nan"):
            raise ValueError(msg)
        warnings.append(msg)

    dim = platform[lon_name][0]
    out = []
    for name in (lat_name, lon_name):
        _, t, v = platform[name]
        t, v = np.asarray(t), np.asarray(v, dtype=np.float64)
        if nmea_sentence and datagram_type is None:
            keep = np.asarray(platform["sentence_type"][2]) == nmea_sentence
            t, v = t[keep], v[keep]
        elif nmea_sentence:
            raise ValueError("If datagram_type is not `None`, then `nmea_sentence` cannot be specified.")
        if len(np.unique(t)) != len(t):
            raise ValueError(f'Data contains duplicate time values in time_dim_name "{dim}". '
                             "Downstream interpolation on the position variables requires unique time values.")
        out.append(align_to_ping_time(t, v, ping_time, "linear"))
    return out[0], out[1], warnings
