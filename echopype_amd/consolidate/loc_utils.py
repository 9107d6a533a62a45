"""What ``add_location`` asks of the Platform group's position variables before it interpolates them: are they there,
do they hold anything, do they hold NaNs or zeros, are their times unique -- and the choice of the fixes of one NMEA
sentence type.  Behaviour and messages are those of echopype's consolidate/loc_utils.py (the tests hold every message to
what the reference raised or logged).  Host work on the navigation track: a few thousand fixes."""
import logging

import numpy as np

from ..xr_lite import DataArray

logger = logging.getLogger("echopype_amd.consolidate")

_ADVICE = ("Interpolation may be negatively impacted, "
           "consider handling these values before calling ``add_location``.")
# check -> (what is said, does it stop the call?)
_CHECKS = {
    "missing": ("Coordinate variables not present.", True),
    "all_nan": ("Coordinate variables are all NaN.", True),
    "some_nan": ("Coordinate variables contain NaN(s). " + _ADVICE, False),
    "some_zero": ("Coordinate variables contain zero(s). " + _ADVICE, False),
}
# what a pair of host arrays is tested for, per check
_TESTS = {
    "all_nan": lambda a: np.isnan(a).all(),
    "some_nan": lambda a: np.isnan(a).any(),
    "some_zero": lambda a: (a == 0).any(),
}
# the datagram types a user can be pointed to, in the order they are listed (None: the NMEA positions)
_DATAGRAM_TYPES = (None, "MRU1", "IDX")


def loc_names(sonar_model, datagram_type):
    """(latitude name, longitude name) in the Platform group: the plain names unless an EK file is asked for the
    positions of its MRU1 / IDX datagrams.  A datagram type on any other sonar model is refused."""
    ek = sonar_model.startswith("EK")
    if datagram_type and not ek:
        raise ValueError("Sonar Model must be EK in order to specify datagram_type.")
    suffix = f"_{datagram_type.lower()}" if ek and datagram_type in ("MRU1", "IDX") else ""
    return "latitude" + suffix, "longitude" + suffix


def compute_invalid_check(lat_var, lon_var, validity_check):
    """True when the pair of position variables fails ``validity_check`` ("missing", "all_nan", "some_nan" or
    "some_zero": either variable failing is enough).  A missing variable fails every check; so does an unknown check."""
    absent = lat_var is None or lon_var is None
    if validity_check == "missing" or absent or validity_check not in _TESTS:
        return absent or validity_check not in _CHECKS
    test = _TESTS[validity_check]
    return bool(test(np.asarray(lat_var.values)) or test(np.asarray(lon_var.values)))


def _usable_instead(platform, datagram_type, validity_check):
    """The other datagram types whose variables would pass: present and not all NaN when the complaint is about
    missing / all-NaN variables, free of NaNs and zeros when it is about those.  The reference looks the LATITUDE
    variable of a datagram type up twice (its longitude is never looked at); so does this."""
    family = ("missing", "all_nan") if _CHECKS[validity_check][1] else ("some_nan", "some_zero")
    good = []
    for cand in _DATAGRAM_TYPES:
        if cand == datagram_type:
            continue
        if cand is None:
            pair = platform.get("latitude"), platform.get("longitude")
        else:
            pair = (platform.get(f"latitude_{cand.lower()}"),) * 2
        if not any(compute_invalid_check(*pair, check) for check in family):
            good.append(cand)
    return good


def check_loc_vars_validity(echodata, lat_name, lon_name, datagram_type, validity_check):
    """One of the four checks on ``echodata["Platform"][lat_name / lon_name]``: "missing" and "all_nan" raise
    ``ValueError``, "some_nan" and "some_zero" log a warning.  For EK models the message ends with the datagram types
    that could be used instead, when there are any."""
    platform = echodata["Platform"]
    if not compute_invalid_check(platform.get(lat_name), platform.get(lon_name), validity_check):
        return
    message, fatal = _CHECKS[validity_check]
    if echodata.sonar_model.startswith("EK"):
        good = _usable_instead(platform, datagram_type, validity_check)
        if good:
            message += f" Consider setting datagram_type to any of {good}."
    if fatal:
        raise ValueError(message)
    logger.warning(message)


def check_loc_time_dim_duplicates(da, time_dim_name):
    """Interpolation needs one value per time: a time that occurs twice in ``da``'s coordinate raises."""
    times = np.asarray(da.coords[time_dim_name])
    if np.unique(times).size != times.size:
        raise ValueError(f'Data contains duplicate time values in time_dim_name "{time_dim_name}". '
                         "Downstream interpolation on the position variables requires unique time values.")


def sel_nmea(echodata, loc_name, nmea_sentence=None, datagram_type=None):
    """``echodata["Platform"][loc_name]``, cut down to the fixes whose ``sentence_type`` is ``nmea_sentence`` when one is
    given.  Sentence types belong to the NMEA positions (``datagram_type`` None): with another datagram type a
    sentence is refused."""
    platform = echodata["Platform"]
    if nmea_sentence and datagram_type is not None:
        raise ValueError("If datagram_type is not `None`, then `nmea_sentence` cannot be specified.")
    da = platform[loc_name]
    if not nmea_sentence:
        return da
    keep = np.asarray(platform["sentence_type"].values) == nmea_sentence
    dim = da.dims[0]
    coords = {dim: np.asarray(da.coords[dim])[keep]} if dim in da.coords else {}
    return DataArray(np.asarray(da.values)[keep], da.dims, coords, da.attrs, da.name)


__all__ = ["compute_invalid_check", "check_loc_vars_validity", "check_loc_time_dim_duplicates", "sel_nmea"]
