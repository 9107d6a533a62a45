"""The oracle of mask.label_regions / mask.region_statistics: ``scipy.ndimage.label`` and NumPy float64 restating the
definitions of the docstrings.  scipy numbers the regions in the raster order of their first pixel.

Every sum is ``math.fsum`` of its float64 terms (correctly rounded), and comes with the sum of the terms' absolute
values and their number, from which the tests derive the error bound of a sum taken in any order."""
import math

import numpy as np
from scipy import ndimage

NASC_FACTOR = 4 * np.pi * 1852.0 ** 2
SUMS = ("sum_sv", "sum_range", "sum_sv_range", "sum_sv_at_range", "sum_dz", "sum_sv_dz")


def structure(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(connectivity)
    return ndimage.generate_binary_structure(2, 1) if connectivity == 4 else np.ones((3, 3), dtype=bool)


def label(mask, connectivity=8):
    """-> (int32 (P, S) labels, N)"""
    mask = np.asarray(mask, dtype=bool)
    if mask.size == 0:
        return np.zeros(mask.shape, dtype=np.int32), 0
    lab, n = ndimage.label(mask, structure=structure(connectivity))
    return lab.astype(np.int32), int(n)


def delta_z(r):
    """dz[s] = r[s] - r[s-1] along the last axis, dz[0] = dz[1]; NaN with a single sample."""
    r = np.asarray(r, dtype=np.float64)
    dz = np.full(r.shape, np.nan)
    if r.shape[-1] > 1:
        dz[..., 1:] = r[..., 1:] - r[..., :-1]
        dz[..., 0] = dz[..., 1]
    return dz


def linear(sv):
    """10 ** (Sv / 10) in float64.  The quotient Sv / 10 is no float64 number: rounded to one before the power it costs up
    to |Sv / 10| ln(10) 2**-53 in the result, 11 * 2**-53 at -95 dB -- more than the kernels' whole error.  So the
    quotient and the power are taken in np.longdouble where that is wider than float64 (x86: a 64-bit significand) and
    the result is rounded to float64 once; elsewhere plain float64 has to do."""
    sv = np.asarray(sv, dtype=np.float64)
    L = np.longdouble
    with np.errstate(over="ignore"):
        if np.finfo(L).eps < 2.0 ** -60:
            return np.power(L(10), sv.astype(L) / L(10)).astype(np.float64)
        return np.power(10.0, sv / 10.0)


def _sum(terms):
    return math.fsum(terms), math.fsum(np.abs(terms)), len(terms)


def statistics(sv, rng, mask, connectivity=8, ping_time=None):
    """``sv`` (C, P, S); ``rng`` anything that broadcasts to it AFTER its dz was taken along its own last axis (so it
    must carry the sample axis); ``mask`` (P, S).  -> dict: ``region_label``, ``n_regions``, the per-region variables
    (N,), the per-(channel, region) variables (C, N) under the names of region_statistics with the range variable
    called ``range``, and ``sums[name] = (value, sum of |terms|, number of terms)``, (C, N) each."""
    sv = np.asarray(sv, dtype=np.float64)
    C, P, S = sv.shape
    lab, n = label(mask, connectivity)
    r = np.broadcast_to(np.asarray(rng, dtype=np.float64), sv.shape)
    dz = np.broadcast_to(delta_z(rng), sv.shape)
    lin = linear(sv)
    out = {"region_label": lab, "n_regions": n}
    for k in ("n_samples", "ping_first", "ping_last", "sample_first", "sample_last"):
        out[k] = np.zeros(n, dtype=np.int64)
    out["n_valid"] = np.zeros((C, n), dtype=np.int64)
    per = ("Sv_mean", "Sv_max", "range_min", "range_max", "range_mean", "center_of_mass", "height_mean", "NASC")
    for k in per:
        out[k] = np.full((C, n), np.nan)
    sums = {k: tuple(np.zeros((C, n)) for _ in range(3)) for k in SUMS}
    for k in range(n):
        idx = lab == k + 1
        pp, ss = np.nonzero(idx)
        out["n_samples"][k] = len(pp)
        out["ping_first"][k], out["ping_last"][k] = pp.min(), pp.max()
        out["sample_first"][k], out["sample_last"][k] = ss.min(), ss.max()
        n_pings = int(pp.max() - pp.min() + 1)
        for c in range(C):
            x, l_, rr, d = sv[c][idx], lin[c][idx], r[c][idx], dz[c][idx]
            xv, rv, dv = ~np.isnan(x), ~np.isnan(rr), ~np.isnan(d)
            terms = {"sum_sv": l_[xv], "sum_range": rr[rv], "sum_sv_range": (l_ * rr)[xv & rv],
                     "sum_sv_at_range": l_[xv & rv], "sum_dz": d[dv], "sum_sv_dz": (l_ * d)[xv & dv]}
            s = {}
            for name, t in terms.items():
                s[name] = _sum(t)
                for j in range(3):
                    sums[name][j][c, k] = s[name][j]
            nv, nr = int(xv.sum()), int(rv.sum())
            out["n_valid"][c, k] = nv
            with np.errstate(divide="ignore", invalid="ignore"):
                if nv:
                    out["Sv_mean"][c, k] = 10.0 * np.log10(np.float64(s["sum_sv"][0]) / nv)
                    out["Sv_max"][c, k] = x[xv].max()
                if nr:
                    out["range_min"][c, k], out["range_max"][c, k] = rr[rv].min(), rr[rv].max()
                    out["range_mean"][c, k] = s["sum_range"][0] / nr
                out["center_of_mass"][c, k] = np.float64(s["sum_sv_range"][0]) / np.float64(s["sum_sv_at_range"][0])
                out["height_mean"][c, k] = s["sum_dz"][0] / n_pings
                out["NASC"][c, k] = NASC_FACTOR * s["sum_sv_dz"][0] / n_pings
    out["n_pings"] = out["ping_last"] - out["ping_first"] + 1
    if ping_time is not None:
        ping_time = np.asarray(ping_time)
        out["ping_time_start"], out["ping_time_end"] = ping_time[out["ping_first"]], ping_time[out["ping_last"]]
    out["sums"] = sums
    return out
