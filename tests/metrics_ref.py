"""NumPy float64 oracle of the echo summary statistics (metrics/summary_statistics.py of the reference, restated).

A dataset here is a dict {name: array}; the LAST axis of every array is ``range_sample``; a range variable has the shape
of ``Sv`` or is 1-D (one row shared by all).  For every row and for samples j = 1 .. S-1, with r = ds[range_label]:

    dz_j = r_j - r_{j-1}  in r's own dtype (np.diff), a zero -> NaN      sv_j = 10 ** (Sv_j / 10)      w_j = sv_j dz_j
    A = sum w_j     B = sum r_j w_j     Q = sum sv_j**2 dz_j     I = sum (r_j - cm)**2 w_j

each sum skipping its NaN terms (an all-NaN row sums to 0), everything after dz in float64 on the values handed in
(float32 inputs upcast; anything but float32 / float64 is converted to float64 first, as the package does).

    abundance = 10 log10 A    center_of_mass = B / A    dispersion = I / A    evenness = A**2 / Q    aggregation = 1 / evenness

``dispersion`` takes cm from ``echo_range`` whatever ``range_label`` names (the reference's call ``center_of_mass(ds)``).
``sums`` also returns sum |term| of every sum: what the float32 bounds (tests/metrics_bounds.py) are made of."""
import numpy as np

NAMES = ("abundance", "center_of_mass", "dispersion", "evenness", "aggregation")


def _floating(a):
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def _pair(ds, range_label):
    if range_label not in ds:
        raise ValueError(f"{range_label} not in the input Dataset!")
    sv, r = _floating(ds["Sv"]), _floating(ds[range_label])
    if sv.dtype != r.dtype:
        sv, r = sv.astype(np.float64), r.astype(np.float64)
    return sv, r


def sums(sv, r, cm=None):
    """The four sums of every row, their sum |term|, and the cm that I is about (``cm``: given centres, else B / A)."""
    sv, r = np.asarray(sv), np.asarray(r)
    rb = np.broadcast_to(r, sv.shape)
    with np.errstate(all="ignore"):
        dz = np.diff(rb, axis=-1)  # in the dtype of the range
        dz = np.where(dz != 0, dz, np.nan).astype(np.float64)
        rj = rb[..., 1:].astype(np.float64)
        lin = 10.0 ** (sv[..., 1:].astype(np.float64) / 10)
        w = lin * dz
        tA, tB, tQ = w, rj * w, lin * lin * dz
        A, B, Q = (np.nansum(t, axis=-1) for t in (tA, tB, tQ))
        c = B / A if cm is None else np.asarray(cm, np.float64)
        d = rj - c[..., None]
        tI = d * d * w
        out = {"A": A, "B": B, "Q": Q, "I": np.nansum(tI, axis=-1), "cm": c, "n": sv.shape[-1],
               "svmax": _absmax_finite(sv[..., 1:])}
        for k, t in (("A", tA), ("B", tB), ("Q", tQ), ("I", tI)):
            out["abs" + k] = np.nansum(np.abs(t), axis=-1)
    return out


def _absmax_finite(a):
    a = np.abs(np.asarray(a, np.float64))
    a = np.where(np.isfinite(a), a, 0.0)
    return a.max(axis=-1) if a.shape[-1] else np.zeros(a.shape[:-1])


def statistics(s):
    """The five statistics from ``sums``'s result."""
    with np.errstate(all="ignore"):
        even = s["A"] ** 2 / s["Q"]
        return {"abundance": 10 * np.log10(s["A"]), "center_of_mass": s["B"] / s["A"], "dispersion": s["I"] / s["A"],
                "evenness": even, "aggregation": 1 / even}


def rows(sv, r, cm=None):
    """(statistics, sums) of the rows of ``sv`` with the range ``r`` -- what one call of the kernel returns."""
    s = sums(sv, r, cm)
    return statistics(s), s


def dispersion_floor(cm):
    """What a relative comparison of two float64 dispersions needs besides its rtol: cm = B / A carries a few roundings
    (the products, the sums, the quotient: within 8 ulp), and by I(c) = I(cm) + (c - cm)^2 A the dispersion sees that
    squared.  A row whose mass sits in ONE sample has dispersion 0 exactly; evaluated, it is this noise (1e-30 m^2 at
    30 m), in the reference as in the oracle, and no two evaluations agree on it to any rtol."""
    with np.errstate(all="ignore"):
        c = np.abs(np.asarray(cm, np.float64))
        return np.where(np.isfinite(c), (8 * np.spacing(c)) ** 2, 0.0)


# ---- the seven names --------------------------------------------------------------------------------------------------
def delta_z(ds, range_label="echo_range"):
    if range_label not in ds:
        raise ValueError(f"{range_label} not in the input Dataset!")
    r = np.asarray(ds[range_label])
    dz = np.diff(r, axis=-1)
    return np.where(dz != 0, dz, np.nan)


def convert_to_linear(ds, Sv_label="Sv"):
    return 10 ** (np.asarray(ds[Sv_label]) / 10)


def abundance(ds, range_label="echo_range"):
    return rows(*_pair(ds, range_label))[0]["abundance"]


def center_of_mass(ds, range_label="echo_range"):
    return rows(*_pair(ds, range_label))[0]["center_of_mass"]


def dispersion(ds, range_label="echo_range"):
    sv, r = _pair(ds, range_label)
    return rows(sv, r, cm=center_of_mass(ds))[0]["dispersion"]


def evenness(ds, range_label="echo_range"):
    return rows(*_pair(ds, range_label))[0]["evenness"]


def aggregation(ds, range_label="echo_range"):
    return 1 / evenness(ds, range_label=range_label)


FUNCS = {"abundance": abundance, "center_of_mass": center_of_mass, "dispersion": dispersion, "evenness": evenness,
         "aggregation": aggregation}
