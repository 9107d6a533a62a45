"""Per-row bounds of the float32 route of ``epa_echo_metrics`` (csrc/metrics.hip) against the float64 oracle
(tests/metrics_ref.py), derived from the kernel's operation sequence on top of tests/f32_bounds.py.  Nothing is fitted.

What the float32 route does per sample (``mt_group``): ``lin = exp10f(v * 0.1f)`` in float32 -- relative error
e1 = ``exp10_rel(|v|)``, the only float32 rounding there is; ``dz = r_j - r_{j-1}`` is ONE float32 subtraction, the very
number the oracle takes (np.diff in the input dtype), and r is read as it is.  From there on everything is double:
w = lin dz, the terms r w, lin lin dz, (r - cm)^2 w, the sums (a tree over lanes, a fixed order), the quotients and the
logarithm; each result is rounded to float32 once.  So, with n = S samples and sum|t| the oracle's sum of |term|:

    |dA| <= (e1 + eps64) sum|w|          |dB| <= (e1 + eps64) sum|r w|          |dQ| <= (2 e1 + e1^2 + eps64) sum|lin^2 dz|

where eps64 = 2 (n + 8) 2^-53 covers the double products and the double sums of both sides (any order: (n-1) u each).
The bounds hold for linear values in float32's normal range: |Sv| <= 370 dB is required of the finite samples.

    abundance        db_of_rel(dA / |A|)                                      + 1/2 ulp32
    center_of_mass   dcm = (dB + |cm| dA) / (|A| - dA)                        + 1/2 ulp32
    evenness         |E| ((1 + a)^2 / (1 - q) - 1),  a = dA/|A|, q = dQ/|Q|  + 1/2 ulp32
    aggregation      |G| ((1 + q) / (1 - a)^2 - 1)                            + 1/2 ulp32
    dispersion       (dI + |D| dA) / (|A| - dA)                               + 1/2 ulp32

For dI the identity I(c) = I(cm) + (c - cm)^2 A, which holds for any weights about their own centre cm, turns the error
of the centre into a second-order term: the kernel's I'(c') is taken with its perturbed weights w' about its own
c' = B'/A' (their centre up to 2^-52), so I'(c') - I'(cm) = -(cm - c')^2 A' and
    |dI| <= (e1 + eps64) sum|(r - cm)^2 w| + dcm^2 (|A| + dA).
With the centres handed in (``cm_in``) the second term is absent when both sides use the same numbers; where the
oracle's centres differ from the ones the judged side used by at most ``centre_err``, I is off by at most
2 |B - c A| centre_err + centre_err^2 |A| more (dI/dc = -2 (B - c A): first order, c is not this range's centre).

``reference_f32_slack`` is the same propagation for the reference's OWN float32 evaluation (the fixture's float32 results):
per term ``10 ** (Sv / 10)`` in float32 (the quotient rounds once, powf at 2 ulp), k float32 roundings of the products
(A: 1, B: 2, Q: 3 with the square, I: 6 with the difference and its square), and a float32 sum of n terms, gamma(n) of
sum|term| in any order; its final float32 operations (log10 and a product, a quotient, a square and a quotient, one more
reciprocal) are at most 4 half-ulps of the result."""
import numpy as np

import f32_bounds as F
from f32_bounds import U, U64, db_of_rel, exp10_rel, gamma, half_ulp  # noqa: F401

SV_ABS_MAX = 370.0


def _propagate(st, s, eA, eB, eQ, eI, given_cm, half_ulps, centre_err=0.0):
    with np.errstate(all="ignore"):
        A, absA = np.abs(s["A"]), s["absA"]
        dA, dB, dQ = eA * absA, eB * s["absB"], eQ * s["absQ"]
        a, q = dA / A, dQ / np.abs(s["Q"])
        ok = a < 1.0
        den = np.where(ok, A - dA, np.nan)
        dcm = (dB + np.abs(st["center_of_mass"]) * dA) / den
        # (the reference rounds its centre to float32 before it takes I about it: half an ulp more, squared as well)
        dc = dcm + (half_ulp(st["center_of_mass"]) if half_ulps > 1 else 0.0)
        if given_cm:  # I(c) is linear in c to first order: dI/dc = -2 (B - c A)
            dc = np.asarray(centre_err, np.float64)
            first = 2 * np.abs(s["B"] - s["cm"] * s["A"]) * dc + dc ** 2 * (A + dA)
            dI = eI * s["absI"] + np.where(dc > 0, first, 0.0)  # (the same centres on both sides, NaN or inf ones too)
        else:
            dI = eI * s["absI"] + dc ** 2 * (A + dA)
        out = {
            "abundance": db_of_rel(a),
            "center_of_mass": dcm,
            "dispersion": (dI + np.abs(st["dispersion"]) * dA) / den,
            "evenness": np.abs(st["evenness"]) * np.where(q < 1.0, (1 + a) ** 2 / (1 - q) - 1, np.inf),
            "aggregation": np.abs(st["aggregation"]) * np.where(ok, (1 + q) / (1 - a) ** 2 - 1, np.inf),
        }
        for k in out:
            b = np.where(np.isfinite(out[k]), out[k], np.inf)
            out[k] = np.where(np.isfinite(st[k]), b + half_ulps * half_ulp(st[k]), b)
    return out


def _checked_svmax(s):
    assert np.all(s["svmax"] <= SV_ABS_MAX), "the bounds need the linear values in float32's normal range"
    return s["svmax"]


def kernel_bounds(st, s, given_cm=False, centre_err=0.0):
    """{name: per-row absolute bound} of the float32 kernel's results against the oracle's (``st``, ``s`` =
    ``metrics_ref.rows(...)`` on the float32 values the kernel read)."""
    e1 = exp10_rel(_checked_svmax(s))
    eps = 2 * (s["n"] + 8) * U64
    return _propagate(st, s, e1 + eps, e1 + eps, 2 * e1 + e1 * e1 + eps, e1 + eps, given_cm, 1, centre_err)


def reference_f32_slack(st, s, given_cm=False, centre_err=0.0):
    """{name: per-row absolute bound} of the reference's own float32 evaluation against the oracle."""
    sv = _checked_svmax(s)
    p = np.expm1(F.LN10 * sv / 10.0 * U) * (1 + 4 * U) + 4 * U  # fl32(Sv / 10), powf at 2 ulp
    g = gamma(s["n"])
    e = {k: ((1 + p) ** m * (1 + U) ** n_ops - 1) + g * (1 + p) ** m * (1 + U) ** n_ops
         for k, m, n_ops in (("A", 1, 1), ("B", 1, 2), ("Q", 2, 3), ("I", 1, 6))}
    return _propagate(st, s, e["A"], e["B"], e["Q"], e["I"], given_cm, 4, centre_err)
