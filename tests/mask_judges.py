"""Shared judges of the noise-mask GPU tests (test_gpu_masks.py, test_gpu_masks_f32.py, test_gpu_masks_api.py,
test_gpu_fuzz.py): a pooled Sv and its mask, an attenuated-signal mask, and two checks on a case's INPUT.  float64 is held
to 1e-9, float32 to the derived bounds of f32_bounds.py.  Pure NumPy."""
import warnings

import numpy as np

import f32_bounds as fb
from oracle import masks as omask

F64_TOL = 1e-9   # float64: relative tolerance of a pooled value, and the margin (dB) a decision is left out within


def close(got, exp, rtol, what=""):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{what}: NaN pattern")
    fin = np.isfinite(exp)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(exp)], exp[~fin & ~np.isnan(exp)])
    err = np.abs(got[fin] - exp[fin]) / np.maximum(np.abs(exp[fin]), 1.0)
    assert err.size == 0 or err.max() <= rtol, f"{what}: max rel err {err.max():.3e} > {rtol}"


def t_of(dtype, x):
    """A window parameter as the kernel holds it: rounded to float32 for a float32 case (``(T)bin`` ...), explicitly --
    not left to NumPy's scalar promotion."""
    return np.float32(x) if dtype == "float32" else float(x)


def judge_pooled(dtype, what, sv, pooled, mask, exp, thr, bound=None, need_nan=True):
    """A pooled Sv and the mask ``Sv - pooled > thr`` against the oracle's ``exp`` (run on the values ``sv`` of the
    case's type).  float64: 1e-9 and the decisions outside a 1e-9 dB margin.  float32: ``bound`` (a derived bound of
    tests/f32_bounds.py), the decisions outside the bound of the compared quantity, at most 0.1 % of them inside it,
    and a case that is not degenerate (a mask with both values, a pooled field with finite and NaN elements)."""
    sv64 = np.asarray(sv, np.float64)
    with np.errstate(invalid="ignore"):
        margin = sv64 - exp - thr
    if dtype == "float64":
        close(pooled, exp, F64_TOL, what)
        if mask is not None:
            sure = ~(np.abs(margin) < F64_TOL)
            np.testing.assert_array_equal(np.asarray(mask).astype(bool)[sure], (margin > 0)[sure], err_msg=what)
        return
    fb.assert_f32_close(pooled, exp, bound, "mask: " + what)
    assert np.isfinite(exp).any() and (np.isnan(exp).any() or not need_nan), what
    if mask is not None:
        bd = fb.threshold_decision_bound(sv64, exp, bound, thr)
        fb.assert_few_near(margin, bd, what)
        fb.check_decisions(np.asarray(mask).astype(bool), margin > 0, margin, bd, what)
        assert (margin > 0).any() and not (margin > 0).all(), what


def value_mean_bound(sv, exp, n):
    """``pooled_mean_bound`` of a value-window nanmean, whatever route summed it: the running sums of a row hold up to S
    values, the sum carried down a column up to (2n+1) S, over S + P additions."""
    P, S = sv.shape[-2:]
    return fb.pooled_mean_bound(sv, exp, carried_terms=(2 * n + 1) * S, carried_ops=S + P)


def attenuated_medians(sv, range_var, upper, lower, n, thr):
    """The two medians ``echopy_attenuated_signal_mask`` compares (oracle/masks.py:120-137, restated to expose them):
    (ping median, block median) in dB per ping, NaN where the oracle does not compare.  ``sv`` (P, S) float64."""
    P, S = sv.shape
    ping, block = np.full(P, np.nan), np.full(P, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for p in range(P):
            up = int(np.argmin(np.abs(range_var[p] - upper)))
            lw = int(np.argmin(np.abs(range_var[p] - lower)))
            if p - n < 0 or p + n > P - 1 or np.all(np.isnan(sv[p, up:lw])):
                continue
            ping[p] = 10 * np.log10(np.nanmedian(10 ** (sv[p, up:lw] / 10)))
            block[p] = 10 * np.log10(np.nanmedian(10 ** (sv[p - n:p + n, up:lw] / 10)))
    return ping, block


def judge_attenuated(what, got, sv, depth, upper, lower, n, thr, need_both=True):
    """A float32 attenuated-signal mask: the oracle's mask on the float32 range and limits; a ping may differ only where
    ping median - block median lies within ``attenuated_decision_bound`` of the threshold (at most 0.1 % of the pings)."""
    C, P, S = sv.shape
    sv64 = sv.astype(np.float64)
    up32, lw32 = np.float32(upper), np.float32(lower)
    exp = np.stack([omask.echopy_attenuated_signal_mask(sv64[c], depth[c], up32, lw32, n, thr) for c in range(C)])
    med = [attenuated_medians(sv64[c], depth[c], up32, lw32, n, thr) for c in range(C)]
    ping, block = np.stack([m[0] for m in med]), np.stack([m[1] for m in med])
    with np.errstate(invalid="ignore"):
        margin = ping - block - thr
    np.testing.assert_array_equal(margin < 0, exp[:, :, 0], err_msg=f"{what}: the restated medians decide as the oracle")
    bd = fb.attenuated_decision_bound(ping, block, thr)
    fb.assert_few_near(margin, bd, what)
    got = np.asarray(got).astype(bool)
    assert (got == got[:, :, :1]).all(), what
    fb.check_decisions(got[:, :, 0], exp[:, :, 0], margin, bd, what)
    assert not need_both or (exp.any() and not exp.all()), what
    return exp


def same_bins(depth32, bin32, r0, delta, nb):
    """The edges np.arange gives on float32 scalars (its step is the float32 sum r0 + bin minus r0) and the kernel's
    (r0 + j * delta in double) put every sample of the case into the same bin: the case does not hinge on how an arange
    of float32 scalars rounds its step."""
    e_or = np.arange(np.nanmin(depth32), np.nanmax(depth32) + bin32, bin32)
    e_k = r0 + np.arange(nb + 1) * delta
    d = depth32[np.isfinite(depth32)].astype(np.float64)
    return len(e_or) == nb + 1 and np.array_equal(np.searchsorted(e_or, d, side="right"), np.searchsorted(e_k, d, side="right"))


def assert_edges_decide(sv, depth, func, dbin, n, excl, exp, bound):
    """The input does its job: with the membership decided on the float64 depth at least 1 % of the finite outputs differ
    from the float32-membership oracle ``exp`` by more than the bound."""
    other = omask.pool_Sv(sv.astype(np.float64), depth.astype(np.float64), func, float(dbin), n, float(excl))
    fin = np.isfinite(exp) & np.isfinite(other)
    share = float((np.abs(other[fin] - exp[fin]) > bound[fin]).mean())
    assert share >= 0.01, f"float32 and float64 membership differ at only {share:.4f} of the outputs"
    return share
