"""A fast NumPy restatement of the reference's seafloor detectors (echopype mask/seafloor_detection/bottom_basic.py,
bottom_blackwell.py), the oracle of the GPU fuzz tests at sizes where the reference's direct convolve2d would take
minutes.  Planes are (ping_time, range_sample) of one channel.  The box filter is window sums of cumulative sums with
NaN counts over the "symm" extension (the edge sample repeated, periodic with period 2N for windows longer than the
axis); tests/test_seafloor_host.py pins all of it to the reference-executed goldens."""
import os
import warnings

import numpy as np

GOLDEN = "ref_seafloor_goldens.npz"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def _reflect(m, n):
    m = np.mod(m, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _window_sums(x, w, axis):
    """sum over i - w//2 .. i + w - 1 - w//2 of the symm-extended x along ``axis``; NaN where the window holds one."""
    n = x.shape[axis]
    h = w // 2
    idx = _reflect(np.arange(-h, n + w - 1 - h), n)
    xp = np.take(x, idx, axis=axis)
    nan = np.isnan(xp)
    v = np.where(nan, 0.0, xp)
    shape = list(v.shape)
    shape[axis] = 1
    cs = np.concatenate([np.zeros(shape), np.cumsum(v, axis=axis)], axis=axis)
    cn = np.concatenate([np.zeros(shape, dtype=np.int64), np.cumsum(nan, axis=axis)], axis=axis)
    hi = np.take(cs, np.arange(w, n + w), axis=axis) - np.take(cs, np.arange(0, n), axis=axis)
    bad = np.take(cn, np.arange(w, n + w), axis=axis) - np.take(cn, np.arange(0, n), axis=axis)
    return np.where(bad > 0, np.nan, hi)


def box_mean(x, w):
    """convolve2d(x, ones((w, w)) / w**2, "same", boundary="symm") up to the order of the additions (f64)."""
    x = np.asarray(x, dtype=np.float64)
    return _window_sums(_window_sums(x, w, 1), w, 0) / (w * w)


def basic(sv, depth0, tmin, tmax, skip, offset):
    """bottom_basic: (P,) f64."""
    sv = np.asarray(sv)
    t0, t1 = np.asarray(tmin, sv.dtype), np.asarray(tmax, sv.dtype)  # NumPy rounds a Python float to the array's type
    cond = (sv[:, skip:] > t0) & (sv[:, skip:] < t1)
    idx = cond.argmax(axis=1) + skip
    return np.asarray(depth0, dtype=np.float64)[idx] - float(offset)


def _lin2log(x):
    return 10 * np.log10(x)


def _log2lin(x):
    return 10 ** (x / 10)


def blackwell(sv, theta, phi, r, tSv, ttheta, tphi, offset, r0, r1, wtheta, wphi, details=False):
    """bottom_blackwell: (P,) of r's dtype; with ``details`` also a dict (crop, angle mask, threshold, the smallest
    relative distance of a smoothed angle square from its threshold)."""
    from scipy import ndimage

    sv, theta, phi, r = np.asarray(sv), np.asarray(theta), np.asarray(phi), np.asarray(r)
    P, S = sv.shape
    r0_idx = int(np.nanargmin(abs(r - r0)))
    r1_idx = int(np.nanargmin(abs(r - r1))) + 1
    svc = sv[:, r0_idx:r1_idx]
    info = {"r0_idx": r0_idx, "r1_idx": r1_idx, "margin": np.inf, "threshold": None, "n_masked": 0}
    idx = np.zeros(P, dtype=np.int64)
    if svc.size:
        mt = box_mean(theta[:, r0_idx:r1_idx], wtheta) ** 2
        mp = box_mean(phi[:, r0_idx:r1_idx], wphi) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            for m, t in ((mt, ttheta), (mp, tphi)):
                f = np.isfinite(m)
                if f.any():
                    rel = np.abs(m[f] - t) / max(abs(t), 1e-300)
                    info["margin"] = min(info["margin"], float(rel.min()))
        amask = (mt > ttheta) | (mp > tphi)
        info["n_masked"] = int(amask.sum())
        if amask.any():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                thr = float(_lin2log(np.nanmedian(_log2lin(svc[amask]))))
            if np.isnan(thr):
                thr = np.inf
            if thr < tSv:
                thr = tSv
            info["threshold"] = thr
            items = ndimage.label(svc > thr, np.ones((3, 3), dtype=bool))[0]
            keep = np.zeros(items.max() + 1, dtype=bool)
            keep[np.unique(items[amask])] = True
            keep[0] = False
            kept = keep[items]
            any_k = kept.any(axis=1)
            idx = np.where(any_k, kept.argmax(axis=1) + r0_idx, 0)
    out = r[idx] - offset
    return (out, info) if details else out


def load_goldens(path=GOLDEN_PATH):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
