"""A fast NumPy / scipy restatement of the reference's shoal detectors (echopype mask/shoal_detection/shoal_weill.py,
shoal_echoview.py), the oracle of the GPU fuzz tests at sizes where the reference's loops over labels (each touching
the whole image) would take minutes.  Planes are (ping_time, range_sample) of one channel: "vertical" is axis 1,
"horizontal" axis 0.  Gap filling is by the distance between the previous and the next foreground index along an axis
(cumulative max / min of indices); components come from ``ndimage.label`` + ``find_objects``; Echoview's linking is a
small union-find over components.  tests/test_shoal_host.py pins all of it to the reference-executed goldens."""
import os

import numpy as np
from scipy import ndimage

GOLDEN = "ref_shoal_goldens.npz"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def load_goldens():
    return np.load(GOLDEN_PATH, allow_pickle=False)


def unpack_mask(g, tag, shape):
    """The reference's boolean mask of a case (stored bit-packed)."""
    n = int(np.prod(shape))
    return np.unpackbits(g[f"{tag}_out"])[:n].astype(bool).reshape(shape)


def threshold(sv, thr):
    """``Sv > thr`` as ``np.ma.masked_greater`` evaluates it: the masked-array operation turns ``thr`` into a float64
    array first, so a float32 ``Sv`` is compared in float64 (``thr`` is NOT rounded to float32); NaN is False."""
    with np.errstate(invalid="ignore"):
        return np.asarray(sv, dtype=np.float64) > np.float64(thr)


def fill_gaps(m, maxgap, axis):
    """Background runs along ``axis`` with foreground on both sides and length <= ``maxgap`` become foreground."""
    m = np.moveaxis(m, axis, -1)
    n = m.shape[-1]
    idx = np.arange(n)
    prev = np.maximum.accumulate(np.where(m, idx, -1), axis=-1)
    nxt = np.minimum.accumulate(np.where(m, idx, n)[..., ::-1], axis=-1)[..., ::-1]
    out = m | ((prev >= 0) & (nxt < n) & (nxt - prev - 1 <= maxgap))
    return np.moveaxis(out, -1, axis)


def weill(sv, thr=-70.0, maxvgap=5, maxhgap=0, minvlen=0, minhlen=0):
    m = threshold(sv, thr)
    m = fill_gaps(m, maxvgap, 1)
    m = fill_gaps(m, maxhgap, 0)
    lab, n = ndimage.label(m)
    keep = np.zeros(n + 1, dtype=bool)
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        hlen, vlen = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
        keep[k] = not ((vlen < minvlen) or (hlen < minhlen))
    return keep[lab]


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def echoview(sv, idim, jdim, thr=-70.0, mincan=(3.0, 10.0), maxlink=(3.0, 15.0), minsho=(3.0, 15.0), details=False):
    idim, jdim = np.asarray(idim, dtype=np.float64), np.asarray(jdim, dtype=np.float64)
    m = threshold(sv, thr)
    P, S = m.shape
    lab, n = ndimage.label(m, np.ones((3, 3)))
    objs = ndimage.find_objects(lab)
    box = np.array([[sl[1].start, sl[1].stop - 1, sl[0].start, sl[0].stop - 1] for sl in objs],
                   dtype=np.int64).reshape(n, 4)  # i0, i1 (samples), j0, j1 (pings)

    def small(b, lim):
        return (idim[b[1] + 1] - idim[b[0]] < lim[0]) or (jdim[b[3] + 1] - jdim[b[2]] < lim[1])

    alive = np.array([not small(b, mincan) for b in box], dtype=bool).reshape(n)
    par = np.arange(n)
    touched = np.zeros(n, dtype=bool)
    alive1 = np.concatenate([[False], alive])
    for a in np.flatnonzero(alive):
        i0, i1, j0, j1 = box[a]
        i00 = int(np.argmin(np.abs(idim - (idim[i0] - (maxlink[0] + 1)))))
        i11 = int(np.argmin(np.abs(idim - (idim[i1] + (maxlink[0] + 1))))) + 1
        j00 = int(np.argmin(np.abs(jdim - (jdim[j0] - (maxlink[1] + 1)))))
        j11 = int(np.argmin(np.abs(jdim - (jdim[j1] + (maxlink[1] + 1))))) + 1
        sub = lab[j00:j11, i00:i11]
        ids = np.unique(sub[alive1[sub]]) - 1
        if ids.size == 0:
            continue
        touched[ids] = True
        r = _find(par, ids[0])
        for b in ids[1:]:
            rb = _find(par, b)
            if rb != r:
                par[max(r, rb)] = min(r, rb)
                r = min(r, rb)
    keep = alive.copy()
    roots = np.array([_find(par, c) for c in range(n)], dtype=np.int64)
    for g in np.unique(roots[alive & touched]):
        mem = np.flatnonzero((roots == g) & alive & touched)
        gb = [box[mem, 0].min(), box[mem, 1].max(), box[mem, 2].min(), box[mem, 3].max()]
        if small(gb, minsho):
            keep[mem] = False
    out = np.concatenate([[False], keep])[lab]
    if details:
        return out, {"components": n, "candidates": int(alive.sum()), "groups": len(np.unique(roots[alive & touched])),
                     "untouched": int((alive & ~touched).sum())}
    return out
