"""commongrid.regrid_Sv restated in NumPy: the oracle of csrc/regrid.hip (there is no reference implementation to hold
against).  Plain loops, float64 throughout, one rounding to the output type.

One row, ``r`` its range promoted to float64 and ``v`` its Sv, onto the cells ``[e[j], e[j+1])``:
  n     the length of the leading run of finite r; samples behind it are ignored
  the row is UNORDERED if n < 2 or r[:n] decreases somewhere: every output NaN, coverage 0
  m     n + 1 cell bounds: m[i] = (r[i-1] + r[i]) / 2, m[0] = r[0] - (r[1] - r[0]) / 2, m[n] = r[n-1] + (r[n-1] - r[n-2]) / 2
  o_ij  = max(0, min(m[i+1], e[j+1]) - max(m[i], e[j]))
  W_j   = sum_i o_ij,  N_j = sum_i o_ij * 10^(v_i / 10)  over i < n with v_i not NaN and o_ij > 0, in ascending i
  Sv_j  = 10 log10(N_j / W_j) where W_j > 0, else NaN;  coverage_j = W_j / (e[j+1] - e[j])
"""
import numpy as np


def cell_bounds(r):
    """(n, m) of one row: m is None when the row is unordered."""
    r = np.asarray(r).astype(np.float64)
    fin = np.isfinite(r)
    n = int(r.size if fin.all() else np.argmin(fin))
    if n < 2 or np.any(r[1:n] < r[:n - 1]):
        return n, None
    m = np.empty(n + 1)
    for i in range(1, n):
        m[i] = (r[i - 1] + r[i]) / 2
    m[0] = r[0] - (r[1] - r[0]) / 2
    m[n] = r[n - 1] + (r[n - 1] - r[n - 2]) / 2
    return n, m


def regrid_row_ref(r, v, e):
    """-> (Sv (J,), coverage (J,), unordered) in float64, not yet rounded."""
    e = np.asarray(e, dtype=np.float64)
    J = e.size - 1
    v = np.asarray(v).astype(np.float64)
    n, m = cell_bounds(r)
    if m is None:
        return np.full(J, np.nan), np.zeros(J), True
    W, N = np.zeros(J), np.zeros(J)
    with np.errstate(over="ignore"):
        lin = np.float64(10.0) ** (v / 10.0)
    for i in range(n):
        if np.isnan(v[i]) or not m[i + 1] > m[i]:
            continue
        j = max(int(np.searchsorted(e, m[i], side="right")) - 1, 0)
        while j < J and e[j] < m[i + 1]:
            o = min(m[i + 1], e[j + 1]) - max(m[i], e[j])
            if o > 0:
                W[j] += o
                N[j] += o * lin[i]
            j += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        sv = np.where(W > 0, 10.0 * np.log10(N / W), np.nan)
    return sv, W / (e[1:] - e[:-1]), False


def _cube(rng, shape):
    """A range over (S,), (C, S) -- channel first, as in a dataset -- or (C, P, S) as a read-only view of that shape."""
    rng = np.asarray(rng)
    return np.broadcast_to(rng[:, None, :] if rng.ndim == 2 else rng, shape)


def regrid_ref(sv, rng, e, dtype=None):
    """``sv`` (C, P, S) and ``rng`` over (S,), (C, S) or (C, P, S) -> (Sv (C, P, J), coverage (C, P, J), number of unordered rows),
    the two arrays rounded once to ``dtype`` (default: sv's)."""
    sv = np.asarray(sv)
    C, P, S = sv.shape
    rng = _cube(rng, sv.shape)
    dtype = np.dtype(dtype or sv.dtype)
    J = len(e) - 1
    out, cov, bad = np.empty((C, P, J)), np.empty((C, P, J)), 0
    for c in range(C):
        for p in range(P):
            out[c, p], cov[c, p], u = regrid_row_ref(rng[c, p], sv[c, p], e)
            bad += int(u)
    with np.errstate(over="ignore"):
        return out.astype(dtype), cov.astype(dtype), bad


def conserved_sides(sv, rng, e):
    """Both sides of the conserved quantity, one pair per ordered row of (C, P, S) input, from the UNROUNDED oracle:
    sum_j 10^(Sv_j/10) coverage_j (e[j+1] - e[j])  and  sum_i 10^(v_i/10) |[m[i], m[i+1]) n [e[0], e[J])| over the non-NaN
    samples -> two (C, P) arrays, NaN in unordered rows."""
    sv = np.asarray(sv)
    C, P, S = sv.shape
    rng = _cube(rng, sv.shape)
    e = np.asarray(e, dtype=np.float64)
    lhs, rhs = np.full((C, P), np.nan), np.full((C, P), np.nan)
    for c in range(C):
        for p in range(P):
            got, cov, bad = regrid_row_ref(rng[c, p], sv[c, p], e)
            if bad:
                continue
            n, m = cell_bounds(rng[c, p])
            v = sv[c, p].astype(np.float64)
            width = np.clip(np.minimum(m[1:], e[-1]) - np.maximum(m[:-1], e[0]), 0, None)
            ok = ~np.isnan(v[:n]) & (width > 0)
            rhs[c, p] = np.sum((10.0 ** (v[:n][ok] / 10.0)) * width[ok])
            use = cov > 0
            lhs[c, p] = np.sum((10.0 ** (got[use] / 10.0)) * cov[use] * (e[1:] - e[:-1])[use])
    return lhs, rhs
