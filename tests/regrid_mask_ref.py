"""NumPy judge of mask.regrid_mask: edges from ``np.arange``, membership by ``np.searchsorted``, one loop over the
cells.  A cell is 1 where samples fall into it and all are one (AND) / one of them is (OR), 0 otherwise -- the
reference's group-by mean with ``fill_value=0.0`` tested for ``== 1.0`` / ``!= 0.0``.  tests/test_regrid_mask_host.py
checks the memberships against pandas (``pd.cut`` on ``IntervalIndex.from_breaks``) and the time edges against
``Series.resample``."""
import numpy as np

DAY = 86400 * 10**9


def range_edges(rng, range_bin, range_var_max=None):
    """np.arange(0, max + 1e-8 + bin, bin), max the NaN-skipping maximum unless given."""
    if range_var_max is None:
        range_var_max = np.nanmax(np.asarray(rng, dtype=np.float64))
    return np.arange(0, (range_var_max + 1e-8) + range_bin, range_bin)


def time_edges(ping_ns, dt_ns):
    """int64 ns edges of fixed-frequency bins anchored at midnight of the first ping's day, from the bin of the first
    ping to the bin of the last, plus the closing edge."""
    ping_ns = np.asarray(ping_ns, dtype=np.int64)
    first, last = int(ping_ns.min()), int(ping_ns.max())
    origin = first // DAY * DAY
    e0 = origin + (first - origin) // dt_ns * dt_ns
    n = (last - e0) // dt_ns + 1
    return e0 + dt_ns * np.arange(n + 1, dtype=np.int64)


def member(x, edges, closed):
    """Index of the interval of ``edges`` that holds each x, -1 for none (NaN, outside, the open end)."""
    x = np.asarray(x)
    i = np.searchsorted(edges, x, side="right" if closed == "left" else "left") - 1
    ok = (i >= 0) & (i < len(edges) - 1)
    if x.dtype.kind == "f":
        ok &= ~np.isnan(x)
    return np.where(ok, i, -1)


def _indices(mask, ping_ns, rng, tedges, redges, closed):
    T, P, D = mask.shape
    ti = np.broadcast_to(member(ping_ns, tedges, closed)[:, None], (P, D))
    ri = np.broadcast_to(member(np.asarray(rng, dtype=np.float64), redges, closed), (P, D))
    return ti, ri


def regrid(mask, ping_ns, rng, range_bin, dt_ns, func="logical-AND", closed="left", third=None, range_var_max=None):
    """mask (T, P, D) of any type holding 0 / 1 -> (sorted distinct ``third`` values, time edges, range edges,
    result (G, n_t, n_r) of the mask's type).  Plain loops over the cells."""
    mask = np.asarray(mask)
    T, P, D = mask.shape
    third = np.arange(T) if third is None else np.asarray(third)
    uniq = np.unique(third)
    tedges, redges = time_edges(ping_ns, dt_ns), range_edges(rng, range_bin, range_var_max)
    ti, ri = _indices(mask, ping_ns, rng, tedges, redges, closed)
    out = np.zeros((len(uniq), len(tedges) - 1, len(redges) - 1), dtype=mask.dtype)
    for g, u in enumerate(uniq):
        planes = mask[third == u]
        for tb in range(out.shape[1]):
            in_t = ti == tb
            if not in_t.any():
                continue
            for rb in range(out.shape[2]):
                vals = planes[:, in_t & (ri == rb)]
                if vals.size:
                    out[g, tb, rb] = bool((vals != 0).all()) if func == "logical-AND" else bool((vals != 0).any())
    return uniq, tedges, redges, out


def regrid_by_counts(mask, ping_ns, rng, range_bin, dt_ns, func="logical-AND", closed="left", third=None,
                     range_var_max=None):
    """The same result from per-cell counts (for grids with too many cells to loop over); the host tests tie it to
    ``regrid``."""
    mask = np.asarray(mask)
    T, P, D = mask.shape
    third = np.arange(T) if third is None else np.asarray(third)
    uniq, gi = np.unique(third, return_inverse=True)
    tedges, redges = time_edges(ping_ns, dt_ns), range_edges(rng, range_bin, range_var_max)
    ti, ri = _indices(mask, ping_ns, rng, tedges, redges, closed)
    nt, nr = len(tedges) - 1, len(redges) - 1
    ok = (ti >= 0) & (ri >= 0)
    cnt = np.zeros((len(uniq), nt, nr), dtype=np.int64)
    ones = np.zeros_like(cnt)
    for t in range(T):
        flat = (gi[t] * nt + ti[ok]) * nr + ri[ok]
        np.add.at(cnt.reshape(-1), flat, 1)
        np.add.at(ones.reshape(-1), flat, (mask[t][ok] != 0).astype(np.int64))
    res = ((cnt > 0) & (ones == cnt)) if func == "logical-AND" else (ones > 0)
    return uniq, tedges, redges, res.astype(mask.dtype)
