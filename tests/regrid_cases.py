"""Seeded inputs of the regrid_Sv tests (tests/test_regrid_host.py, tests/test_gpu_regrid.py): data only."""
import numpy as np

D0 = 0.047  # metres between the samples of the finest channel


def ranges(C, S, seed, d0=D0):
    """(C, S) float64 ranges: channel 0 at spacing d0, channel 1 at 4 d0, channel 2 at irregular steps of 0.2 .. 2.2 d0
    (further channels repeat the three).  Every row starts 0.3 steps above 0, so its first cell reaches below the grid."""
    g = np.random.default_rng([seed, C, S, 1])
    out = np.empty((C, S))
    for c in range(C):
        steps = (np.full(S, d0), np.full(S, 4 * d0), g.uniform(0.2, 2.2, S) * d0)[c % 3]
        out[c] = 0.3 * steps[0] + np.cumsum(steps) - steps[0]
    return out


def volume(seed, C, P, S, sv_dtype, range_dtype, form="CS", d0=D0, nan_frac=0.08):
    """(Sv (C, P, S), range) of the two types.  ``form``: the range as "S" (one row for all), "CS" (one per channel) or
    "CPS" (a cube: every ping stretched by another factor).  Sv is uniform in [-90, -30] dB with runs of 1 .. 6 NaN."""
    g = np.random.default_rng([seed, C, P, S, 2])
    r = ranges(C, S, seed, d0)
    if form == "S":
        r = r[1 % C]
    elif form == "CPS":
        r = r[:, None, :] * (1.0 + 0.003 * np.arange(P))[None, :, None]
    elif form != "CS":
        raise ValueError(form)
    sv = g.uniform(-90.0, -30.0, (C, P, S))
    starts = np.argwhere(g.random((C, P, S)) < nan_frac / 3.5)
    for (c, p, s), n in zip(starts, g.integers(1, 7, len(starts))):
        sv[c, p, s:s + n] = np.nan
    return sv.astype(sv_dtype), np.ascontiguousarray(r).astype(range_dtype)


def plant(sv, r):
    """Into a (3+, 2+, 12+) volume with a cube range (changed in place): a NaN range tail of another length in every
    ping, three repeated leading zeros, +-inf samples, and three rows to refuse -- one that decreases once, one with a
    single finite range, one with none.  Returns the number of rows to refuse."""
    C, P, S = sv.shape
    assert r.shape == sv.shape and C >= 3 and P >= 2 and S >= 12
    for p in range(P):
        tail = (3 * p + 1) % (S - 8)
        r[:, p, S - tail:] = np.nan
    r[0, 0] = np.maximum(r[0, 0] - r[0, 0, 2], 0.0)  # (the reference clips echo_range at 0)
    assert (r[0, 0, :3] == 0).all() and r[0, 0, 3] > 0
    sv[0, 1, 5] = np.inf
    sv[1, 0, 2:5] = -np.inf
    sv[0, 0, 1] = -np.inf
    r[1, 1, [4, 5]] = r[1, 1, [5, 4]]  # decreases once
    r[2, 0, 1:] = np.nan  # n == 1
    r[2, 1, :] = np.nan  # n == 0
    return 3


def grid(rmax, range_bin, odd=False):
    """The edges compute_MVBS would use for ``rmax`` (np.arange defines them); ``odd``: one more cell if their number is
    even, so that the output rows of a cube start at unaligned addresses."""
    e = np.arange(0, rmax + range_bin, range_bin)
    if odd and (len(e) - 1) % 2 == 0:
        e = np.arange(0, rmax + 2 * range_bin, range_bin)
        if (len(e) - 1) % 2 == 0:
            e = e[:-1]
    return e
