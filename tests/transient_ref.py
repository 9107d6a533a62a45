"""A NumPy restatement of the reference's transient-noise detectors (echopype clean/transient_noise/
transient_fielding.py, transient_matecho.py), the oracle of the GPU tests.  It evaluates the reference's own
expressions ping by ping (so it agrees with it to the bit, dtype by dtype), can be asked for a subset of pings, and
returns per ping the mask column and the DECISION MARGIN: the smallest |quantity - threshold| over the comparisons the
reference actually evaluates for that ping --
    fielding   p75 - maxts;  (ping - block) - thr[0] when the first holds;  every walk step's diff - thr[1]
    matecho    H - min_window;  mean_db - (pctl + delta_db)           (after dilation: the smallest over [j-e, j+e])
A comparison with a NaN side is False whatever the rounding and counts as infinitely far; so does a ping that evaluates
none.  The GPU arithmetic is float64 for both input types, the reference keeps float32 inputs in float32: a GPU test
compares the pings whose margin is at least MARGIN and may leave out the rest.
tests/test_transient_host.py pins all of it to the reference-executed goldens (scripts/gen_transient_goldens.py),
margins included."""
import os
import warnings

import numpy as np

GOLDEN = "ref_transient_goldens.npz"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
MARGIN = {"float64": 1e-9, "float32": 2e-3}  # dB: tests/test_gpu_masks.py's


def load_goldens():
    return np.load(GOLDEN_PATH, allow_pickle=False)


def unpack_mask(g, tag, shape):
    n = int(np.prod(shape))
    return np.unpackbits(g[f"{tag}_out"])[:n].astype(bool).reshape(shape)


def _log2lin(x):
    return 10 ** (x / 10)


def _lin2log(x):
    return 10 * np.log10(x)


def _gap(q, thr):
    """|q - thr|, infinite when the comparison has a NaN side."""
    d = abs(float(q) - float(thr))
    return d if d == d else np.inf


def fielding_rows(r, r0, r1, roff, jumps):
    """(up, lw, rmin, sf) by the reference's expressions, None where it returns early."""
    r = np.asarray(r)
    if r0 > r1:
        return None
    if (r0 > r[-1]) or (r1 < r[0]):
        return None
    up = np.argmin(abs(r - r0))
    lw = np.argmin(abs(r - r1))
    rmin = np.argmin(abs(r - roff))
    dr = float(np.nanmedian(np.diff(r)))
    sf = max(1, int(round(jumps / dr)))
    return int(up), int(lw), int(rmin), sf


def fielding(sv, r, r0=900, r1=1000, n=30, thr=(3, 1), roff=20, jumps=5, maxts=-35, pings=None):
    """One channel: ``sv`` (P, S), ``r`` (S,).  -> (valid (len(pings), S) bool, margin (len(pings),) float64);
    ``pings`` defaults to all."""
    P, S = sv.shape
    pings = np.arange(P) if pings is None else np.asarray(pings)
    valid = np.ones((len(pings), S), dtype=bool)
    margin = np.full(len(pings), np.inf)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        rows = fielding_rows(r, r0, r1, roff, jumps)
        if rows is None:
            return valid, margin
        up, lw, rmin, sf = rows
        Sv = np.asarray(sv).T  # (range, ping), as the reference holds it
        for i, j in enumerate(pings):
            if (j - n < 0) or (j + n > P - 1) or np.all(np.isnan(Sv[up:lw, j])):
                continue
            pm = _lin2log(np.nanmedian(_log2lin(Sv[up:lw, j])))
            p75 = _lin2log(np.nanpercentile(_log2lin(Sv[up:lw, j]), 75))
            bm = _lin2log(np.nanmedian(_log2lin(Sv[up:lw, j - n:j + n])))
            m = _gap(p75, maxts)
            if p75 < maxts:
                m = min(m, _gap(pm - bm, thr[0]))
                if (pm - bm) > thr[0]:
                    r0_, r1_ = up - sf, up
                    while r0_ > rmin:
                        a = _lin2log(np.nanmedian(_log2lin(Sv[r0_:r1_, j])))
                        b = _lin2log(np.nanmedian(_log2lin(Sv[r0_:r1_, j - n:j + n])))
                        r0_, r1_ = r0_ - sf, r1_ - sf
                        m = min(m, _gap(a - b, thr[1]))
                        if (a - b) < thr[1]:
                            break
                    valid[i, r0_:] = False
            margin[i] = m
    return valid, margin


def matecho_raw(sv, r, bottom=None, start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=12,
                min_window=20, pings=None):
    """Per-ping flags BEFORE dilation and their margins: ``sv`` (P, S), ``r`` (S,), ``bottom`` (P,) or None."""
    P, S = sv.shape
    pings = np.arange(P) if pings is None else np.asarray(pings)
    bad = np.zeros(len(pings), dtype=bool)
    margin = np.full(len(pings), np.inf)
    r = np.asarray(r)
    Sv = np.asarray(sv).T
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        depth_mask = (r >= start_depth) & (r <= start_depth + window_meter)
        if bottom is None:
            bottom = np.full(P, r[-1], dtype=float)
        else:
            bottom = np.array(bottom, dtype=float, copy=True)
            bottom[np.isnan(bottom)] = r[-1]
        h = window_ping // 2
        for i, j in enumerate(pings):
            j0, j1 = max(0, j - h), min(P, j + h)
            local_bottom = np.min(bottom[j0:j1])
            refined = depth_mask & (r < local_bottom)
            if not np.any(refined):
                continue
            H = (r[1] - r[0]) * np.sum(refined)
            margin[i] = _gap(H, min_window)
            if H < min_window:
                continue
            win = Sv[refined, j0:j1]
            flat = win[~np.isnan(win)]
            if flat.size == 0:
                continue
            pctl = np.percentile(flat, percentile)
            mean_db = _lin2log(np.nanmean(_log2lin(Sv[refined, j])))
            margin[i] = min(margin[i], _gap(mean_db, pctl + delta_db))
            bad[i] = mean_db > pctl + delta_db
    return bad, margin


def matecho_route(sv, r, bottom=None, start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=12,
                  min_window=20, **_):
    """How the DEVICE decides each ping (a float64 replay of tr_matecho_flag_kernel's counting sweep) -> (route (P,)
    int, t (P,) float): route 0 = no decision (skipped), 1 = the count says "not flagged" (at most k values with
    v + delta_db < mean_db), 2 = the count says "flagged" (at least k + 2, or k + 1 without interpolation), 3 = the
    threshold lies between ranks k and k + 1: the percentile is selected and interpolated; t = the fractional part
    of the virtual index (N - 1) * percentile / 100."""
    P, S = sv.shape
    r = np.asarray(r)
    Sv = np.asarray(sv, dtype=np.float64).T
    route, frac = np.zeros(P, dtype=int), np.full(P, np.nan)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        depth_mask = (r >= start_depth) & (r <= start_depth + window_meter)
        b = np.full(P, r[-1], dtype=float) if bottom is None else np.where(np.isnan(bottom), r[-1], bottom).astype(float)
        h = window_ping // 2
        for j in range(P):
            j0, j1 = max(0, j - h), min(P, j + h)
            refined = depth_mask & (r < np.min(b[j0:j1]))
            if not np.any(refined) or (r[1] - r[0]) * np.sum(refined) < min_window:
                continue
            own = Sv[refined, j]
            if np.all(np.isnan(own)):
                continue
            mean_db = 10 * np.log10(np.nanmean(10 ** (own / 10)))
            win = Sv[refined, j0:j1]
            flat = win[~np.isnan(win)]
            v = (flat.size - 1) * (percentile / 100.0)
            k, frac[j] = int(np.floor(v)), v - np.floor(v)
            nxt = frac[j] > 0 and k + 1 < flat.size
            lt = int((flat + delta_db < mean_db).sum())
            route[j] = 1 if lt <= k else (2 if lt >= k + (2 if nxt else 1) else 3)
    return route, frac


def fielding_p75_bracket(sv, r, r0, r1, n, maxts, **_):
    """Per ping: True where ``maxts`` lies strictly between the two layer values (dB) that the 75th percentile
    interpolates, so that the interpolation itself decides ``p75 < maxts``; and the count of non-NaN layer samples."""
    P, S = sv.shape
    up, lw = int(np.argmin(abs(np.asarray(r) - r0))), int(np.argmin(abs(np.asarray(r) - r1)))
    out, cnt = np.zeros(P, dtype=bool), np.zeros(P, dtype=int)
    for j in range(P):
        a = np.sort(np.asarray(sv[j, up:lw], dtype=np.float64))
        a = a[~np.isnan(a)]
        cnt[j] = a.size
        if a.size < 2 or j - n < 0 or j + n > P - 1:
            continue
        v = (a.size - 1) * 0.75
        k = int(np.floor(v))
        out[j] = v > k and a[k] < maxts < a[k + 1]
    return out, cnt


def dilate(bad, margin, extend_ping):
    """binary_dilation with ones(2e + 1) along pings; a ping's margin becomes the smallest of those it depends on."""
    e = int(extend_ping)
    if e <= 0:
        return bad, margin
    P = len(bad)
    out, m = bad.copy(), margin.copy()
    for j in range(P):
        lo, hi = max(0, j - e), min(P, j + e + 1)
        out[j] = bad[lo:hi].any()
        m[j] = margin[lo:hi].min()
    return out, m


def matecho(sv, r, bottom=None, start_depth=220, window_meter=450, window_ping=100, percentile=25, delta_db=12,
            extend_ping=0, min_window=20, pings=None):
    """One channel -> (valid (len(pings),) bool per ping: the mask is whole columns; margin (len(pings),))."""
    P = sv.shape[0]
    pings = np.arange(P) if pings is None else np.asarray(pings)
    e = max(int(extend_ping), 0)
    need = np.unique(np.clip(np.add.outer(pings, np.arange(-e, e + 1)), 0, P - 1)) if e else pings
    bad_n, mar_n = matecho_raw(sv, r, bottom, start_depth, window_meter, window_ping, percentile, delta_db, min_window,
                               need)
    if not e:
        return ~bad_n, mar_n
    bad, mar = np.zeros(P, dtype=bool), np.full(P, np.inf)
    bad[need], mar[need] = bad_n, mar_n
    bad, mar = dilate(bad, mar, e)
    return ~bad[pings], mar[pings]


def detect(method, sv, rng, bottom=None, **kw):
    """All channels: ``sv`` (C, P, S), ``rng`` (C, S), ``bottom`` None, (P,) or (C, P) -> (valid (C, P, S), margin
    (C, P))."""
    C, P, S = sv.shape
    valid = np.ones((C, P, S), dtype=bool)
    margin = np.full((C, P), np.inf)
    for c in range(C):
        if method == "fielding":
            valid[c], margin[c] = fielding(sv[c], rng[c], **kw)
        else:
            b = None if bottom is None else (bottom if np.ndim(bottom) == 1 else bottom[c])
            v, margin[c] = matecho(sv[c], rng[c], b, **kw)
            valid[c] = v[:, None]
    return valid, margin


# ---- the seeded fuzz cases of tests/test_gpu_transient.py (a CPU test asserts their margins stay within the cap) ---
def fuzz_cases():
    """(tag, method, dtype, C, P, S, seed, params): continuous (ungridded) Sv, elevations from 2 dB up."""
    F = []
    for i, (dt, C, P, S, prm) in enumerate([
        ("float64", 1, 96, 260, dict(r0=500, r1=600, n=10, thr=(3, 1), roff=50, jumps=12, maxts=-35)),
        ("float32", 2, 140, 330, dict(r0=600, r1=720, n=15, thr=(2.5, 0.8), roff=100, jumps=20, maxts=-40)),
        ("float64", 3, 83, 411, dict(r0=700, r1=900, n=6, thr=(3, 1), roff=20, jumps=5, maxts=-35)),
        ("float32", 1, 301, 257, dict(r0=400, r1=560, n=30, thr=(4, 2), roff=150, jumps=33, maxts=-30)),
        ("float64", 2, 120, 512, dict(r0=900, r1=1000, n=1, thr=(3, 1), roff=300, jumps=7.5, maxts=-35)),
        ("float32", 1, 180, 300, dict(r0=450, r1=470, n=20, thr=(3, 1), roff=20, jumps=50, maxts=-35)),
    ]):
        F.append((f"f{i}", "fielding", dt, C, P, S, 100 + i, prm))
    for i, (dt, C, P, S, prm) in enumerate([
        ("float64", 1, 96, 260, dict(start_depth=300, window_meter=200, window_ping=20, percentile=25, delta_db=4,
                                     extend_ping=0, min_window=20)),
        ("float32", 2, 140, 330, dict(start_depth=220, window_meter=450, window_ping=50, percentile=25, delta_db=5,
                                      extend_ping=1, min_window=20)),
        ("float64", 3, 83, 411, dict(start_depth=500, window_meter=300, window_ping=9, percentile=60, delta_db=3,
                                     extend_ping=2, min_window=5)),
        ("float32", 1, 301, 257, dict(start_depth=100, window_meter=400, window_ping=100, percentile=10, delta_db=6,
                                      extend_ping=0, min_window=50)),
        ("float64", 2, 120, 512, dict(start_depth=700, window_meter=500, window_ping=31, percentile=50, delta_db=3.5,
                                      extend_ping=0, min_window=20)),
        ("float32", 1, 180, 300, dict(start_depth=220, window_meter=450, window_ping=40, percentile=33.3, delta_db=4.5,
                                      extend_ping=3, min_window=20)),
    ]):
        F.append((f"m{i}", "matecho", dt, C, P, S, 200 + i, prm))
    return F


def fuzz_inputs(case):
    """-> (sv (C, P, S), rng (C, S), bottom (C, P) or None) of a fuzz case."""
    from echopype_amd import synth

    tag, method, dt, C, P, S, seed, prm = case
    svs, rngs, bots = [], [], []
    for c in range(C):
        sc = synth.transient_scene(P=P, S=S, seed=seed * 10 + c, dtype=np.dtype(dt), dz=2.5 + 0.25 * c,
                                   elevated=max(4, P // 12), elevation=(2.0, 14.0), nan_frac=0.01 * (1 + seed % 4))
        svs.append(sc["Sv"])
        rngs.append(sc["depth"])
        bots.append(sc["bottom"])
    bottom = np.stack(bots) if (method == "matecho" and seed % 2 == 0) else None
    return np.stack(svs), np.stack(rngs), bottom


def fuzz_expected(case):
    """-> (valid (C, P, S), margin (C, P), compare (C, P) bool: the pings at least MARGIN from every threshold)."""
    sv, rng, bottom = fuzz_inputs(case)
    valid, margin = detect(case[1], sv, rng, bottom, **case[7])
    return valid, margin, margin >= MARGIN[case[2]]


# ---- the fixture's cases as inputs -----------------------------------------------------------------------------------
DIMS = ("channel", "ping_time", "range_sample")
_CORE_KEYS = {"fielding": ("r0", "r1", "n", "thr", "roff", "jumps", "maxts"),
              "matecho": ("start_depth", "window_meter", "window_ping", "percentile", "delta_db", "extend_ping",
                          "min_window")}


def cases(g):
    import json

    return json.loads(g["cases"].item())


def case_params(c):
    """The keyword arguments of a case as the reference got them."""
    p = dict(c["params"])
    if "thr" in p:
        p["thr"] = tuple(p["thr"])
    return p


def case_arrays(g, c):
    """-> (sv (C, P, S), rows (C, S), bottom or None)."""
    return g[c["sv"]], g[c["rows"]], (g[c["bottom"]] if "bottom" in c else None)


def case_dataset(g, c, to_data=lambda a: a):
    """The xr_lite Dataset of a case; ``to_data`` wraps every variable's array (e.g. into a device array)."""
    from echopype_amd.xr_lite import DataArray, Dataset

    sv, rows, bottom = case_arrays(g, c)
    C, P, S = sv.shape
    ds = Dataset(coords={"channel": np.array([f"chan{i + 1}" for i in range(C)]), "ping_time": np.arange(P),
                         "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(to_data(sv), DIMS, name="Sv")
    if c["rlayout"] == "cps":
        ds["depth"] = DataArray(to_data(np.ascontiguousarray(np.broadcast_to(rows[:, None, :], (C, P, S)))), DIMS)
    elif c["rlayout"] == "s":
        ds["depth"] = DataArray(to_data(rows[0]), ("range_sample",))
    else:
        ds["depth"] = DataArray(to_data(np.zeros((C, P), dtype=rows.dtype)), DIMS[:2])
    if bottom is not None:
        ds["bottom_depth"] = DataArray(to_data(bottom), tuple(c["bottom_dims"]))
    if "drop" in c:
        del ds.data_vars[c["drop"]]
    return ds


def case_oracle(g, c):
    """The oracle on a fixture case -> (valid (C, P, S), margin (C, P))."""
    sv, rows, bottom = case_arrays(g, c)
    p = case_params(c)
    kw = {k: p[k] for k in _CORE_KEYS[c["method"]] if k in p}
    if c["rlayout"] == "s":
        rows = np.broadcast_to(rows[0], (sv.shape[0], rows.shape[1]))
    if c["method"] == "matecho" and p.get("bottom_var") != "bottom_depth":
        bottom = None
    return detect(c["method"], sv, rows, bottom, **kw)
