"""The single-target detection rules (split beam) as plain NumPy loops in float64: the judge of
``targets.detect_single_targets``.  Independent of the package: nothing here imports it.  The rules are the ones the
function's docstring states (this project's restatement of the Echoview method; never run against Echoview):

1. candidate: TS[s] >= TS_threshold, the left neighbour absent or not >= TS[s], the right neighbour absent or not > TS[s];
2. envelope [l, r] at L = TS[s] - pldl (NaN and the row ends stop the walk), n = r - l + 1, npl = n / spp;
   rule 1 rejects unless spp > 0 and min <= npl <= max;
3. rule 2 rejects if any TS[k] > TS[s] inside the envelope;
4. a, b the means of the angles over the envelope, x = 2 (a - off_al) / bw_al, y likewise,
   B = 6.0206 (x^2 + y^2 - 0.18 x^2 y^2); rule 3 rejects unless B <= max_beam_compensation; TS_comp = TS[s] + B;
5. rule 4 rejects unless both population standard deviations of the angles over the envelope are <= their limits;
6. target_range = sum(w r) / sum(w), w = 10^(TS / 10), over the samples of the envelope whose range is not NaN."""
import numpy as np

ICOLS = ("channel_index", "ping_index", "range_sample", "sample_first", "sample_last")
FCOLS = ("TS_uncomp", "TS_comp", "beam_compensation", "target_range", "angle_alongship", "angle_athwartship",
         "std_angle_alongship", "std_angle_athwartship", "normalized_pulse_length")
DEFAULTS = {"TS_threshold": -50.0, "pldl": 6.0, "min_norm_pulse_length": 0.7, "max_norm_pulse_length": 1.5,
            "max_beam_compensation": 4.0, "max_std_alongship": 0.6, "max_std_athwartship": 0.6}


def candidates(ts, thr):
    """Indices of the candidates of one row (rule 1 of the list above)."""
    S = len(ts)
    out = []
    for s in range(S):
        v = ts[s]
        if not v >= thr:
            continue
        if s > 0 and ts[s - 1] >= v:
            continue
        if s < S - 1 and ts[s + 1] > v:
            continue
        out.append(s)
    return out


def envelope(ts, s, pldl):
    S = len(ts)
    L = ts[s] - pldl
    l = r = s
    while l > 0 and ts[l - 1] >= L:
        l -= 1
    while r < S - 1 and ts[r + 1] >= L:
        r += 1
    return l, r


def detect_row(ts, al, at, rng, spp, bw_al, bw_at, off_al, off_at, prm):
    """One row -> (targets: list of dicts, n_candidates, rejected[4], margins: list of (rule, distance) for every
    candidate decided by rule 3 or 4 -- the distances of B and of both standard deviations from their limits, as far
    as they were looked at; a NaN B has no distance and is left out)."""
    ts = np.asarray(ts, dtype=np.float64)
    al = np.asarray(al, dtype=np.float64)
    at = np.asarray(at, dtype=np.float64)
    rng = np.asarray(rng, dtype=np.float64)
    spp = float(spp)
    targets, rejected, margins = [], [0, 0, 0, 0], []
    cands = candidates(ts, prm["TS_threshold"])
    for s in cands:
        v = ts[s]
        l, r = envelope(ts, s, prm["pldl"])
        n = r - l + 1
        with np.errstate(divide="ignore", invalid="ignore"):
            npl = np.float64(n) / np.float64(spp)
        if not (spp > 0 and npl >= prm["min_norm_pulse_length"] and npl <= prm["max_norm_pulse_length"]):
            rejected[0] += 1
            continue
        if np.any(ts[l:r + 1] > v):
            rejected[1] += 1
            continue
        a = al[l:r + 1].sum() / n
        b = at[l:r + 1].sum() / n
        x = 2.0 * (a - off_al) / bw_al
        y = 2.0 * (b - off_at) / bw_at
        B = 6.0206 * (x * x + y * y - 0.18 * x * x * y * y)
        if B == B:  # (a NaN B is rejected for being NaN, on the device as here: no rounding can change that)
            margins.append((3, abs(B - prm["max_beam_compensation"])))
        if not B <= prm["max_beam_compensation"]:
            rejected[2] += 1
            continue
        sa = np.sqrt(((al[l:r + 1] - a) ** 2).sum() / n)
        sb = np.sqrt(((at[l:r + 1] - b) ** 2).sum() / n)
        margins.append((4, abs(sa - prm["max_std_alongship"])))
        margins.append((4, abs(sb - prm["max_std_athwartship"])))
        if not (sa <= prm["max_std_alongship"] and sb <= prm["max_std_athwartship"]):
            rejected[3] += 1
            continue
        rr = rng[l:r + 1]
        ok = ~np.isnan(rr)
        w = 10.0 ** (ts[l:r + 1][ok] / 10.0)
        t_range = (w * rr[ok]).sum() / w.sum() if ok.any() else np.nan
        targets.append({"range_sample": s, "sample_first": l, "sample_last": r, "TS_uncomp": v, "TS_comp": v + B,
                        "beam_compensation": B, "target_range": t_range, "angle_alongship": a, "angle_athwartship": b,
                        "std_angle_alongship": sa, "std_angle_athwartship": sb, "normalized_pulse_length": npl})
    return targets, len(cands), rejected, margins


def _cp(v, C, P):
    return np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(np.shape(v) + (1,) * (2 - np.ndim(v))), (C, P))


def detect(ts, al, at, rng, spp, bw_al, bw_at, off_al, off_at, prm):
    """(C, P, S) cubes, ``rng`` broadcasting to them, the parameters scalars, (C,) or (C, P) -> dict: the table columns
    (ordered by channel, ping, sample), ``n_targets`` (C, P), ``n_candidates`` (C,), ``n_rejected`` (C, 4),
    ``margins`` (the list of (rule, distance) of ``detect_row`` over all rows)."""
    ts = np.asarray(ts)
    C, P, S = ts.shape
    rng = np.broadcast_to(np.asarray(rng), (C, P, S))
    q = [_cp(v, C, P) for v in (spp, bw_al, bw_at, off_al, off_at)]
    cols = {k: [] for k in ICOLS + FCOLS}
    n_targets = np.zeros((C, P), dtype=np.int32)
    n_cand = np.zeros(C, dtype=np.int64)
    n_rej = np.zeros((C, 4), dtype=np.int64)
    margins = []
    for c in range(C):
        for p in range(P):
            tg, nc, rej, mg = detect_row(ts[c, p], al[c, p], at[c, p], rng[c, p], *(v[c, p] for v in q), prm)
            n_targets[c, p] = len(tg)
            n_cand[c] += nc
            n_rej[c] += rej
            margins += mg
            for t in tg:
                cols["channel_index"].append(c)
                cols["ping_index"].append(p)
                for k, v in t.items():
                    cols[k].append(v)
    out = {k: np.asarray(cols[k], dtype=np.int32) for k in ICOLS}
    out.update({k: np.asarray(cols[k], dtype=np.float64) for k in FCOLS})
    out.update(n_targets=n_targets, n_candidates=n_cand, n_rejected=n_rej, margins=margins)
    return out
