"""The rules of targets.track_targets restated in NumPy, independent of the package: the judge of csrc/track.hip.

``track(table, params)`` -> dict of the result's variables.  ``table``: dict with ``C``, ``P`` and the columns
``channel_index``, ``ping_index``, ``target_range``, ``angle_alongship``, ``angle_athwartship``, ``TS_comp`` and
optionally ``target_ping_time`` (int64 ns).  ``margins(table, params)`` -> (gate margins, choice margins): how far every
gate quantity that decided something was from 1, and the gap between the best and the second-best cost of every
propose / accept choice that had more than one candidate."""
import numpy as np

DEFAULTS = {"max_ping_gap": 2, "missed_ping_expansion": 0.0, "weight_alongship": 30.0, "weight_athwartship": 30.0,
            "weight_range": 40.0, "weight_TS": 0.0, "weight_ping_gap": 0.0, "max_TS_difference": None, "link_rounds": 3,
            "min_targets": 3, "min_pings": 3}
TARGET_VARS = ("track_id", "x", "y", "z", "next_target")
TRACK_INTS = ("channel_index", "n_targets", "ping_first", "ping_last", "target_first", "target_last")
TRACK_FLOATS = ("TS_mean", "TS_max", "range_mean", "x_first", "y_first", "z_first", "x_last", "y_last", "z_last",
                "path_length", "displacement", "tortuosity", "delta_range")
TRACK_TIMES = ("time_first", "time_last", "duration", "speed")
CHANNEL_VARS = ("n_tracks", "n_links", "n_tracked_targets")


def positions(rng, al, at):
    u, v = np.tan(al * np.pi / 180.0), np.tan(at * np.pi / 180.0)
    z = rng / np.sqrt(1.0 + u * u + v * v)
    return z * u, z * v, z


def check_table(table):
    c, p = np.asarray(table["channel_index"], dtype=np.int64), np.asarray(table["ping_index"], dtype=np.int64)
    if ((c < 0) | (c >= table["C"]) | (p < 0) | (p >= table["P"])).any():
        raise ValueError("index out of range")
    key = c * table["P"] + p
    if (np.diff(key) < 0).any():
        raise ValueError("not ordered")


class _Pairs:
    """Rules 2 and 3 for one earlier target against an array of later ones (or the other way round)."""

    def __init__(self, table, prm, gate_margins):
        self.q = prm
        self.c = np.asarray(table["channel_index"], dtype=np.int64)
        self.p = np.asarray(table["ping_index"], dtype=np.int64)
        self.ts = np.asarray(table["TS_comp"], dtype=np.float64)
        self.x, self.y, self.z = positions(*(np.asarray(table[k], dtype=np.float64) for k in
                                             ("target_range", "angle_alongship", "angle_athwartship")))
        self.ok = ~(np.isnan(self.x) | np.isnan(self.y) | np.isnan(self.z) | np.isnan(self.ts))
        self.gm = gate_margins

    def cost(self, i, j):
        """The cost of the link i -> j, or None if the pair is not gated."""
        q = self.q
        if self.c[i] != self.c[j] or not (self.ok[i] and self.ok[j]):
            return None
        k = int(self.p[j] - self.p[i] - 1)
        if k < 0 or k > q["max_ping_gap"]:
            return None
        f = 1.0 + float(k) * q["missed_ping_expansion"] / 100.0
        d = []
        for a, g in ((self.x, "gate_alongship"), (self.y, "gate_athwartship"), (self.z, "gate_range")):
            d.append(abs(a[j] - a[i]) / (f * q[g]))
            self.gm.append(abs(d[-1] - 1.0))
            if not d[-1] <= 1.0:
                return None
        dT = 0.0
        if q["max_TS_difference"] is not None:
            dT = abs(self.ts[j] - self.ts[i]) / q["max_TS_difference"]
            self.gm.append(abs(dT - 1.0))
            if not dT <= 1.0:
                return None
        c = q["weight_alongship"] * (d[0] * d[0])
        c = c + q["weight_athwartship"] * (d[1] * d[1])
        c = c + q["weight_range"] * (d[2] * d[2])
        if q["weight_TS"] > 0:
            c = c + q["weight_TS"] * (dT * dT)
        c = c + q["weight_ping_gap"] * float(k) / float(max(q["max_ping_gap"], 1))
        return float(c)


def _choose(cands, choice_margins):
    """cands: list of (cost, row) -> the row of the least (cost, row), or -1."""
    if not cands:
        return -1
    cands = sorted(cands)
    if len(cands) > 1:
        choice_margins.append(cands[1][0] - cands[0][0])
    return cands[0][1]


def link(table, prm, gate_margins, choice_margins):
    pairs = _Pairs(table, prm, gate_margins)
    n = len(pairs.c)
    rows = {}
    for i in range(n):
        rows.setdefault((int(pairs.c[i]), int(pairs.p[i])), []).append(i)
    succ, pred = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for _ in range(prm["link_rounds"]):
        prop = np.full(n, -1, dtype=np.int64)
        for i in range(n):
            if succ[i] >= 0 or not pairs.ok[i]:
                continue
            cands = []
            for ping in range(int(pairs.p[i]) + 1, int(pairs.p[i]) + 2 + prm["max_ping_gap"]):
                for j in rows.get((int(pairs.c[i]), ping), ()):
                    if pred[j] < 0:
                        c = pairs.cost(i, j)
                        if c is not None:
                            cands.append((c, j))
            prop[i] = _choose(cands, choice_margins)
        proposers = {}
        for i in range(n):
            if prop[i] >= 0:
                proposers.setdefault(int(prop[i]), []).append(i)
        for j in range(n):
            if pred[j] >= 0 or j not in proposers:
                continue
            i = _choose([(pairs.cost(i, j), i) for i in proposers[j]], choice_margins)
            pred[j], succ[i] = i, j
    return pairs, succ, pred


def _params(params):
    return {**DEFAULTS, **params}


def margins(table, params):
    gm, cm = [], []
    link(table, _params(params), gm, cm)
    return np.asarray(gm, dtype=np.float64), np.asarray(cm, dtype=np.float64)


def track(table, params):
    prm = _params(params)
    check_table(table)
    pairs, succ, pred = link(table, prm, [], [])
    n, C = len(succ), table["C"]
    x, y, z, ts, ping = pairs.x, pairs.y, pairs.z, pairs.ts, pairs.p
    rng = np.asarray(table["target_range"], dtype=np.float64)
    track_id = np.zeros(n, dtype=np.int32)
    cols = {k: [] for k in TRACK_INTS + TRACK_FLOATS}
    for r in range(n):
        if pred[r] >= 0:
            continue
        mem = [r]
        while succ[mem[-1]] >= 0:
            mem.append(int(succ[mem[-1]]))
        f, l = mem[0], mem[-1]
        if not pairs.ok[r] or len(mem) < prm["min_targets"] or ping[l] - ping[f] + 1 < prm["min_pings"]:
            continue
        track_id[mem] = len(cols["n_targets"]) + 1
        lin = 0.0
        for m in mem:
            lin += 10.0 ** (ts[m] / 10.0)
        path = 0.0
        for a, b in zip(mem[:-1], mem[1:]):
            path += np.sqrt((x[b] - x[a]) ** 2 + (y[b] - y[a]) ** 2 + (z[b] - z[a]) ** 2)
        disp = np.sqrt((x[l] - x[f]) ** 2 + (y[l] - y[f]) ** 2 + (z[l] - z[f]) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            tort = np.float64(path) / np.float64(disp)
        for k, v in (("channel_index", pairs.c[f]), ("n_targets", len(mem)), ("ping_first", ping[f]),
                     ("ping_last", ping[l]), ("target_first", f), ("target_last", l),
                     ("TS_mean", 10.0 * np.log10(lin / len(mem))), ("TS_max", max(ts[m] for m in mem)),
                     ("range_mean", sum(rng[m] for m in mem) / len(mem)), ("x_first", x[f]), ("y_first", y[f]),
                     ("z_first", z[f]), ("x_last", x[l]), ("y_last", y[l]), ("z_last", z[l]), ("path_length", path),
                     ("displacement", disp), ("tortuosity", tort), ("delta_range", z[l] - z[f])):
            cols[k].append(v)
    out = {"track_id": track_id, "x": x, "y": y, "z": z, "next_target": succ.astype(np.int32)}
    for k in TRACK_INTS:
        out[k] = np.asarray(cols[k], dtype=np.int32)
    for k in TRACK_FLOATS:
        out[k] = np.asarray(cols[k], dtype=np.float64)
    if "target_ping_time" in table:
        t = np.asarray(table["target_ping_time"], dtype=np.int64)
        out["time_first"], out["time_last"] = t[out["target_first"]], t[out["target_last"]]
        out["duration"] = (out["time_last"] - out["time_first"]).astype(np.float64) / 1e9
        with np.errstate(divide="ignore", invalid="ignore"):
            out["speed"] = out["path_length"] / out["duration"]
    chan = np.asarray(table["channel_index"], dtype=np.int64)
    out["n_tracks"] = np.bincount(out["channel_index"], minlength=C).astype(np.int64)
    out["n_links"] = np.bincount(chan[succ >= 0], minlength=C).astype(np.int64)
    out["n_tracked_targets"] = np.bincount(chan[track_id > 0], minlength=C).astype(np.int64)
    return out
