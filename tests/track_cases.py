"""Hand-made target tables for targets.track_targets, with exactly representable values where ties are wanted: no detector
run is needed.  ``CASES``: name -> (table, params, planted ties); ``expected(name)`` is the restatement's answer,
computed once.  ``BAD``: tables that must raise ``ValueError``.

A table is built from rows (channel, ping, range, alongship, athwartship, TS); ``table()`` orders them by (channel,
ping), keeping the order given within a ping.  Most fish swim along the beam axis (angles 0: x = y = 0 and z = range,
exactly), ``lanes()`` spreads many of them over range, 0.5 m apart with gates of 0.1 m."""
import functools

import numpy as np
import track_ref as R

NAN = float("nan")
TILE = 128  # EPA_TRACK_TILE: the rows of a run a workgroup stages at a time
T0 = np.datetime64("2026-10-20T00:00:00", "ns").astype(np.int64)
GATES = {"gate_alongship": 0.1, "gate_athwartship": 0.1, "gate_range": 0.1}
LOOSE = {**GATES, "min_targets": 2, "min_pings": 2}


def table(C, P, rows, time=True):
    rows = sorted(rows, key=lambda r: (r[0], r[1]))  # (stable)
    a = np.asarray(rows, dtype=np.float64).reshape(len(rows), 6)
    t = {"C": C, "P": P, "channel_index": a[:, 0].astype(np.int32), "ping_index": a[:, 1].astype(np.int32),
         "target_range": a[:, 2].copy(), "angle_alongship": a[:, 3].copy(), "angle_athwartship": a[:, 4].copy(),
         "TS_comp": a[:, 5].copy()}
    if time:
        t["target_ping_time"] = T0 + t["ping_index"].astype(np.int64) * 1_000_000_000
    return t


def lane_row(c, p, k):
    """Fish k of channel c at ping p: its own range lane, a drift of a centimetre per ping and a jitter below a
    millimetre that no two pings share; a fixed direction per fish; a TS of its own."""
    r = 5.0 + 0.5 * k + 0.01 * p + 0.001 * ((k * 7 + p * 3) % 11) / 11.0
    return (c, p, r, 0.1 * (k % 5 - 2), 0.05 * (k % 3 - 1), -50.0 + 0.25 * (k % 17) + 0.125 * (p % 3))


def lanes(counts, C=1, extra_pings=1):
    """Per ping p the fish 0 .. counts[p] - 1, in every channel."""
    P = len(counts) + extra_pings
    return table(C, P, [lane_row(c, p, k) for c in range(C) for p, m in enumerate(counts) for k in range(m)])


def axis(c, p, r, ts=-45.0):
    return (c, p, r, 0.0, 0.0, ts)


def _counts():
    # 0, 1, 2, a wave less one / exactly / plus one, a tile less one / exactly / plus one; an empty ping inside windows;
    # the last pings' windows are clipped at the channel's end (no spare ping)
    return lanes([1, 2, 0, 63, 64, 65, TILE - 1, TILE, TILE + 1, TILE + 1, 0, TILE, 65, 2], extra_pings=0)


def _two_channels():
    # the last ping of channel 0 and the first ping of channel 1 hold targets at one position (adjoining rows): no link
    rows = [axis(0, p, 10.0 + 0.01 * p) for p in (1, 2, 3)] + [axis(0, 3, 12.0)]
    rows += [axis(1, 0, 12.0), axis(1, 1, 12.03), axis(1, 2, 12.04)] + [axis(1, p, 10.04 + 0.01 * p) for p in (0, 1, 2)]
    return table(2, 4, rows)


def _gap():
    rows = [axis(0, p, 10.0 + 0.01 * p) for p in (0, 1, 4)]        # a gap of exactly max_ping_gap: links
    rows += [axis(0, p, 12.0 + 0.01 * p) for p in (0, 1, 5)]       # one more: does not
    return table(1, 7, rows)


def _expansion():
    # ping 0 -> ping 2 (one ping missed), 0.11 m apart in range: outside the gate of 0.1 m, inside 1.2 x 0.1 m
    return table(1, 4, [axis(0, 0, 10.0), axis(0, 2, 10.11), axis(0, 3, 10.13)])


def _ts_gate():
    # the nearest successor differs by 8 dB, the second nearest by 1 dB
    rows = [axis(0, 0, 10.0, -40.0), axis(0, 1, 10.01, -48.0), axis(0, 1, 10.06, -41.0), axis(0, 2, 10.03, -47.5),
            axis(0, 2, 10.08, -41.5)]
    return table(1, 3, rows)


def _nan():
    rows = []
    for k, col in enumerate((2, 3, 4, 5)):  # a fish per column; its ping-2 echo holds a NaN there
        for p in range(5):
            row = list(lane_row(0, p, k))
            if p == 2:
                row[col] = NAN
            rows.append(tuple(row))
    rows.append((0, 4, NAN, 0.0, 0.0, -40.0))
    rows.append(axis(0, 0, 30.0))  # alone, and whole
    return table(1, 5, rows)


def _contention():
    # A and B (ping 0) both want J (ping 1); J takes A; B's second choice is K, which A cannot reach
    return table(1, 2, [axis(0, 0, 10.0), axis(0, 0, 10.06), axis(0, 1, 10.02), axis(0, 1, 10.12)])


def _mirror():
    # channel 0: one target, two mirrored successors at +-1 degree and equal range: bit-equal costs, the lower row wins
    # channel 1: two mirrored targets propose to one successor on the axis: bit-equal costs, the lower row is accepted
    rows = [(0, 0, 10.0, 0.0, 0.0, -45.0), (0, 1, 10.0, 0.0, 0.5, -45.0), (0, 1, 10.0, 0.0, -0.5, -45.0),
            (1, 0, 20.0, 0.25, 0.0, -45.0), (1, 0, 20.0, -0.25, 0.0, -45.0), (1, 1, 20.0, 0.0, 0.0, -45.0)]
    return table(2, 2, rows)


def _chains():
    # chains of 1, 2, 3, 32 and 33 targets among 33 pings: every doubling pass is needed
    rows = []
    for k, (first, m) in enumerate(((5, 1), (7, 2), (9, 3), (1, 32), (0, 33))):
        rows += [lane_row(0, p, k) for p in range(first, first + m)]
    return table(1, 33, rows)


def _min_rules():
    rows = [axis(0, p, 10.0 + 0.01 * p) for p in (0, 1, 2)]          # 3 targets over 3 pings: min_pings = 4 rejects
    rows += [axis(0, p, 12.0 + 0.01 * p) for p in (0, 3)]            # 2 targets over 4 pings: min_targets = 3 rejects
    rows += [axis(0, p, 14.0 + 0.01 * p) for p in (0, 1, 2, 3)]      # kept by both
    return table(1, 4, rows)


def _nothing():
    return table(2, 3, [axis(c, p, 10.0 + 3.0 * p + c) for c in range(2) for p in range(3)])


def _dropped():
    t = lanes([5, 6, 7, 7, 6, 5, 7, 7], C=2)
    keep = np.arange(len(t["channel_index"])) % 5 != 3
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def _crossing():
    # two fish whose ranges cross between pings 2 and 3, apart in alongship angle
    a = [(0, p, 10.0 + 0.02 * p, 0.0, 0.0, -45.0) for p in range(6)]
    b = [(0, p, 10.1 - 0.02 * p, 1.0, 0.0, -42.0) for p in range(6)]
    return table(1, 6, [r for pair in zip(a, b) for r in pair])


def _no_time():
    return table(1, 4, [lane_row(0, p, k) for p in range(4) for k in range(3)], time=False)


CASES = {
    "counts": (_counts(), GATES, 0),
    "counts_ping_gap_weight": (_counts(), {**GATES, "weight_ping_gap": 5.0, "max_ping_gap": 3}, 0),
    "two_channels": (_two_channels(), GATES, 0),
    "gap": (_gap(), LOOSE, 0),
    "expansion_off": (_expansion(), LOOSE, 0),
    "expansion_on": (_expansion(), {**LOOSE, "missed_ping_expansion": 20.0}, 0),
    "ts_gate_off": (_ts_gate(), GATES, 0),
    "ts_gate_on": (_ts_gate(), {**GATES, "max_TS_difference": 6.0}, 0),
    "ts_weight": (_ts_gate(), {**GATES, "max_TS_difference": 10.0, "weight_TS": 500.0}, 0),
    "nan": (_nan(), GATES, 0),
    "nan_lone_targets": (_nan(), {**GATES, "min_targets": 1, "min_pings": 1}, 0),
    "contention_1": (_contention(), {**LOOSE, "link_rounds": 1}, 0),
    "contention_3": (_contention(), {**LOOSE, "link_rounds": 3}, 0),
    "mirror": (_mirror(), LOOSE, 2),
    "chains": (_chains(), GATES, 0),
    "min_rules": (_min_rules(), {**GATES, "min_targets": 3, "min_pings": 4}, 0),
    "crossing": (_crossing(), GATES, 0),
    "nothing": (_nothing(), GATES, 0),
    "empty": (table(2, 3, []), GATES, 0),
    "dropped": (_dropped(), GATES, 0),
    "no_time": (_no_time(), GATES, 0),
}


def _bad(t, **change):
    return {**t, **{k: np.asarray(v, dtype=t[k].dtype) for k, v in change.items()}}


_SMALL = table(2, 3, [axis(c, p, 10.0 + 0.01 * p) for c in range(2) for p in range(3)])
BAD = {
    "pings_unordered": _bad(_SMALL, ping_index=[0, 2, 1, 0, 1, 2]),
    "channels_unordered": _bad(_SMALL, channel_index=[0, 0, 1, 0, 1, 1]),
    "channel_too_large": _bad(_SMALL, channel_index=[0, 0, 0, 1, 1, 2]),
    "ping_too_large": _bad(_SMALL, ping_index=[0, 1, 2, 0, 1, 3]),
    "ping_negative": _bad(_SMALL, ping_index=[-1, 1, 2, 0, 1, 2]),
    "channel_negative": _bad(_SMALL, channel_index=[-1, 0, 0, 1, 1, 1]),
}


@functools.lru_cache(maxsize=None)
def expected(name):
    t, prm, _ = CASES[name]
    return R.track(t, prm)


@functools.lru_cache(maxsize=None)
def case_margins(name):
    t, prm, _ = CASES[name]
    return R.margins(t, prm)
