#!/usr/bin/env python3
"""``targets.track_targets`` at a survey's size: a target table of one channel x 200 000 pings generated on the device,
about six targets per ping: five drifting fish (a random walk of half a centimetre per ping in range, lanes 10 m apart,
each echo detected with probability 0.9) and clutter (two slots per ping, each filled with probability 0.75, anywhere
in the beam).  Gates of 0.1 m, the default weights, ``max_ping_gap`` 2, three link rounds.

In one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup`` warm-up runs,
by device events around the calls of the wrappers, the groups alternating so that they see the same machine:

1. ``prepare``: positions, segment starts, verdict (1 launch);
2. ``link_rounds``: three rounds of propose + accept (6 launches);
3. ``roots``: pointer doubling, ``ceil(log2(P))`` passes (18 launches at 200 000 pings);
4. ``chains``: the flag and length per track (1 launch), and next to it ``scans_torch_cumsum``, the two torch scans;
5. ``table``: track numbers, the members in chain order, one wave per track (2 launches);
6. the gating test alone as a dense torch expression over the same windows -- the targets padded to 7 slots per ping,
   every slot against every slot of the next three pings, three comparisons and an ``&`` -- the only fair floor there
   is: it links nothing, chooses nothing and builds no track.

The whole ``track_targets`` call (all of the above, the one synchronisation, the time columns and per-channel counts;
host clock ended by a synchronise) is timed next to them.  Writes the JSON document to ``--out`` (default
profiles/track_bench.json) and prints it."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import echopype_amd as ep  # noqa: E402
from echopype_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pings", type=int, default=200_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_track.py needs a GPU: a time taken elsewhere says nothing")
P, REPS, WARM = args.pings, args.reps, args.warmup
FISH, CLUTTER, SLOTS = 5, 2, 7
PRM = {"gate_alongship": 0.1, "gate_athwartship": 0.1, "gate_range": 0.1}
FULL = {**ep.targets.track.DEFAULTS, **PRM}
GATES = [0.0 if FULL[k] is None else float(FULL[k]) for k in _lib.TRACK_PARAM_NAMES]
ROUNDS, GAP = FULL["link_rounds"], FULL["max_ping_gap"]
logging.disable(logging.WARNING)
dev = torch.device("cuda", 0)


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def scene():
    """The table's columns on the device, ordered by ping, and the same targets padded to (P, SLOTS) with NaN."""
    g = torch.Generator(device=dev).manual_seed(20261020)
    f64 = dict(dtype=torch.float64, device=dev)
    rng = torch.empty((P, SLOTS), **f64)
    al, at, ts = torch.empty_like(rng), torch.empty_like(rng), torch.empty_like(rng)
    base = 10.0 + 10.0 * torch.arange(FISH, **f64)
    rng[:, :FISH] = base[None, :] + torch.cumsum(0.005 * torch.randn((P, FISH), generator=g, **f64), 0)
    al[:, :FISH] = (torch.arange(FISH, **f64) - 2.0)[None, :] + 0.02 * torch.randn((P, FISH), generator=g, **f64)
    at[:, :FISH] = (2.0 - torch.arange(FISH, **f64))[None, :] * 0.5 + 0.02 * torch.randn((P, FISH), generator=g, **f64)
    ts[:, :FISH] = -45.0 + torch.randn((P, FISH), generator=g, **f64)
    rng[:, FISH:] = 5.0 + 55.0 * torch.rand((P, CLUTTER), generator=g, **f64)
    al[:, FISH:] = 7.0 * torch.rand((P, CLUTTER), generator=g, **f64) - 3.5
    at[:, FISH:] = 7.0 * torch.rand((P, CLUTTER), generator=g, **f64) - 3.5
    ts[:, FISH:] = -55.0 + 5.0 * torch.randn((P, CLUTTER), generator=g, **f64)
    seen = torch.rand((P, SLOTS), generator=g, device=dev)
    seen = torch.cat([seen[:, :FISH] < 0.9, seen[:, FISH:] < 0.75], 1)
    ping = torch.arange(P, dtype=torch.int32, device=dev)[:, None].expand(P, SLOTS)
    cols = {"ping_index": ping[seen].contiguous(), "target_range": rng[seen], "angle_alongship": al[seen],
            "angle_athwartship": at[seen], "TS_comp": ts[seen]}
    cols["channel_index"] = torch.zeros_like(cols["ping_index"])
    nan = torch.full_like(rng, float("nan"))
    padded = [torch.where(seen, v, nan) for v in (rng, al, at)]
    return cols, padded, int(seen[:, :FISH].sum())


cols, padded, n_fish_echoes = scene()
ci, pi = cols["channel_index"], cols["ping_index"]
rng, al, at, ts = (cols[k] for k in ("target_range", "angle_alongship", "angle_athwartship", "TS_comp"))
n = ci.numel()
PASSES = (max(P, 2) - 1).bit_length()


def link_rounds(seg, xyz, succ, pred, prop):
    succ.fill_(-1)
    pred.fill_(-1)
    for _ in range(ROUNDS):
        ops.track_link_round(ci, pi, xyz, ts, 1, P, seg, GATES, succ, pred, prop)


def chains(xyz, succ, root, rank):
    return ops.track_chains(pi, xyz, ts, succ, root, rank, FULL["min_targets"], FULL["min_pings"])


def scan(flag_len):
    return torch.stack([torch.cumsum(row, 0, dtype=torch.int64) for row in flag_len])


def torch_gates():
    """The gate of every padded slot against every slot of the next 1 + GAP pings (no expansion: f = 1)."""
    u, v = torch.tan(padded[1] * (np.pi / 180.0)), torch.tan(padded[2] * (np.pi / 180.0))
    z = padded[0] / torch.sqrt(1.0 + u * u + v * v)
    x, y = z * u, z * v
    out = []
    for k in range(1, GAP + 2):
        ok = torch.ones((P - k, SLOTS, SLOTS), dtype=torch.bool, device=dev)
        for a, gate in ((x, PRM["gate_alongship"]), (y, PRM["gate_athwartship"]), (z, PRM["gate_range"])):
            ok &= (a[k:, None, :] - a[:-k, :, None]).abs() / gate <= 1.0
        out.append(ok)
    return out


with _lib.launch_trace() as tr:
    seg, xyz, succ, pred, bad = ops.track_prepare(ci, pi, rng, al, at, 1, P)
    prop = torch.empty(n, dtype=torch.int32, device=dev)
    link_rounds(seg, xyz, succ, pred, prop)
    root, rank = ops.track_roots(pred, PASSES)
    flag_len = chains(xyz, succ, root, rank)
    scans = scan(flag_len)
    T, M = int(scans[0, -1]), int(scans[1, -1])
    track_id, icols, fcols = ops.track_table(ci, pi, rng, ts, xyz, root, rank, flag_len, scans, T, M)
launches = {"prepare": 1, "link_rounds": 2 * ROUNDS, "roots": PASSES, "chains": 1, "table": 2}
assert len(tr.kernels) == sum(launches.values()) and int(bad[0]) == 0, tr.kernels
gated_pairs = int(sum(int(g.sum()) for g in torch_gates()))

routes = {
    "prepare": lambda: ops.track_prepare(ci, pi, rng, al, at, 1, P),
    "link_rounds": lambda: link_rounds(seg, xyz, succ, pred, prop),
    "roots": lambda: ops.track_roots(pred, PASSES),
    "chains": lambda: chains(xyz, succ, root, rank),
    "scans_torch_cumsum": lambda: scan(flag_len),
    "table": lambda: ops.track_table(ci, pi, rng, ts, xyz, root, rank, flag_len, scans, T, M),
    "torch_gate_expression": torch_gates,
}
times = {k: [] for k in routes}
for i in range(WARM + REPS):
    for k, f in routes.items():
        ms, out = event_timed(f)
        del out
        if i >= WARM:
            times[k].append(ms)

ds = ep.Dataset(coords={"channel": ["chan1"], "ping_time": np.arange(P)})
for k, t in cols.items():
    ds[k] = ep.DataArray(ep.DeviceArray(t), ("target",), name=k)
t_api = [host_timed(lambda: ep.targets.track_targets(ds, "gated_nearest", PRM))[0] for _ in range(WARM + 7)][WARM:]
out = ep.targets.track_targets(ds, "gated_nearest", PRM)
assert np.array_equal(out["track_id"].values, track_id.cpu().numpy())

res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": 1, "pings": P, "targets": n, "targets_per_ping": n / P, "fish": FISH,
                    "fish_echoes": n_fish_echoes, "params": {k: FULL[k] for k in FULL}},
       "result": {"tracks": T, "targets_in_tracks": M, "links": int((succ >= 0).sum()),
                  "longest_track": int(icols[1].max()) if T else 0, "gated_pairs_of_the_torch_expression": gated_pairs},
       "tuning": "untuned, a single run: one wave per (channel, ping) segment in propose / accept, runs staged in LDS "
                 "tiles of %d rows; one launch per doubling pass" % ops.TRACK_TILE,
       "timing": f"device events around the calls, median of {REPS} after {WARM} warm-ups, the groups alternating"}
kernel_ms = 0.0
for k in routes:
    res[k] = summary(times[k])
    if k in launches:
        res[k]["launches"] = launches[k]
        res[k]["ms_per_launch_median"] = res[k]["ms_median"] / launches[k]
    if k != "torch_gate_expression":
        kernel_ms += res[k]["ms_median"]
res["all_groups_and_scans_ms_median_sum"] = kernel_ms
res["launches_per_call"] = sum(launches.values())
res["torch_gate_expression_over_link_rounds_time_ratio_median"] = \
    res["torch_gate_expression"]["ms_median"] / res["link_rounds"]["ms_median"]
res["track_targets_whole_call_host_clock"] = summary(t_api)

doc = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
