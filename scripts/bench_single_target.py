#!/usr/bin/env python3
"""``targets.detect_single_targets`` at a survey's size: one channel x 200 000 pings x 2500 samples of TS with the two
angle cubes, float32 and float64, generated on the device: a noise floor around -75 dB with six echoes per ping,
parabolic in dB, planted one to a sixth of the row (about five of them pass the rules); ``spp`` = 4, the range as a
(range_sample,) vector.

Per dtype, in one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup``
warm-up runs, by device events around the call of the wrapper, the three alternating so that they see the same machine:

1. the count pass (``ops.single_target_count``: TS read once, 4 B per ping written);
2. the emit pass (``ops.single_target_emit``: TS read once more, 92 B per target written);
3. the candidate test alone as a torch expression on the device, ``(ts >= thr) & local maximum``: a floor that does
   less work (no envelope, no rule, no table) -- and may well be faster.

Bytes counted: one read of TS per pass plus the rows written (the angles and the range, read at the envelopes of a few
candidates only, are left out), against 8 TB/s.  The whole ``detect_single_targets`` call (both passes, the scan, the
one synchronisation and the gather of the ping times; host clock ended by a synchronise) is timed next to them.
Writes the JSON document to ``--out`` (default profiles/single_target_bench.json) and prints it."""
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
ap.add_argument("--samples", type=int, default=2500)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_target_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_single_target.py needs a GPU: a time taken elsewhere says nothing")
P, S, REPS, WARM = args.pings, args.samples, args.reps, args.warmup
HBM_PEAK = 8.0e12
ECHOES = 6
PRM = {"TS_threshold": -50.0, "pldl": 6.0, "min_norm_pulse_length": 0.7, "max_norm_pulse_length": 1.5,
       "max_beam_compensation": 4.0, "max_std_alongship": 0.6, "max_std_athwartship": 0.6}
LIMITS = [PRM[k] for k in _lib.SINGLE_TARGET_LIMITS]
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


def scene(tdt):
    """(1, P, S) TS and angle cubes of ``tdt`` on the device: the floor in chunks of pings, then the echoes."""
    g = torch.Generator(device=dev).manual_seed(20261020)
    ts = torch.empty((1, P, S), dtype=tdt, device=dev)
    al, at = torch.empty_like(ts), torch.empty_like(ts)
    step = 20_000
    for p0 in range(0, P, step):
        n = min(step, P - p0)
        ts[0, p0:p0 + n] = -75.0 + 3.0 * torch.randn((n, S), generator=g, device=dev, dtype=torch.float32)
        al[0, p0:p0 + n] = 10.0 * torch.rand((n, S), generator=g, device=dev, dtype=torch.float32) - 5.0
        at[0, p0:p0 + n] = 10.0 * torch.rand((n, S), generator=g, device=dev, dtype=torch.float32) - 5.0
    width = S // ECHOES
    rows = torch.arange(P, device=dev)[:, None].expand(P, ECHOES)
    centre = (torch.arange(ECHOES, device=dev) * width)[None, :] + 8 + \
        torch.randint(0, max(width - 16, 1), (P, ECHOES), generator=g, device=dev)
    peak = -45.0 + 13.0 * torch.rand((P, ECHOES), generator=g, device=dev)
    half = 1.2 + 1.3 * torch.rand((P, ECHOES), generator=g, device=dev)      # 6 dB down at 1.2 .. 2.5 samples
    frac = torch.rand((P, ECHOES), generator=g, device=dev) - 0.5
    rad = 2.6 * torch.rand((P, ECHOES), generator=g, device=dev)
    phi = 2.0 * np.pi * torch.rand((P, ECHOES), generator=g, device=dev)
    for j in range(-5, 6):
        cols = (centre + j).clamp_(0, S - 1)
        ts[0, rows, cols] = (peak - 6.0 * ((j - frac) / half) ** 2).to(tdt)
        al[0, rows, cols] = (rad * torch.cos(phi) + 0.05 * torch.randn((P, ECHOES), generator=g, device=dev)).to(tdt)
        at[0, rows, cols] = (rad * torch.sin(phi) + 0.05 * torch.randn((P, ECHOES), generator=g, device=dev)).to(tdt)
    return ts, al, at


res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": 1, "pings": P, "range_samples": S, "echoes_planted_per_ping": ECHOES, "spp": 4.0,
                    "range": "(range_sample,) vector", "params": PRM},
       "tuning": "untuned, a single run: one workgroup per row, tiles of %d samples in LDS" % ops.SINGLE_TARGET_TILE,
       "bytes_counted": "TS read once per pass + what the pass writes (4 B per ping; 92 B per target)",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, the three alternating"}

for dtype in ("float32", "float64"):
    tdt = torch.float32 if dtype == "float32" else torch.float64
    ts, al, at = scene(tdt)
    rng = (0.2 * torch.arange(S, device=dev, dtype=torch.float64)).to(tdt)
    r_b = rng[None, None, :]
    prm = torch.stack([torch.full((1, P), v, dtype=torch.float64, device=dev) for v in (4.0, 7.0, 7.0, 0.0, 0.0)]).contiguous()
    n_targets, n_cand, n_rej = ops.single_target_count(ts, al, at, r_b, prm, LIMITS)
    flat = n_targets.reshape(-1).to(torch.int64)
    incl = torch.cumsum(flat, 0)
    offsets, n = (incl - flat).reshape(1, P), int(incl[-1])
    thr = PRM["TS_threshold"]

    def torch_candidates():
        x = ts[0]
        c = x >= thr
        c[:, 1:] &= ~(x[:, :-1] >= x[:, 1:])
        c[:, :-1] &= ~(x[:, 1:] > x[:, :-1])
        return c

    routes = {
        "count_pass": lambda: ops.single_target_count(ts, al, at, r_b, prm, LIMITS),
        "emit_pass": lambda: ops.single_target_emit(ts, al, at, r_b, prm, LIMITS, n_targets, offsets, n),
        "torch_candidate_expression": torch_candidates,
    }
    with _lib.launch_trace() as tr:
        got = {k: f() for k, f in routes.items()}
    assert tr.kernels == ["single_target_count_kernel", "single_target_emit_kernel"], tr.kernels
    # the torch expression finds the candidates the count pass counted
    assert int(got["torch_candidate_expression"].sum()) == int(n_cand.sum())
    del got
    times = {k: [] for k in routes}
    for i in range(WARM + REPS):
        for k, f in routes.items():
            ms, out = event_timed(f)
            del out
            if i >= WARM:
                times[k].append(ms)
    ds = ep.Dataset(coords={"channel": ["chan1"], "ping_time": np.arange(P), "range_sample": np.arange(S)})
    dims = ("channel", "ping_time", "range_sample")
    for k, t in (("TS", ts), ("angle_alongship", al), ("angle_athwartship", at)):
        ds[k] = ep.DataArray(ep.DeviceArray(t), dims, name=k)
    ds["echo_range"] = ep.DataArray(ep.DeviceArray(rng), ("range_sample",))
    for k, v in (("beamwidth_alongship", 7.0), ("beamwidth_athwartship", 7.0), ("angle_offset_alongship", 0.0),
                 ("angle_offset_athwartship", 0.0)):
        ds[k] = (("channel",), np.array([v]))
    api = lambda: ep.targets.detect_single_targets(ds, "split_beam", {**PRM, "pulse_length_samples": 4.0})  # noqa: E731
    t_api = [host_timed(api)[0] for _ in range(WARM + 7)][WARM:]
    item = ts.element_size()
    need = {"count_pass": P * S * item + 4 * P, "emit_pass": P * S * item + 92 * n,
            "torch_candidate_expression": P * S * (item + 1)}
    doc = {"targets": n, "targets_per_ping": n / P, "candidates": int(n_cand.sum()),
           "rejected_by_rule_1_to_4": [int(v) for v in n_rej[0].tolist()]}
    for k in routes:
        s = summary(times[k])
        rate = need[k] / (s["ms_median"] * 1e-3)
        doc[k] = {**s, "bytes_needed": need[k], "TB_per_s_median": rate / 1e12, "fraction_of_8_TB_per_s": rate / HBM_PEAK}
    doc["torch_candidate_expression_over_count_pass_time_ratio_median"] = \
        doc["torch_candidate_expression"]["ms_median"] / doc["count_pass"]["ms_median"]
    doc["detect_single_targets_whole_call_host_clock"] = summary(t_api)
    res[f"TS_{dtype}"] = doc
    del ts, al, at, ds, routes, api, n_targets, offsets, prm

out = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out + "\n")
print(out)
