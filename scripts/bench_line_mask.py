#!/usr/bin/env python3
"""``mask.line_mask`` at a survey's size: EK60, 4 channels x 100 000 pings x 2000 samples, ``depth`` from
``compute_Sv -> add_depth(depth_offset, tilt)`` in float32 and in float64, both bounds given as (channel, ping_time)
lines on the device (the lower one NaN in one ping of a hundred, as a bottom line is).

Per dtype, in one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup``
warm-up runs, by device events around the call of the wrapper, the three alternating so that they see the same machine:

1. the array route: ``epa_line_mask`` reading the written ``depth`` (4 or 8 B per sample read, 1 B written);
2. the lazy route: ``epa_line_mask`` on the coefficient rows of the unwritten ``depth`` (the 4 B raw sample read for its
   NaN, 1 B written);
3. what a user writes today, on the device: ``(d >= ub[..., None]) & (d < lb[..., None])`` on the written ``depth``.

Bytes counted: the samples read once and the mask bytes written once (the lines and the coefficient rows, 16 to 96 B per
2000 samples, are left out), against 8 TB/s.  The three results are compared bit for bit before anything is timed, and
the whole ``mask.line_mask`` call (host clock ended by a synchronise) is timed next to the kernels.  Writes the JSON
document to ``--out`` (default profiles/line_mask_bench.json) and prints it."""
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
from echopype_amd.mask.api import _lazy_range_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=100_000)
ap.add_argument("--samples", type=int, default=2000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_mask_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_line_mask.py needs a GPU: a time taken elsewhere says nothing")
C, P, S, REPS, WARM = args.channels, args.pings, args.samples, args.reps, args.warmup
HBM_PEAK = 8.0e12
logging.disable(logging.WARNING)


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


# resident echodata: the samples generated in HBM, the per-ping parameters at full length from the host recipe
d = ep.synth.ek60_numpy(C, P, 8)
d["backscatter_r"] = ep.DeviceArray(ep.synth.ek60_device(C, P, S)["backscatter_r"])
ed = ep.echodata.from_ek60_arrays(d).to_device()

p = np.arange(P)
up_h = np.tile(10.0 + 0.25 * (p % 7), (C, 1))
lo_h = np.tile(150.0 + 30.0 * np.sin(p / 5000.0), (C, 1))
lo_h[:, ::100] = np.nan
ub, lb = ops.to_device(up_h), ops.to_device(lo_h)
up_da = ep.DataArray(ep.DeviceArray(ub), ("channel", "ping_time"))
lo_da = ep.DataArray(ep.DeviceArray(lb), ("channel", "ping_time"))
samples = C * P * S
res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": C, "pings": P, "range_samples": S, "bounds": "upper and lower, (channel, ping_time) float64 "
                    "on the device, lower NaN in 1 ping of 100", "closed": "left", "nan_line": "exclude"},
       "tuning": "untuned, a single run: 16 samples per lane, one 16-byte store each, one piece of rows per workgroup",
       "bytes_counted": "range samples read once (array: 4 / 8 B, lazy: the 4 B raw sample) + 1 mask byte written per sample",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, the three routes alternating"}

for dtype in ("float32", "float64"):
    ds = ep.consolidate.add_depth(ep.calibrate.compute_Sv(ed, dtype=dtype), depth_offset=5.0, tilt=10.0)
    lazy = ds["depth"].data
    rows, raw, scale, offset = _lazy_range_rows(ds["depth"], tuple(ds["Sv"].dims))
    tdt = torch.float32 if dtype == "float32" else torch.float64
    kw = dict(upper=ub, lower=lb)
    api = lambda: ep.mask.line_mask(ds, upper=up_da, lower=lo_da)  # noqa: E731
    t_api_lazy = [host_timed(api)[0] for _ in range(WARM + 7)][WARM:]
    assert not lazy.materialized
    depth = lazy.tensor  # written now: 4 / 8 B per sample
    routes = {
        "array_route": lambda: ops.line_mask((C, P, S), range=depth, **kw),
        "lazy_route": lambda: ops.line_mask((C, P, S), coef=rows, nan_raw=raw, scale=scale, offset=offset, dtype=tdt, **kw),
        "torch_expression": lambda: (depth >= ub[..., None]) & (depth < lb[..., None]),
    }
    # the same mask three times, bit for bit, and from the kernels they are meant to be
    with _lib.launch_trace() as tr:
        got = {k: f() for k, f in routes.items()}
    assert tr.kernels == ["line_mask_kernel", "line_mask_kernel_rows"], tr.kernels
    assert torch.equal(got["array_route"], got["torch_expression"]) and torch.equal(got["lazy_route"], got["torch_expression"])
    kept = float(got["array_route"].float().mean())
    del got
    times = {k: [] for k in routes}
    for i in range(WARM + REPS):
        for k, f in routes.items():
            ms, out = event_timed(f)
            del out
            if i >= WARM:
                times[k].append(ms)
    t_api_array = [host_timed(api)[0] for _ in range(WARM + 7)][WARM:]
    item = 4 if dtype == "float32" else 8
    need = {"array_route": samples * (item + 1), "lazy_route": samples * (4 + 1), "torch_expression": samples * (item + 1)}
    doc = {"fraction_of_samples_kept": kept, "bit_equal_to_the_torch_expression": True}
    for k in routes:
        s = summary(times[k])
        rate = need[k] / (s["ms_median"] * 1e-3)
        doc[k] = {**s, "bytes_needed": need[k], "TB_per_s_median": rate / 1e12, "fraction_of_8_TB_per_s": rate / HBM_PEAK}
    tm = doc["torch_expression"]["ms_median"]
    doc["torch_expression_over_array_route_time_ratio_median"] = tm / doc["array_route"]["ms_median"]
    doc["torch_expression_over_lazy_route_time_ratio_median"] = tm / doc["lazy_route"]["ms_median"]
    doc["mask_line_mask_whole_call_lazy_depth_host_clock"] = summary(t_api_lazy)
    doc["mask_line_mask_whole_call_written_depth_host_clock"] = summary(t_api_array)
    res[f"depth_{dtype}"] = doc
    del ds, lazy, depth, rows, raw, scale, offset, routes, api

out = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out + "\n")
print(out)
