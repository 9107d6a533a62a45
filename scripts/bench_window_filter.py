#!/usr/bin/env python3
"""``clean.window_filter``'s kernel at a survey's size: 4 channels x 100 000 pings x 2000 samples of Sv, noise of 3 dB around
-70 dB with one sample in a hundred raised by 35 dB and a NaN tail of 100 samples in one ping of ten; float32 and float64.

Cases: the median and the mean at 3 x 3, 5 x 5 and 7 x 7, the minimum at 3 x 3.  Per type and case, in one process, the
median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup`` warm-up runs, by device events around
``ops.window_filter`` writing into an output allocated beforehand.  Bytes counted: the input read once + the output written
once, against 8 TB/s.  Two floors that do less work, timed the same way:

1. ``torch.nn.functional.avg_pool2d`` on the linear values, converted beforehand (no NaN rule -- a NaN spreads --, no
   dB <-> linear conversion; ``count_include_pad=False`` is its shrinking edge), beside every mean;
2. a device-to-device copy of the volume: the same bytes.

Before a case is timed its kernel is named by the launch trace and the result of one channel's first 64 pings is held to
the NumPy restatement (tests/window_filter_ref.py) by the rule of tests/test_gpu_window_filter.py.  Writes the JSON
document to ``--out`` (default profiles/window_filter_bench.json) and prints it.  One command, under its own limit:

    timeout -k 10 900 python scripts/bench_window_filter.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from echopype_amd import _lib, ops  # noqa: E402
from window_filter_ref import window_filter_ref, window_results  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=100_000)
ap.add_argument("--samples", type=int, default=2000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_filter_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_window_filter.py needs a GPU: a time taken elsewhere says nothing")
C, P, S, REPS, WARM = args.channels, args.pings, args.samples, args.reps, args.warmup
HBM_PEAK = 8.0e12
CASES = [("median", 3), ("median", 5), ("median", 7), ("mean", 3), ("mean", 5), ("mean", 7), ("min", 3)]
dev = torch.device("cuda")


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn):
    ts = [event_timed(fn) for _ in range(WARM + REPS)]
    return summary(ts[WARM:])


def volume(tdt):
    g = torch.Generator(device=dev).manual_seed(20261020)
    sv = torch.randn((C, P, S), generator=g, device=dev, dtype=tdt) * 3.0 - 70.0
    sv += 35.0 * (torch.rand((C, P, S), generator=g, device=dev, dtype=torch.float32) < 0.01).to(tdt)
    sv[:, ::10, S - 100:] = float("nan")
    return sv


def check(sv, got, method, k):
    """One channel's first 64 pings against the oracle (their windows reach into 64 + k // 2 pings)."""
    n_p = min(P, 64)
    x = sv[0, :n_p + k // 2].cpu().numpy()
    want = window_filter_ref(x, method, k, k)[:n_p]
    n = window_results(x, k, k)[1][:n_p]
    g = got[0, :n_p].cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), (method, k)
    f = np.isfinite(want)
    exact = f if method == "min" else (f & (n % 2 == 1) if method == "median" else np.zeros_like(f))
    assert np.array_equal(g[exact], want[exact]), (method, k)
    f &= ~exact
    tol = 1e-9 if want.dtype == np.float64 else np.spacing(np.abs(want[f])).astype(np.float64)
    assert (np.abs(g[f].astype(np.float64) - want[f].astype(np.float64)) <= tol).all(), (method, k)


res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": C, "pings": P, "range_samples": S, "sv": "normal, 3 dB around -70 dB, one sample in a hundred "
                    "35 dB higher, the last 100 samples NaN in one ping of ten"},
       "tuning": f"untuned, a single run: a workgroup of 256 lanes per tile of {_lib.WINDOW_FILTER_TP} x "
                 f"{_lib.WINDOW_FILTER_TS} samples, the tile and its halo in LDS, element loads and stores; the median is one "
                 "bitwise selection for every window size",
       "bytes_counted": "the input read once + the output written once",
       "floors": "torch.nn.functional.avg_pool2d on the linear values (no NaN rule, no conversion) beside the mean; a "
                 "device-to-device copy of the volume for the bytes: both do less work",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, the output allocated beforehand"}

for name, tdt in (("float32", torch.float32), ("float64", torch.float64)):
    sv = volume(tdt)
    out = torch.empty_like(sv)
    need = 2 * sv.numel() * sv.element_size()
    entry = {"bytes_needed": need}
    s = timed(lambda: out.copy_(sv))
    entry["device_to_device_copy"] = {**s, "TB_per_s_median": need / (s["ms_median"] * 1e-3) / 1e12}
    lin = torch.pow(10.0, sv / 10.0).unsqueeze(0)  # (1, C, P, S): channels as avg_pool2d's feature planes
    for method, k in CASES:
        with _lib.launch_trace() as tr:
            ops.window_filter(sv, method, k, k, out=out)
        assert tr.kernels == [f"window_filter_kernel<{method}>"], tr.kernels
        check(sv, out, method, k)
        s = timed(lambda: ops.window_filter(sv, method, k, k, out=out))
        rate = need / (s["ms_median"] * 1e-3)
        case = {"window_filter": {**s, "TB_per_s_median": rate / 1e12, "fraction_of_8_TB_per_s": rate / HBM_PEAK}}
        if method == "mean":
            fl = timed(lambda: torch.nn.functional.avg_pool2d(lin, k, stride=1, padding=k // 2, count_include_pad=False))
            case["torch_avg_pool2d_on_linear_values"] = fl
            case["floor_over_kernel_time_ratio_median"] = fl["ms_median"] / s["ms_median"]
        entry[f"{method}_{k}x{k}"] = case
    res[name] = entry
    del sv, out, lin

doc = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
