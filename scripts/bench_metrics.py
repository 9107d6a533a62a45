#!/usr/bin/env python3
"""The echo summary statistics (csrc/metrics.hip) at workload-sized shapes next to the same formulas as device torch
expressions on the same data, in one run: ``metrics.summary`` (all five from one sweep) and ``metrics.abundance`` alone
on a 4 x 100 000 x 2000 cube in float32 and float64 (a row per wave) and on 4 x 500 x 100 000 in float32 (long rows: a
workgroup per row, read twice, the second time from L2).  Median and minimum of 20 timed calls in ms (HIP events around
each call) and the algorithmic bytes -- ONE read of Sv and one of the range, 8 B per sample in float32, 16 B in
float64 -- per second, also as a fraction of 8 TB/s.  Prints one JSON document."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import echopype_amd as ep  # noqa: E402
from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray  # noqa: E402

PEAK = 8e12


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def torch_sums(sv, r):
    dz = torch.diff(r, dim=-1)
    dz = torch.where(dz != 0, dz, torch.full_like(dz, float("nan")))
    lin = torch.pow(10.0, sv[..., 1:] / 10)
    return dz, lin, lin * dz


def torch_abundance(sv, r):
    return 10 * torch.log10(torch.nansum(torch_sums(sv, r)[2], dim=-1))


def torch_summary(sv, r):
    dz, lin, w = torch_sums(sv, r)
    r1 = r[..., 1:]
    A = torch.nansum(w, dim=-1)
    cm = torch.nansum(r1 * w, dim=-1) / A
    even = A ** 2 / torch.nansum(lin ** 2 * dz, dim=-1)
    return {"abundance": 10 * torch.log10(A), "center_of_mass": cm,
            "dispersion": torch.nansum((r1 - cm[..., None]) ** 2 * w, dim=-1) / A, "evenness": even, "aggregation": 1 / even}


def shape_case(tag, C, P, S, dtype, res):
    g = torch.Generator(device="cuda").manual_seed(1)
    sv = (torch.rand((C, P, S), device="cuda", generator=g) * 60 - 90).to(dtype)
    r = torch.cumsum(torch.rand((C, P, S), device="cuda", generator=g) * 0.2 + 0.1, dim=-1).to(dtype)
    sv[:, :, S - S // 8:] = float("nan")  # a NaN tail, as below the seafloor
    ds = Dataset(coords={"channel": np.arange(C), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    dims = ("channel", "ping_time", "range_sample")
    ds["Sv"], ds["echo_range"] = DataArray(DeviceArray(sv), dims), DataArray(DeviceArray(r), dims)
    nbytes = 2 * sv.numel() * sv.element_size()
    for name, fn, base in (("summary", lambda: ep.metrics.summary(ds), lambda: torch_summary(sv, r)),
                           ("abundance", lambda: ep.metrics.abundance(ds), lambda: torch_abundance(sv, r))):
        med, mn = timed(fn)
        tmed, tmn = timed(base)
        res[f"{name}_{tag}"] = {"shape": [C, P, S], "dtype": str(dtype).replace("torch.", ""), "ms_median": med, "ms_min": mn,
                                "bytes": nbytes, "TB_per_s": nbytes / med / 1e9, "of_8_TB_per_s": nbytes / (med * 1e-3) / PEAK,
                                "torch_ms_median": tmed, "torch_ms_min": tmn, "torch_over_kernel": tmed / med}
    got, want = ep.metrics.summary(ds), torch_summary(sv, r)
    tol = 1e-4 if dtype == torch.float32 else 1e-9
    for k, v in want.items():
        assert torch.allclose(got[k].data.tensor, v, rtol=tol, atol=tol, equal_nan=True), (tag, k)
    del ds, sv, r


res = {}
shape_case("f32", 4, 100000, 2000, torch.float32, res)
shape_case("f64", 4, 100000, 2000, torch.float64, res)
shape_case("f32_long_rows", 4, 500, 100000, torch.float32, res)
print(json.dumps(res, indent=1))
