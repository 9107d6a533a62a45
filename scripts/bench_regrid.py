#!/usr/bin/env python3
"""``commongrid.regrid_Sv``'s kernel at a survey's size: 4 channels x 100 000 pings x 2000 samples, two channels sampled
every 0.047 m and two every 0.188 m, the range a (channel, ping_time, range_sample) cube of Sv's type as ``compute_Sv``
leaves it, Sv uniform in [-90, -30] dB with a NaN tail of 100 samples in one ping of ten; float32 and float64; onto cells
of 0.2 m and of 1 m up to the largest range.

Per type and cell size, in one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after
``--warmup`` warm-up runs, by device events around the call of the wrapper, the two alternating so that they see the
same machine:

1. ``ops.regrid_rows`` (``epa_regrid_rows``, Sv and coverage written);
2. a floor that does less work: sample-CENTRE binning as a torch expression (``bucketize`` + two ``index_add_``), which
   neither splits a sample between cells nor weighs it by its thickness.

Bytes counted for the kernel: Sv and range read once, Sv and coverage written once, against 8 TB/s.  Before anything is
timed the conserved quantity is checked on the whole volume with torch in float64: for every row
``sum_j 10^(Sv_j/10) coverage_j bin`` against the integral of the samples over the grid.  Writes the JSON document to
``--out`` (default profiles/regrid_bench.json) and prints it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from echopype_amd import _lib, ops  # noqa: E402
from echopype_amd.commongrid.deferred import range_edges  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=4)
ap.add_argument("--pings", type=int, default=100_000)
ap.add_argument("--samples", type=int, default=2000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_regrid.py needs a GPU: a time taken elsewhere says nothing")
C, P, S, REPS, WARM = args.channels, args.pings, args.samples, args.reps, args.warmup
HBM_PEAK = 8.0e12
D0 = 0.047
dev = torch.device("cuda")


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def volume(tdt):
    g = torch.Generator(device=dev).manual_seed(20261020)
    sv = torch.rand((C, P, S), generator=g, device=dev, dtype=tdt) * 60.0 - 90.0
    sv[:, ::10, S - 100:] = float("nan")
    step = torch.tensor([D0 if c < C // 2 else 4 * D0 for c in range(C)], device=dev, dtype=torch.float64)
    r = (torch.arange(S, device=dev, dtype=torch.float64)[None, :] + 0.5) * step[:, None]
    # every ping its own sound speed, a few parts in a thousand: the cube is not one row repeated
    scale = 1.0 + 0.004 * torch.sin(torch.arange(P, device=dev, dtype=torch.float64) / 3000.0)
    return sv, (r[:, None, :] * scale[None, :, None]).to(tdt).contiguous()


def integral_of_the_samples(sv, r, top):
    """sum_i 10^(v_i/10) |[m[i], m[i+1]) n [0, top)| per row, float64 (all ranges finite and increasing here)."""
    r = r.double()
    mid = (r[..., :-1] + r[..., 1:]) / 2
    lo = torch.cat([r[..., :1] - (r[..., 1:2] - r[..., :1]) / 2, mid], dim=-1)
    hi = torch.cat([mid, r[..., -1:] + (r[..., -1:] - r[..., -2:-1]) / 2], dim=-1)
    width = (hi.clamp(max=top) - lo.clamp(min=0.0)).clamp(min=0.0)
    lin = torch.pow(10.0, sv.double() / 10.0)
    return torch.where(torch.isnan(lin), torch.zeros_like(lin), lin * width).sum(dim=-1)


res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": C, "pings": P, "range_samples": S, "sample_spacing_m": [D0, 4 * D0],
                    "range": "(channel, ping_time, range_sample) cube of Sv's type", "sv": "uniform in [-90, -30] dB, the last "
                    "100 samples NaN in one ping of ten"},
       "tuning": f"untuned, a single run: a workgroup of 256 lanes per row, tiles of {_lib.REGRID_TILE} samples in "
                 "LDS, float64 arithmetic for both types, element loads",
       "bytes_counted": "Sv and range read once + Sv and coverage written once",
       "floor": "sample-centre binning as a torch expression (bucketize + two index_add_): less work, another result",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, kernel and floor alternating"}

for name, tdt in (("float32", torch.float32), ("float64", torch.float64)):
    sv, r = volume(tdt)
    rmax = float(r.max().item())
    item = sv.element_size()
    rows = torch.arange(C * P, device=dev).view(C, P, 1)
    for range_bin in (0.2, 1.0):
        edges = range_edges(rmax, range_bin)
        J = len(edges) - 1
        edges_t = torch.as_tensor(edges, device=dev).to(tdt)

        def kernel():
            return ops.regrid_rows(sv, r, range_bin, J)

        def floor():
            j = torch.bucketize(r, edges_t, right=True) - 1
            ok = (j >= 0) & (j < J) & ~torch.isnan(sv)
            flat = (rows * J + j.clamp(0, J - 1)).view(-1)
            lin = torch.where(ok, torch.pow(10.0, sv / 10.0), torch.zeros_like(sv)).view(-1)
            num = torch.zeros(C * P * J, dtype=tdt, device=dev).index_add_(0, flat, lin)
            cnt = torch.zeros(C * P * J, dtype=tdt, device=dev).index_add_(0, flat, ok.to(tdt).view(-1))
            return 10.0 * torch.log10(num / cnt)

        with _lib.launch_trace() as tr:
            got_sv, got_cov, n_bad = kernel()
        assert tr.kernels == ["regrid_rows_kernel"], tr.kernels
        assert int(n_bad.item()) == 0
        lin = torch.where(got_cov > 0, torch.pow(10.0, got_sv.double() / 10.0), torch.zeros_like(got_sv, dtype=torch.float64))
        lhs = (lin * got_cov.double() * range_bin).sum(dim=-1)
        rhs = integral_of_the_samples(sv, r, float(edges[-1]))
        worst = float(((lhs - rhs).abs() / rhs).max().item())
        assert worst <= (1e-12 if tdt == torch.float64 else 1e-6), worst  # (the bounds of tests/test_gpu_regrid.py)
        covered = float((got_cov > 0).double().mean().item())
        del got_sv, got_cov, lin, lhs, rhs
        times = {"regrid_rows": [], "torch_centre_binning": []}
        for i in range(WARM + REPS):
            for k, f in (("regrid_rows", kernel), ("torch_centre_binning", floor)):
                ms, out = event_timed(f)
                del out
                if i >= WARM:
                    times[k].append(ms)
        need = C * P * S * 2 * item + C * P * J * 2 * item
        s = summary(times["regrid_rows"])
        rate = need / (s["ms_median"] * 1e-3)
        fl = summary(times["torch_centre_binning"])
        res[f"{name}_bin_{range_bin}m"] = {
            "range_cells": J, "fraction_of_cells_covered": covered, "conserved_quantity_worst_relative_difference": worst,
            "regrid_rows": {**s, "bytes_needed": need, "TB_per_s_median": rate / 1e12, "fraction_of_8_TB_per_s": rate / HBM_PEAK},
            "torch_centre_binning": fl,
            "floor_over_kernel_time_ratio_median": fl["ms_median"] / s["ms_median"]}
    del sv, r, rows

out = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out + "\n")
print(out)
