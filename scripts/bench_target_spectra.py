#!/usr/bin/env python3
"""``targets.target_spectra`` at a survey's size: a device-generated table of 10**6 targets over one channel x 200 000
pings x 2500 samples x 4 sectors of float32 complex samples, the 177-tap replica of the synthetic 70 kHz channel,
F = 101 frequencies, half windows h = 8 and 32, float32 and float64 spectra.

Per case, in one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup``
warm-up runs, by device events around the call of the wrapper, the two routes alternating so that they see the same
machine:

1. the kernel wrapper (``ops.target_spectra``: both kernels);
2. the same rules as batched torch operations on the device, a floor in complex128: a gather of the sector-summed
   windows, a product with the replica's Toeplitz matrix, a product with the DFT matrix, |Y|^2 / |A|^2 and the
   logarithm -- in chunks of ``--chunk`` targets, without the NaN handling, the per-sector path and the compensation.

Bytes counted: the staged samples read (2h + L samples x 4 sectors x 2 parts x 4 B per target) plus the rows written
(2 F values and 4 B per target), against 8 TB/s.  Writes the JSON document to ``--out`` (default
profiles/target_spectra_bench.json) and prints it."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from echopype_amd import _lib, ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pings", type=int, default=200_000)
ap.add_argument("--samples", type=int, default=2500)
ap.add_argument("--targets", type=int, default=1_000_000)
ap.add_argument("--frequencies", type=int, default=101)
ap.add_argument("--chunk", type=int, default=50_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_spectra_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_target_spectra.py needs a GPU: a time taken elsewhere says nothing")
P, S, N, F, REPS, WARM, B = args.pings, args.samples, args.targets, args.frequencies, args.reps, args.warmup, 4
HBM_PEAK = 8.0e12
DT = 8e-6
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


# ---- the workload, generated on the device ------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(20261021)
re = torch.empty((1, P, S, B), dtype=torch.float32, device=dev)
im = torch.empty_like(re)
for p0 in range(0, P, 20_000):
    n = min(20_000, P - p0)
    re[0, p0:p0 + n] = 1e-3 * torch.randn((n, S, B), generator=g, device=dev)
    im[0, p0:p0 + n] = 1e-3 * torch.randn((n, S, B), generator=g, device=dev)
_, replicas, _ = synth.target_spectra_scene(C=1, P=2, S=256, echoes=[])
tx = replicas[0]
L = tx.size
key = torch.sort(torch.randint(0, P * S, (N,), generator=g, device=dev)).values  # ordered by (ping, sample)
ping, sample = (key // S).to(torch.int32), (key % S).to(torch.int32)
chan = torch.zeros(N, dtype=torch.int32, device=dev)
rng = 0.1 + 0.006 * sample.to(torch.float64)
al = 3.0 * torch.rand(N, generator=g, device=dev, dtype=torch.float64) - 1.5
at = 3.0 * torch.rand(N, generator=g, device=dev, dtype=torch.float64) - 1.5
f = np.linspace(49.5e3, 85.5e3, F)
fparams = np.stack([f, np.asarray(synth.fg_absorption(f)), np.full(F, 27.0), np.full(F, 75.0), 6.8 * 70e3 / f, 6.9 * 70e3 / f,
                    np.full(F, 0.05), np.full(F, -0.02)])[None]
fparams_t = torch.as_tensor(fparams).to(dev)
pparams = torch.stack([torch.full((1, P), v, dtype=torch.float64, device=dev) for v in (750.0, 1500.0, 5400.0)]).contiguous()
rep_t = torch.as_tensor(np.ascontiguousarray(tx).view(np.float32)).to(dev)
off_t = torch.as_tensor(np.array([0, L], dtype=np.int32)).to(dev)
dt_t = torch.full((1,), DT, dtype=torch.float64, device=dev)
cmap = torch.zeros(1, dtype=torch.int32, device=dev)

res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": 1, "pings": P, "range_samples": S, "sectors": B, "samples": "float32", "targets": N,
                    "replica_taps": int(L), "frequencies": F},
       "tuning": "untuned, a single run: one workgroup per target, the tap sum of an output split over 256 / (2h + 1) lanes, "
                 "a lane per frequency",
       "bytes_counted": "staged samples read ((2h + L) x 4 sectors x 8 B per target) + rows written (2 F values + 4 B per target)",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, the two routes alternating"}

txc = torch.as_tensor(tx.astype(np.complex128)).to(dev)
E = float(np.sum(np.abs(tx.astype(np.complex128)) ** 2))

for h in (8, 32):
    W = 2 * h + 1
    # Toeplitz matrix of the replica: pc = window (W + L - 1) @ T (W + L - 1, W), T[i + k, i] = conj(tx[k]) / (E B)
    T = torch.zeros((W + L - 1, W), dtype=torch.complex128, device=dev)
    for i in range(W):
        T[i:i + L, i] = torch.conj(txc) / (E * B)
    nn = torch.arange(-h, h + 1, device=dev, dtype=torch.float64)
    ft = torch.as_tensor(f).to(dev)
    D = torch.exp(-2j * np.pi * (nn[:, None] * ft[None, :] * DT))  # (W, F)
    a = np.correlate(tx.astype(np.complex128), tx.astype(np.complex128), "full")[L - 1 - h:L + h] / E  # a(-h .. h)
    A2 = torch.as_tensor(np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(-h, h + 1)[None, :] * DT) @ a) ** 2).to(dev)
    span = torch.arange(W + L - 1, device=dev)
    re2, im2 = re.view(P * S, B), im.view(P * S, B)
    # rules 5 and 6 with the parameters above: what does not depend on the target, and the absorption
    const = torch.as_tensor(10.0 * np.log10(B / 8 * (5475.0 / 5400.0) ** 2 / 75.0) - 2 * 27.0
                            - 10.0 * np.log10(750.0 * (1500.0 / f) ** 2 / (16 * np.pi ** 2))).to(dev)
    alpha2 = torch.as_tensor(2.0 * fparams[0, 1]).to(dev)

    def torch_floor():
        out = torch.empty((N, F), dtype=torch.float64, device=dev)
        for n0 in range(0, N, args.chunk):
            sl = slice(n0, min(n0 + args.chunk, N))
            idx = (key[sl, None] - h + span[None, :]).clamp_(0, P * S - 1)  # (a floor: no zero fill at the row ends)
            win = torch.complex(re2[idx].double().sum(-1), im2[idx].double().sum(-1))
            Y = (win @ T) @ D
            out[sl] = 10.0 * torch.log10((Y.real ** 2 + Y.imag ** 2) / A2) + 40.0 * torch.log10(rng[sl, None]) + \
                alpha2[None, :] * rng[sl, None] + const
        return out

    for dtype in ("float64", "float32"):
        kernel = lambda: ops.target_spectra(re, im, rep_t, off_t, L, dt_t, fparams_t, pparams, h, cmap, chan, ping, sample,  # noqa: E731
                                            rng, al, at, dtype=dtype)
        routes = {"kernel": kernel, "torch_gather_toeplitz_dft": torch_floor}
        with _lib.launch_trace() as tr:
            got = kernel()
        assert tr.kernels == ["target_spectrum_replica_kernel", "target_spectrum_kernel"], tr.kernels
        finite = float(torch.isfinite(got[1]).double().mean())
        if dtype == "float64":  # the two routes compute the same thing where a window and its taps lie inside the row
            inner = ((sample >= h) & (sample + h + L <= S)).nonzero().squeeze(1)
            res[f"h{h}_largest_difference_dB_kernel_vs_torch_floor_inside_rows"] = \
                float((got[1].index_select(0, inner) - torch_floor().index_select(0, inner)).abs().max())
        del got
        times = {k: [] for k in routes}
        for i in range(WARM + REPS):
            for k, fn in routes.items():
                if k != "kernel" and dtype == "float32":  # (the floor does not depend on the output type: timed once per h)
                    continue
                ms, out = event_timed(fn)
                del out
                if i >= WARM:
                    times[k].append(ms)
        item = 4 if dtype == "float32" else 8
        need = N * ((2 * h + L) * B * 8 + 2 * F * item + 4)
        s = summary(times["kernel"])
        rate = need / (s["ms_median"] * 1e-3)
        doc = {"kernel": {**s, "targets_per_s_median": N / (s["ms_median"] * 1e-3), "bytes_needed": need,
                          "TB_per_s_median": rate / 1e12, "fraction_of_8_TB_per_s": rate / HBM_PEAK},
               "finite_fraction_of_TS_spectrum_uncomp": finite}
        if times["torch_gather_toeplitz_dft"]:
            floor = summary(times["torch_gather_toeplitz_dft"])
            res.setdefault("torch_floor", {})[f"h{h}"] = floor
        floor = res["torch_floor"][f"h{h}"]
        doc["kernel_over_torch_floor_time_ratio_median"] = s["ms_median"] / floor["ms_median"]
        res[f"h{h}_{dtype}"] = doc

out = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(out + "\n")
print(out)
