#!/usr/bin/env python3
"""``calibrate.compute_Sv_spectrum`` at a survey's size: the device-generated volume of bench_target_spectra.py -- one
channel x 200 000 pings x 2500 samples x 4 sectors of float32 complex noise --, the 177-tap replica of the synthetic
70 kHz channel, F = 101 frequencies, Hann windows of N_w = 64 and 256 samples at the default hop, float64 spectra.

Per case, in one process, the median, minimum and maximum of ``--reps`` (at least 20) timed runs after ``--warmup``
warm-up runs, by device events around the call, the two routes alternating so that they see the same machine:

1. the kernel wrapper (``ops.sv_spectrum``: both kernels) writing into preallocated outputs;
2. the same rules as batched torch operations on the device, a floor in complex128: the sector sum, the compression by
   FFT (length 4096), ``unfold`` into cells, the window, a product with the DFT matrix, |Y|^2 / |A|^2 and the logarithm
   -- in chunks of ``--chunk`` pings, without the NaN handling and the per-sector path.

Work counted: complex multiply-adds of the rules -- S L for the compression and M F N_w for the Fourier sums per ping --
at 8 flops each against the 78.6 TFLOP/s float64 vector peak.  Not asserted, only recorded: the dB difference between the
band mean of 10^(Sv(f)/10) and the mean of ``compute_Sv``'s 10^(Sv/10) over the samples of the cells, on the first
``--compare-pings`` pings of the volume through the public entry points (small but not zero: ``compute_Sv`` uses
tau_effective and the parameters at the centre frequency).  Writes the JSON document to ``--out`` (default
profiles/sv_spectrum_bench.json) and prints it."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import echopype_amd as ep  # noqa: E402
from echopype_amd import _lib, echodata, ops, synth  # noqa: E402
from echopype_amd.calibrate.sv_spectrum import normalised_window  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pings", type=int, default=200_000)
ap.add_argument("--samples", type=int, default=2500)
ap.add_argument("--frequencies", type=int, default=101)
ap.add_argument("--chunk", type=int, default=4000)
ap.add_argument("--compare-pings", type=int, default=500)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sv_spectrum_bench.json"))
args = ap.parse_args()
if args.reps < 20 or args.warmup < 1:
    ap.error("--reps must be at least 20 and --warmup at least 1: the spread is part of the result")
if not torch.cuda.is_available():
    sys.exit("bench_sv_spectrum.py needs a GPU: a time taken elsewhere says nothing")
P, S, F, REPS, WARM, B = args.pings, args.samples, args.frequencies, args.reps, args.warmup, 4
FP64_PEAK = 78.6e12
DT, NFFT = 8e-6, 4096
logging.disable(logging.WARNING)
dev = torch.device("cuda", 0)


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


# ---- the workload, generated on the device (the stream of bench_target_spectra.py) ----------------------------------------
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
f = np.linspace(49.5e3, 85.5e3, F)
P_T, C_W, Z_ER, Z_ET, GAIN, PSI = 750.0, 1500.0, 5400.0, 75.0, 27.0, -20.7
alpha = np.asarray(synth.fg_absorption(f))
fparams = np.stack([f, alpha, np.full(F, GAIN), np.full(F, Z_ET), PSI + 20 * np.log10(70e3 / f)])[None]
fparams_t = torch.as_tensor(fparams).to(dev)
pparams = torch.stack([torch.full((1, P), v, dtype=torch.float64, device=dev) for v in (P_T, C_W, Z_ER, DT)]).contiguous()
rep_t = torch.as_tensor(np.ascontiguousarray(tx).view(np.float32)).to(dev)
off_t = torch.as_tensor(np.array([0, L], dtype=np.int32)).to(dev)
dt_t = torch.full((1,), DT, dtype=torch.float64, device=dev)

res = {"device": torch.cuda.get_device_name(0),
       "workload": {"channels": 1, "pings": P, "range_samples": S, "sectors": B, "samples": "float32", "replica_taps": int(L),
                    "frequencies": F, "window": "hann", "spectra": "float64"},
       "tuning": "untuned, a single run of this script: one workgroup per (ping, tile of cells), a lane per compressed sample, "
                 "a lane per (cell, frequency) pair",
       "work_counted": "complex multiply-adds of the rules per ping, S L (compression) + M F N_w (Fourier sums), 8 flops each, "
                       "against 78.6 TFLOP/s (float64 vector peak)",
       "timing": f"device events around the call, median of {REPS} after {WARM} warm-ups, the two routes alternating"}

txc = np.zeros(NFFT, dtype=np.complex128)
txc[:L] = tx.astype(np.complex128)
E = float(np.sum(np.abs(tx.astype(np.complex128)) ** 2))
TXF = torch.as_tensor(np.conj(np.fft.fft(txc)) / (E * B)).to(dev)  # correlation with the replica, sector mean, 1 / E
r_n = torch.arange(S, dtype=torch.float64, device=dev) * DT * (C_W / 2)

for Nw in (64, 256):
    hop = -(-Nw // 2)
    M = ops.sv_spectrum_cells(S, Nw, hop)
    win = normalised_window(Nw, "hann")
    win_t = torch.as_tensor(win).to(dev)
    hh = min((Nw - 1) // 2, L - 1)
    a = np.correlate(tx.astype(np.complex128), tx.astype(np.complex128), "full")[L - 1 - hh:L + hh] / E  # a(-hh .. hh)
    A2 = torch.as_tensor(np.abs(np.exp(-2j * np.pi * f[:, None] * np.arange(-hh, hh + 1)[None, :] * DT) @ a) ** 2).to(dev)
    kk = torch.arange(Nw, device=dev, dtype=torch.float64)
    D = torch.exp(-2j * np.pi * (kk[:, None] * torch.as_tensor(f).to(dev)[None, :] * DT)) * win_t[:, None]  # (Nw, F), windowed
    r_m = (r_n[torch.arange(M, device=dev) * hop] + r_n[torch.arange(M, device=dev) * hop + Nw - 1]) / 2
    const = torch.as_tensor(10.0 * np.log10(B / 8 * ((Z_ER + Z_ET) / Z_ER) ** 2 / Z_ET) - 2 * GAIN
                            - 10.0 * np.log10(P_T * (C_W / f) ** 2 * C_W / (32 * np.pi ** 2)) - 10.0 * np.log10(Nw * DT)
                            - fparams[0, 4]).to(dev)
    absorb = 2.0 * torch.as_tensor(alpha).to(dev)[None, :] * r_m[:, None]  # (M, F)
    sv = torch.empty((1, P, M, F), dtype=torch.float64, device=dev)
    rng = torch.empty((1, P, M), dtype=torch.float64, device=dev)
    sv_floor = torch.empty((P, M, F), dtype=torch.float64, device=dev)

    def kernel():
        ops.sv_spectrum(re, im, rep_t, off_t, L, dt_t, fparams_t, pparams, win_t, hop, out=(sv, rng))

    def torch_floor():
        for p0 in range(0, P, args.chunk):
            sl = slice(p0, min(p0 + args.chunk, P))
            z = torch.complex(re[0, sl].double().sum(-1), im[0, sl].double().sum(-1))  # (n, S)
            pc = torch.fft.ifft(torch.fft.fft(z, NFFT, dim=1) * TXF[None, :], dim=1)[:, :S]
            cells = (pc * r_n[None, :]).unfold(1, Nw, hop)  # (n, M, Nw)
            Y = cells @ D
            sv_floor[sl] = 10.0 * torch.log10((Y.real ** 2 + Y.imag ** 2) / A2) + absorb + const

    with _lib.launch_trace() as tr:
        kernel()
    assert tr.kernels == ["sv_spectrum_replica_kernel", "sv_spectrum_kernel"], tr.kernels
    torch_floor()
    torch.cuda.synchronize()
    finite = float(torch.isfinite(sv).double().mean())
    diff = float((sv[0] - sv_floor).abs().max())
    routes = {"kernel": kernel, "torch_fft_unfold_dft": torch_floor}
    times = {k: [] for k in routes}
    for i in range(WARM + REPS):
        for k, fn in routes.items():
            ms = event_timed(fn)
            if i >= WARM:
                times[k].append(ms)
    cmacs = P * (S * L + M * F * Nw)
    s, fl = summary(times["kernel"]), summary(times["torch_fft_unfold_dft"])
    rate = cmacs / (s["ms_median"] * 1e-3)
    cells_t, tiles, lds = ops.sv_spectrum_plan(L, Nw, hop, M)
    res[f"Nw{Nw}"] = {
        "step_samples": hop, "cells_per_ping": M, "tile_cells": cells_t, "tiles_per_ping": tiles, "lds_bytes_per_workgroup": lds,
        "kernel": {**s, "complex_multiply_adds": cmacs, "complex_multiply_adds_per_s_median": rate,
                   "fraction_of_78.6_TFLOP_per_s_float64_vector_peak": 8 * rate / FP64_PEAK},
        "torch_floor": fl, "kernel_over_torch_floor_time_ratio_median": s["ms_median"] / fl["ms_median"],
        "finite_fraction_of_Sv_spectrum": finite, "largest_difference_dB_kernel_vs_torch_floor": diff}
    del sv, rng, sv_floor

# ---- the band mean of Sv(f) against compute_Sv's cell mean, through the public entry points (recorded, not asserted) ------
NP = min(args.compare_pings, P)
d, _, _ = synth.target_spectra_scene(C=1, P=NP, S=S, B=B, dtype=np.float32, noise=0.0, tail=0, echoes=[])
d["backscatter_r"], d["backscatter_i"] = re[:, :NP].cpu().numpy(), im[:, :NP].cpu().numpy()
ed = echodata.from_ek80_arrays(d, d["filters"])
sv_band = np.asarray(ep.calibrate.compute_Sv(ed, waveform_mode="BB", encode_mode="complex")["Sv"].values)[0]  # (NP, S)
lin = 10.0 ** (sv_band / 10.0)
for Nw in (64, 256):
    hop = -(-Nw // 2)
    doc = {"pings": NP, "note": "means of 10^(Sv/10) over pings, cells 1 .. M - 3 (away from the row ends, where the "
                                "compression sees the whole replica) and, for Sv(f), the frequencies; recorded, not asserted"}
    for margin in (0.1, 0.25):
        out = ep.calibrate.compute_Sv_spectrum(ed, {"window_samples": Nw, "n_frequencies": F, "band_margin": margin})
        spec = np.asarray(out["Sv_spectrum"].values)[0]  # (NP, M, F)
        M = spec.shape[1]
        cell_mean = np.stack([lin[:, m * hop:m * hop + Nw].mean(axis=1) for m in range(M)], axis=1)  # (NP, M)
        inner = slice(1, M - 2)
        a_db = 10.0 * np.log10(np.nanmean(10.0 ** (spec[:, inner] / 10.0)))
        b_db = 10.0 * np.log10(np.nanmean(cell_mean[:, inner]))
        doc[f"band_margin_{margin}"] = {"difference_dB": float(a_db - b_db), "band_mean_dB": float(a_db),
                                        "compute_Sv_cell_mean_dB": float(b_db)}
    res[f"Nw{Nw}"]["band_mean_of_Sv_spectrum_minus_compute_Sv_cell_mean"] = doc

out = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(out + "\n")
print(out)
