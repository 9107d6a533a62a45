#!/usr/bin/env python3
"""Split-beam angles (consolidate.add_splitbeam_angle) at kernel level: one JSON line per form with the wall time of a
pass (median of --steps timed passes after --warmup), the algorithmic bytes and the fraction of 8 TB/s.

  power   EK60 power/angle, int8 planes in, f64 theta / phi out:      4 x 100 000 x 2000      (2 + 16 = 18 B/sample)
  cw      EK80 CW complex, f32 planes (B = 4), f64 out:              2 x 200 000 x 8192 x 4  (32 + 16 = 48 B/sample)
  bb_pc   the same volume, BB with pulse compression (177-tap replica: the LDS-FFT form), and the ratio of its time to
          compute_Sv's BB kernel (ops.sv_complex, FFT form, Sv + range statistics) on the same volume

The planes are generated in HBM (no PCIe in the timed passes).  --scale shrinks the ping counts (profiling runs)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echopype_amd import _lib, ops, synth  # noqa: E402
from echopype_amd.calibrate.ek80_complex import filter_decimate_chirp, tapered_chirp  # noqa: E402

HBM = 8.0e12


def timed(f, steps, warmup):
    t = ops.Timer()
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t.start()
        f()
        t.stop()
        ms.append(t.elapsed_ms())
    return float(np.median(ms)), [round(m, 3) for m in ms]


def line(form, shape, ms, all_ms, bytes_per_sample, **extra):
    n = int(np.prod(shape[:3]))
    nbytes = n * bytes_per_sample
    out = dict(form=form, shape=list(shape), ms_per_pass=round(ms, 3), passes_ms=all_ms, samples=n,
               bytes_per_sample=bytes_per_sample, algorithmic_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3),
               fraction_of_8tbs=round(nbytes / ms / 1e9 / (HBM / 1e12), 3), **extra)
    print(json.dumps(out), flush=True)


def params(C, dev):
    return [torch.tensor(np.linspace(21.0, 23.0, C), dtype=torch.float64, device=dev),
            torch.tensor(np.linspace(22.0, 24.0, C), dtype=torch.float64, device=dev),
            torch.tensor(np.linspace(-0.1, 0.1, C), dtype=torch.float64, device=dev),
            torch.tensor(np.linspace(0.05, -0.05, C), dtype=torch.float64, device=dev)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the ping counts")
    ap.add_argument("--forms", default="power,cw,bb_pc")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261015)
    forms = a.forms.split(",")

    if "power" in forms:
        C, P, S = 4, max(1, int(100_000 * a.scale)), 2000
        al = torch.randint(-128, 128, (C, P, S), generator=gen, device=dev, dtype=torch.int8)
        at = torch.randint(-128, 128, (C, P, S), generator=gen, device=dev, dtype=torch.int8)
        prm = params(C, dev)
        ms, all_ms = timed(lambda: ops.splitbeam_power(al, at, prm), a.steps, a.warmup)
        line("power_i8_f64", (C, P, S), ms, all_ms, 2 + 16)
        del al, at
        torch.cuda.empty_cache()

    if "cw" in forms or "bb_pc" in forms:
        C, P, S, B = 2, max(1, int(200_000 * a.scale)), 8192, 4
        re = torch.empty((C, P, S, B), device=dev, dtype=torch.float32)
        im = torch.empty_like(re)
        for p0 in range(0, P, 10_000):  # (in slabs: randn's temporaries stay small)
            re[:, p0:p0 + 10_000].normal_(0.0, 1e-3, generator=gen)
            im[:, p0:p0 + 10_000].normal_(0.0, 1e-3, generator=gen)
        prm = params(C, dev)
        bt = [1] * C
        if "cw" in forms:
            ms, all_ms = timed(lambda: ops.splitbeam_complex(re, im, bt, prm), a.steps, a.warmup)
            line("cw_complex_f32_f64", (C, P, S, B), ms, all_ms, 32 + 16)
        if "bb_pc" in forms:
            f = synth.ek80_filters()
            reps = []
            for c in range(C):
                y, _ = tapered_chirp(1.5e6, 1.024e-3, 0.05, 45e3 + 45e3 * c, 90e3 + 80e3 * c)
                reps.append(filter_decimate_chirp(f, y, 1.5e6)[0])
            off = torch.tensor(np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32), device=dev)
            rep = torch.tensor(np.concatenate(reps).astype(np.complex64).view(np.float32), device=dev)
            taps = int(max(r.size for r in reps))
            kw = dict(replica=rep, replica_off=off, max_taps=taps)
            form = "fft" if ops.splitbeam_uses_fft(rep, taps) else "direct"
            ms, all_ms = timed(lambda: ops.splitbeam_complex(re, im, bt, prm, **kw), a.steps, a.warmup)
            torch.cuda.empty_cache()
            cc = np.zeros((C, 1, _lib.NCCOEF))
            cc[..., _lib.CC_RA], cc[..., _lib.CC_RB], cc[..., _lib.CC_PSCALE] = 8e-6, 750.0, 1.0
            cc[..., _lib.CC_SHIFT], cc[..., _lib.CC_ALPHA2], cc[..., _lib.CC_A] = 0.19, 0.02, -30.0
            ccd = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(cc, (C, P, _lib.NCCOEF)))).to(dev)
            sv_ms, sv_all = timed(lambda: ops.sv_complex(re, im, ccd, want_range=False, want_range_stats=True, **kw),
                                  a.steps, a.warmup)
            line("bb_pulse_compressed_f32_f64", (C, P, S, B), ms, all_ms, 32 + 16, taps=taps, method=form,
                 compute_Sv_bb_ms=round(sv_ms, 3), compute_Sv_bb_passes_ms=sv_all, ratio_to_compute_Sv_bb=round(ms / sv_ms, 3))


if __name__ == "__main__":
    main()
