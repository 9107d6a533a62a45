#!/usr/bin/env python3
"""Generate tests/golden/ref_splitbeam_goldens.npz by EXECUTING THE REFERENCE'S OWN split-beam code
(consolidate/split_beam_angle.py: get_angle_power_samples, get_angle_complex_samples with and without pc_params,
_compute_angle_from_complex) over oracle/xr_shim.py.  Authoring container only: needs the reference checkout.

The loaders of oracle/gen_chain_goldens.py set up the reference's packages over the shim (they are imported, not
edited).  Two additions the split-beam module needs are made here: a stub ``dask`` / ``dask.array`` with an ``Array``
class (split_beam_angle.py:95 asks ``isinstance(sens[0].data, da.Array)``) and ``real`` / ``imag`` properties of the
shim's DataArray (np.real / np.imag read them).  get_transmit_signal reads file parameters: it is replaced by the
replicas the reference's own leafs build (tapered_chirp + filter_decimate_chirp), as gen_chain_goldens.py does.

Also stored: the reference's signature of consolidate.add_splitbeam_angle, read with the ast helper of
oracle/gen_ref_signatures.py.  Output = data only (seeded inputs, the reference's outputs)."""
import ast
import json
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_ref_signatures  # noqa: E402
import xr_shim  # noqa: E402
from gen_chain_goldens import load_reference_calibrators  # noqa: E402
from gen_goldens import REF, _load  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_splitbeam_goldens.npz")
DA, DS = xr_shim.DataArray, xr_shim.Dataset
DIMS4 = ["channel", "ping_time", "range_sample", "beam"]


def load_reference_splitbeam():
    _, _, _, ekc = load_reference_calibrators()
    dask = types.ModuleType("dask")
    dask_array = types.ModuleType("dask.array")

    class Array:  # nothing here is a dask array
        pass

    dask_array.Array = Array
    dask.array = dask_array
    sys.modules["dask"], sys.modules["dask.array"] = dask, dask_array
    DA.real = property(lambda self: DA(np.real(self.data), self.coords, self.dims))
    DA.imag = property(lambda self: DA(np.imag(self.data), self.coords, self.dims))
    # a scalar label (the mixed-beam-type branch selects one channel at a time, split_beam_angle.py:236-250): the
    # position along the dimension, which drops it as xarray does
    shim_sel = DA.sel

    def sel(self, drop=False, **ix):
        scalar = {d: v for d, v in ix.items() if not isinstance(v, slice) and np.ndim(v) == 0}
        if not scalar:
            return shim_sel(self, drop=drop, **ix)
        pos = {d: int(np.flatnonzero(np.asarray(self.coords[d]).astype(str) == str(v))[0]) for d, v in scalar.items()}
        rest = {d: v for d, v in ix.items() if d not in scalar}
        out = self.isel(**pos)
        return shim_sel(out, drop=drop, **rest) if rest else out

    DA.sel = sel
    DA.__int__ = lambda self: int(np.asarray(self.data).reshape(()))
    pkg = types.ModuleType("echopype.consolidate")
    pkg.__path__ = [f"{REF}/consolidate"]
    sys.modules[pkg.__name__] = pkg
    sba = _load("echopype.consolidate.split_beam_angle", f"{REF}/consolidate/split_beam_angle.py")
    return sba, ekc


def reference_signature():
    tree = ast.parse(open(os.path.join(REF, "consolidate", "api.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "add_splitbeam_angle")
    return json.dumps({"params": gen_ref_signatures.params(fn), "line": fn.lineno, "file": "consolidate/api.py"})


def _chans(C):
    return np.array([f"ch{i}" for i in range(C)])


def _pings(P):
    return np.datetime64("2026-10-01T00:00:00", "ns") + np.arange(P) * np.timedelta64(1, "s")


def _param(v, chans, pings):
    v = np.asarray(v, float)
    if v.ndim == 1:
        return DA(v, {"channel": chans}, ["channel"])
    return DA(v, {"channel": chans, "ping_time": pings}, ["channel", "ping_time"])


def _angle_params(g, tag, chans, pings, sens_al, sens_at, off_al, off_at):
    for k, v in (("sens_al", sens_al), ("sens_at", sens_at), ("off_al", off_al), ("off_at", off_at)):
        g[f"{tag}_{k}"] = np.asarray(v, float)
    return {"angle_sensitivity_alongship": _param(sens_al, chans, pings),
            "angle_sensitivity_athwartship": _param(sens_at, chans, pings),
            "angle_offset_alongship": _param(off_al, chans, pings),
            "angle_offset_athwartship": _param(off_at, chans, pings)}


def _out(da):
    return np.asarray(da.transpose("channel", "ping_time", "range_sample").data, dtype=np.float64)


def power_case(sba, g, tag, C, P, S, seed, nan_pad, per_ping):
    rng = np.random.default_rng(seed)
    chans, pings = _chans(C), _pings(P)
    beam = DS(coords={"channel": chans, "ping_time": pings, "range_sample": np.arange(S)})
    for k in ("angle_alongship", "angle_athwartship"):
        a = rng.integers(-128, 128, (C, P, S)).astype(np.int8)
        if nan_pad:  # NaN-padded short pings turn the planes into floats (convert/parse_base.py:688)
            a = a.astype(np.float32)
            a[:, 1, S - 9:] = np.nan
            a[0, P - 1, S // 2:] = np.nan
        g[f"{tag}_{k}"] = a
        beam[k] = DA(a, {"channel": chans, "ping_time": pings, "range_sample": np.arange(S)},
                     ["channel", "ping_time", "range_sample"])
    beam["beam_type"] = DA(np.array([1] * (C - 1) + [0]), {"channel": chans}, ["channel"])
    shape = (C, P) if per_ping else (C,)
    prm = _angle_params(g, tag, chans, pings, 21.0 + rng.random(shape) * 3, 22.0 + rng.random(shape) * 3,
                        rng.uniform(-0.2, 0.2, shape), rng.uniform(-0.2, 0.2, shape))
    theta, phi = sba.get_angle_power_samples(beam, prm)
    g[f"{tag}_theta"], g[f"{tag}_phi"] = _out(theta), _out(phi)


def complex_samples(rng, C, P, S, B, replicas=None, echoes=()):
    """Complex sector samples: noise, replica-shaped echoes with a per-sector phase ramp at the given starts,
    NaN-padded pings, one sample with exactly one NaN sector, a sample with every sector NaN.  Every value lies on the
    grid 2^-12 (the noise on 2^-9): the reference and the tests read them as float32 planes, the fixture stores the
    int16 grid codes (encode_plane) -- the same float32 values in a fraction of the bytes."""
    x = (np.round(rng.standard_normal((C, P, S, B)) * 5.12) + 1j * np.round(rng.standard_normal((C, P, S, B)) * 5.12)) / 512
    ramp = np.exp(1j * np.array([0.0, 0.4, 1.1, 0.7])[:B])
    for c in range(C):
        for p in range(P):
            for k0 in echoes:
                r = replicas[c] if replicas is not None else np.ones(40)
                n = max(0, min(r.size, S - k0))
                x[c, p, k0:k0 + n, :] += (0.3 + 0.1 * p) * r[:n, None] * (ramp * np.exp(0.3j * c))[None, :]
    re = (np.round(x.real * QSCALE) / QSCALE).astype(np.float32)
    im = (np.round(x.imag * QSCALE) / QSCALE).astype(np.float32)
    for a in (re, im):
        a[:, P - 1, S - S // 5:, :] = np.nan  # a NaN-padded short ping
    re[0, 0, S // 3, 1] = np.nan              # exactly one NaN sector at one sample
    im[C - 1, 0, S // 2 + 1, B - 1] = np.nan  # an imag-only NaN in the last sector
    re[0, min(1, P - 1), 17, :] = np.nan      # every sector NaN
    im[0, min(1, P - 1), 17, :] = np.nan
    return re, im


QSCALE = 4096.0  # splitbeam_ref.load_goldens decodes with the same constants
QNAN = -32768


def encode_plane(a):
    """float32 plane on the 2^-12 grid -> int16 codes, QNAN for NaN (decoded exactly by splitbeam_ref.load_goldens)."""
    q = np.where(np.isnan(a), QNAN, np.round(np.nan_to_num(a) * QSCALE)).astype(np.int64)
    assert np.all(np.abs(q[q != QNAN]) < 32767)
    out = q.astype(np.int16)
    back = np.where(out == QNAN, np.nan, out.astype(np.float32) / np.float32(QSCALE))
    assert np.array_equal(back, a, equal_nan=True)
    return out


def _beam(re, im, chans, pings, beam_type):
    C, P, S, B = re.shape
    coords = {"channel": chans, "ping_time": pings, "range_sample": np.arange(S), "beam": np.arange(B)}
    beam = DS(coords=coords)
    beam["backscatter_r"] = DA(re, coords, DIMS4)
    beam["backscatter_i"] = DA(im, coords, DIMS4)
    beam["beam_type"] = DA(np.asarray(beam_type), {"channel": chans}, ["channel"])
    return beam


def complex_case(sba, g, tag, C, P, S, B, beam_type, seed, per_ping=False):
    rng = np.random.default_rng(seed)
    chans, pings = _chans(C), _pings(P)
    re, im = complex_samples(rng, C, P, S, B, echoes=(5, S // 2))
    g[f"{tag}_re"], g[f"{tag}_im"] = encode_plane(re), encode_plane(im)
    g[f"{tag}_beam_type"] = np.asarray(beam_type)
    shape = (C, P) if per_ping else (C,)
    prm = _angle_params(g, tag, chans, pings, 20.0 + 4 * rng.random(shape), 20.0 + 4 * rng.random(shape),
                        rng.uniform(-0.1, 0.1, shape), rng.uniform(-0.1, 0.1, shape))
    theta, phi = sba.get_angle_complex_samples(_beam(re, im, chans, pings, beam_type), prm)
    g[f"{tag}_theta"], g[f"{tag}_phi"] = _result(theta, chans), _result(phi, chans)


def _result(da, chans):
    """The reference's result aligned on the full channel list (the assignment into source_Sv aligns on channel: a
    skipped channel is an all-NaN row), float32 (the reference's angles are complex64 phases: float32 is their
    precision)."""
    have = [str(c) for c in np.asarray(da.coords["channel"])]
    out = _out(da)
    full = np.full((len(chans),) + out.shape[1:], np.nan)
    for i, c in enumerate(chans):
        if str(c) in have:
            full[i] = out[have.index(str(c))]
    return full.astype(np.float32)


def make_replica(ekc, fs, tau, f0, f1, coeff):
    y, _ = ekc.tapered_chirp(fs, np.array([tau]), np.array([0.05]), np.array([f0]), np.array([f1]))
    return ekc.filter_decimate_chirp(coeff, y, fs)


def pc_case(sba, ekc, g, tag, C, P, S, B, beam_type, seed, coeff, taus, echoes, intervals=None):
    """BB with pulse compression.  ``intervals``: [(first ping, end ping, per-channel pulse lengths)] -- a
    multi-filter_time file, run slice by slice (one replica per (channel, interval)) and put back together along
    ping_time."""
    rng = np.random.default_rng(seed)
    chans, pings = _chans(C), _pings(P)
    fs = 1.5e6
    f0, f1 = np.array([45e3, 90e3]), np.array([90e3, 170e3])
    ivals = [(slice(a, b), tt) for a, b, tt in (intervals or [(0, P, taus)])]
    reps = {}
    for k, (sl, tt) in enumerate(ivals):
        for c in range(C):
            reps[(k, c)] = make_replica(ekc, fs, tt[c], f0[c % 2], f1[c % 2], coeff)
    re, im = complex_samples(rng, C, P, S, B, [reps[(0, c)][0] for c in range(C)], echoes)
    g[f"{tag}_re"], g[f"{tag}_im"] = encode_plane(re), encode_plane(im)
    g[f"{tag}_beam_type"] = np.asarray(beam_type)
    rid = np.zeros((C, P), dtype=np.int32)
    for k, (sl, _) in enumerate(ivals):
        for c in range(C):
            g[f"{tag}_replica{k}_{c}"] = reps[(k, c)][0]
            rid[c, sl] = k * C + c
    g[f"{tag}_replica_id"] = rid
    prm = _angle_params(g, tag, chans, pings, 20.0 + 4 * rng.random(C), 20.0 + 4 * rng.random(C),
                        rng.uniform(-0.1, 0.1, C), rng.uniform(-0.1, 0.1, C))
    th = np.full((C, P, S), np.nan, np.float32)
    ph = np.full((C, P, S), np.nan, np.float32)
    for k, (sl, _) in enumerate(ivals):
        tx = {str(ch): reps[(k, c)][0] for c, ch in enumerate(chans)}
        tx_time = {str(ch): reps[(k, c)][1] for c, ch in enumerate(chans)}
        sba.get_transmit_signal = lambda *a, _tx=tx, _tt=tx_time, **kw: (_tx, _tt)
        pc_params = {"receiver_sampling_frequency": fs, "drop_last_hanning_zero": False}
        beam = _beam(re[:, sl], im[:, sl], chans, pings[sl], beam_type)
        theta, phi = sba.get_angle_complex_samples(beam, prm, pc_params)
        th[:, sl], ph[:, sl] = _result(theta, chans), _result(phi, chans)
    g[f"{tag}_theta"], g[f"{tag}_phi"] = th, ph


def main():
    logging.disable(logging.WARNING)
    sba, ekc = load_reference_splitbeam()
    g = {"signature": np.array(reference_signature())}
    power_case(sba, g, "pow_i8", 3, 5, 37, 1, nan_pad=False, per_ping=False)
    power_case(sba, g, "pow_f32", 2, 6, 41, 2, nan_pad=True, per_ping=True)
    complex_case(sba, g, "cx_bt1", 2, 3, 160, 4, [1, 1], 3)
    complex_case(sba, g, "cx_bt17", 2, 3, 160, 3, [17, 17], 4, per_ping=True)
    for i, bt in enumerate((49, 65, 81)):
        complex_case(sba, g, f"cx_bt{bt}", 2, 2, 120, 4, [bt, bt], 5 + i)
    complex_case(sba, g, "cx_mixed", 3, 2, 120, 4, [1, 49, 5], 8)  # type 5: skipped, an all-NaN row
    chain = dict(wbt_fil=(np.hanning(47) * np.exp(2j * np.pi * 0.045 * np.arange(47)) / 10).astype(np.complex64),
                 wbt_decifac=6, pc_fil=(np.hanning(91) * np.exp(2j * np.pi * 0.13 * np.arange(91)) / 20).astype(
                     np.complex64), pc_decifac=2)
    short = dict(wbt_fil=np.array([0.25, 0.5, 0.25], np.complex64), wbt_decifac=4,
                 pc_fil=np.array([0.5, 0.5], np.complex64), pc_decifac=2)
    long_ = dict(wbt_fil=np.array([0.25, 0.5, 0.25], np.complex64), wbt_decifac=2,
                 pc_fil=np.array([0.5, 0.5], np.complex64), pc_decifac=2)
    # FFT regime (16 .. 1024 taps), across the overlap-save seam (2048 - taps + 1 = 1872 outputs per tile) and the
    # direct kernel's 2048-sample tile edge
    pc_case(sba, ekc, g, "pc_fft", 1, 2, 2300, 4, [1], 9, chain, [1.024e-3],
            echoes=(3, 1780, 1860, 1990, 2040, 2049, 2250))
    pc_case(sba, ekc, g, "pc_fft17", 1, 2, 500, 3, [17], 10, chain, [0.512e-3], echoes=(30, 300))
    # direct regime: a replica of fewer than 16 taps, and one of more than 1024 (pc_fft crosses the direct tile edge
    # when the tests force the direct form)
    pc_case(sba, ekc, g, "pc_short", 2, 2, 600, 4, [49, 1], 11, short, [0.05e-3, 0.04e-3], echoes=(10, 300, 590))
    pc_case(sba, ekc, g, "pc_long", 1, 1, 1600, 4, [1], 12, long_, [4.0e-3], echoes=(50, 600))
    # a multi-filter_time file: ping 0 and pings 1-2 were recorded with other pulses (one replica per (channel, interval))
    pc_case(sba, ekc, g, "pc_multi", 2, 3, 300, 4, [1, 81], 13, chain, None, echoes=(20, 150),
            intervals=[(0, 1, [1.024e-3, 0.512e-3]), (1, 3, [0.512e-3, 0.256e-3])])
    np.savez_compressed(OUT, **g)
    print("wrote", os.path.normpath(OUT), f"{os.path.getsize(OUT) / 1024:.1f} KiB,", len(g), "arrays")
    for k in sorted(g):
        if k.endswith("_theta"):
            t = g[k]
            taps = [g[r].size for r in g if r.startswith(k[:-6] + "_replica") and r[-2:] != "id"]
            print(f"  {k:16s} {t.shape} NaN {int(np.isnan(t).sum()):6d}  taps {taps}")


if __name__ == "__main__":
    main()
