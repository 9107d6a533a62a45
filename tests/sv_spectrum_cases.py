"""The fixtures of the Sv-spectrum tests, in NumPy: the scene of ``target_spectra_cases.scene`` (C = 2 with replicas of
177 and 113 taps, P = 3, S = 400, a NaN tail of 40 samples on ping 1, the mixed-sector patch on (0, 0)), its
frequency-varying parameter tables plus a row for the equivalent beam angle, with and without two filter intervals, and
one variant with a ping no filter interval covers.  tests/test_sv_spectrum_host.py holds their conditioning;
tests/test_gpu_sv_spectrum.py runs the kernel on them."""
import functools

import numpy as np
import sv_spectrum_ref as R
import target_spectra_cases as TK
import target_spectra_ref as TR

C, P, S, TAIL, DT = TK.C, TK.P, TK.S, TK.TAIL, TK.DT
# The band margin of the fixtures: 0.25, not the default 0.1.  The stand-in filters of the scene pass f_c +- 0.3 bandwidths;
# with a margin of 0.1 the outermost frequencies lie 60 dB down their skirts, where cells off the echoes have Fourier sums
# with kappa up to 1e4 (tests/test_sv_spectrum_host.py holds the bound the kernel tolerance rests on).
MARGIN = 0.25
UNCOVERED = (1, 0)  # the (channel, ping) of the ``uncovered`` variant whose replica_id is -1

# (B, dtype, N_w, hop or None for the default, F, window, two filter intervals): the sweep of the kernel test.  Every
# value the issue lists appears -- B in {4, 3}, float32 and float64 cubes, N_w in {2, 16, 64, 255, 400}, hop in {1, the
# default, N_w, N_w + 7}, F in {1, 41, 257}, both windows, two filter intervals -- and the seams: hop = 1 at N_w = 2 gives
# M = 399 cells in four tiles of 100, 100, 100 and 99 (more than two tiles, M no multiple of the tile); N_w = 400 = S is a
# single cell; hop > N_w leaves gaps between the cells; N_w = hop = 40 has a cell that ends on the last valid sample in
# front of the NaN tail of ping 1 and the next one inside it.
#
# What is NOT in the sweep, and why: hop = 1 (or any hop that puts a cell on the last 40 samples of a row or in front of a
# NaN tail) with N_w from 16 to 64.  There the compression sees only the first taps of the replica -- the start of the
# taper at f_start -- so ps is a smooth sequence whose energy lies outside the analysed band, and the in-band Fourier sums
# cancel to kappa of 4e3 .. 2e4 whatever the band margin, the noise level or the window (measured: Hann and rectangular,
# N_w 16, 32, 64; kappa (N_w + L) 2**-52 = 2e-10 .. 1e-9).  The conditioning test forbids leaving cells out of a compared
# case, so such cases are not compared at all; N_w = 2 at hop = 1 walks every sample of the rows, the ends included.
SWEEP = (
    (4, "float64", 2, 1, 41, "rectangular", False),
    (3, "float32", 2, 9, 1, "rectangular", False),
    (4, "float32", 64, None, 257, "hann", False),
    (3, "float64", 64, 64, 41, "rectangular", False),
    (4, "float64", 255, None, 41, "hann", False),
    (3, "float64", 255, 262, 1, "hann", False),
    (4, "float64", 400, None, 257, "hann", False),
    (4, "float32", 16, 23, 41, "rectangular", True),
    (4, "float64", 64, None, 41, "hann", True),
    (3, "float32", 255, 255, 257, "rectangular", False),
    (4, "float64", 16, 23, 257, "hann", False),
    (4, "float64", 40, 40, 41, "hann", False),
)
SEAM = SWEEP[-1]  # N_w = hop = 40: cell 8 of ping 1 ends on sample S - TAIL - 1, cell 9 lies in the NaN tail
UNCOVERED_CASE = (4, "float64", 64, None, 41, "hann", False)  # ... run with ``uncovered=True``


def scene(B=4, dtype="float64"):
    return TK.scene(B, dtype)


def hop_of(Nw, hop):
    return -(-Nw // 2) if hop is None else hop


def params(d, F, replicas, two_intervals=False, uncovered=False, margin=MARGIN):
    """(fparams (R, 5, F), pparams (4, C, P), rep_dt (R,), replica list, replica_id or None): parameters that vary with
    frequency the way ``target_spectra_cases.params`` makes them (absorption by Francois & Garrison, a gain rising with
    log f, z_et drifting) with the equivalent beam angle psi + 20 log10(f_n / f) as the fifth row, on the grid of band
    margin ``margin``; the sample interval is the fourth per-ping row.  ``two_intervals``: the last ping of every channel
    belongs to a second replica per channel, the first one shortened by 9 taps and scaled.  ``uncovered``: the ping
    UNCOVERED has replica_id -1."""
    from echopype_amd import synth

    C, P = d["backscatter_r"].shape[:2]  # (the long pings of LONG have shapes of their own)
    fn = d["frequency_nominal"]
    freq = TR.grid(d["f_start"], d["f_stop"], F, margin)
    fparams = np.stack([np.stack([f, np.asarray(synth.fg_absorption(f), dtype=np.float64),
                                  d["gain"][c] + 20 * np.log10(f / fn[c]) * 0.5, 75.0 + 5e-5 * (f - fn[c]),
                                  d["psi"][c] + 20 * np.log10(fn[c] / f)]) for c, f in enumerate(freq)])
    reps = list(replicas)
    rid = None
    if two_intervals:
        reps = reps + [(1.25 * r[:-9]).astype(np.complex64) for r in replicas]
        fparams = np.concatenate([fparams, fparams])
        rid = np.repeat(np.arange(C, dtype=np.int32)[:, None], P, axis=1)
        rid[:, P - 1] += C
    if uncovered:
        rid = np.repeat(np.arange(C, dtype=np.int32)[:, None], P, axis=1) if rid is None else rid
        rid[UNCOVERED] = -1
    pparams = np.stack([np.repeat(d["transmit_power"][:, None], P, axis=1), np.asarray(d["sound_speed"], dtype=np.float64),
                        np.repeat(d["z_er"][:, None], P, axis=1), np.asarray(d["sample_interval"], dtype=np.float64)])
    return np.ascontiguousarray(fparams), np.ascontiguousarray(pparams.astype(np.float64)), np.full(len(reps), DT), reps, rid


# Longer pings, for the paths of the kernel that S = 400 cannot reach: a lane compresses J = ceil(span / 256) samples of
# the tile's span side by side, and S = 400 gives J <= 2.  (S, J): one channel, two pings without a NaN tail, N_w = hop =
# 64 in a single tile whose span is 64 M; the last cell ends 63 samples in front of the row's end (see SWEEP for why; 16 to
# 28 samples were measured not to be enough: kappa 2e3 .. 6e3), and the mixed-sector patch of (0, 0) puts that ping on the
# per-sector path.
LONG = ((831, 3), (1087, 4), (1279, 5))
LONG_CASE = (64, 64, 41, "hann")  # N_w, hop, F, window


@functools.lru_cache(maxsize=None)
def long_scene(S):
    from echopype_amd import synth

    d, replicas, _ = synth.target_spectra_scene(C=1, P=2, S=S, B=4, tail=0)
    for a in (d["backscatter_r"], d["backscatter_i"]):
        a.setflags(write=False)
    return d, replicas


@functools.lru_cache(maxsize=None)
def long_reference(S):
    d, replicas = long_scene(S)
    Nw, hop, F, kind = LONG_CASE
    fparams, pparams, rep_dt, reps, rid = params(d, F, replicas)
    want = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, Nw, hop_of(Nw, hop), kind)
    for v in want.values():
        v.setflags(write=False)
    return want


_COMPRESSED = {}


def reference(B, dtype, Nw, hop, F, kind="hann", two_intervals=False, uncovered=False):
    """The oracle on a fixture, computed once per combination and shared (the arrays are read-only)."""
    return _reference(B, str(np.dtype(dtype)), Nw, hop_of(Nw, hop), F, kind, two_intervals, uncovered)


@functools.lru_cache(maxsize=None)
def _reference(B, dtype, Nw, hop, F, kind, two_intervals, uncovered):
    d, replicas, _ = scene(B, dtype)
    fparams, pparams, rep_dt, reps, rid = params(d, F, replicas, two_intervals, uncovered)
    keep = _COMPRESSED.setdefault((B, dtype, two_intervals), {})  # (the compressed rows do not depend on N_w, hop, F)
    want = R.sv_spectrum(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, Nw, hop, kind, keep)
    for v in want.values():
        v.setflags(write=False)
    return want
