"""The fixtures of the target-spectra tests, in NumPy: the scene of ``synth.target_spectra_scene`` (C = 2 with replicas
of 177 and 113 taps, P = 3, S = 400), hand-made parameter tables that vary with frequency, and hand-made target tables.
tests/test_target_spectra_host.py holds their conditioning; tests/test_gpu_target_spectra.py runs the kernel on them."""
import functools

import numpy as np
import target_spectra_ref as R

C, P, S = 2, 3, 400
TAIL = 40
DT = 8e-6
H_ALL = (0, 1, 16, 127)
F_ALL = (1, 41, 257)


@functools.lru_cache(maxsize=None)
def scene(B=4, dtype="float64"):
    from echopype_amd import synth

    d, replicas, echoes = synth.target_spectra_scene(C=C, P=P, S=S, B=B, dtype=np.dtype(dtype), tail=TAIL)
    for a in (d["backscatter_r"], d["backscatter_i"]):
        a.setflags(write=False)
    return d, replicas, echoes


def params(d, F, replicas, two_intervals=False):
    """(fparams (R, 8, F), pparams (3, C, P), rep_dt (R,), replica list, replica_id or None): parameters that vary with
    frequency the way a calibrated file's do (absorption by Francois & Garrison, a gain rising with log f, beamwidths
    falling with 1 / f, offsets drifting); with ``two_intervals`` the last ping of every channel belongs to a second
    replica per channel, the first one shortened by 9 taps and scaled."""
    from echopype_amd import synth

    fn = d["frequency_nominal"]
    freq = R.grid(d["f_start"], d["f_stop"], F)
    rows = []
    for c in range(C):
        f = freq[c]
        rows.append(np.stack([f, np.asarray(synth.fg_absorption(f), dtype=np.float64),
                              d["gain"][c] + 20 * np.log10(f / fn[c]) * 0.5, 75.0 + 5e-5 * (f - fn[c]),
                              d["beamwidth_alongship"][c] * fn[c] / f, d["beamwidth_athwartship"][c] * fn[c] / f,
                              d["angle_offset_alongship"][c] + 0.02 * (f / fn[c] - 1),
                              d["angle_offset_athwartship"][c] - 0.03 * (f / fn[c] - 1)]))
    fparams = np.stack(rows)
    reps = list(replicas)
    rid = None
    if two_intervals:
        reps = reps + [(1.25 * r[:-9]).astype(np.complex64) for r in replicas]
        fparams = np.concatenate([fparams, fparams])
        rid = np.repeat(np.arange(C, dtype=np.int32)[:, None], P, axis=1)
        rid[:, P - 1] += C
    pparams = np.stack([np.repeat(d["transmit_power"][:, None], P, axis=1), np.asarray(d["sound_speed"], dtype=np.float64),
                        np.repeat(d["z_er"][:, None], P, axis=1)]).astype(np.float64)
    return np.ascontiguousarray(fparams), np.ascontiguousarray(pparams), np.full(len(reps), DT), reps, rid


def table(echoes, replicas, channels=(0, 1), extra=True):
    """A hand-made target table (the table's channel k is the cube's ``channels[k]``), rows at ranges and angles of
    their own.  First the SIGNAL rows, ``n_signal(...)`` of them: one at the peak of every whole planted echo -- among
    them the one at sample 0, the one with the mixed-sector patch inside, the one in front of the NaN tail and the one
    that ends with the row.  With ``extra`` then the EDGE rows, two per channel: the last sample S - 1, whose replica
    zero-fills past the row, and a sample inside the NaN tail (a small window lies in it completely); then rows with a
    NaN angle, a NaN and a non-positive range, and rows whose indices are outside the cube."""
    rows = []
    for k, c in enumerate(channels):
        for (ce, p, s, K, e_al, e_at) in echoes:
            if ce == c and s + replicas[c].size <= S:
                rows.append((k, p, s, 5.0 + 0.13 * s, 0.01 * e_al, -0.02 * e_at))
    if extra:
        for k, c in enumerate(channels):
            rows += [(k, P - 1, S - 1, 57.0, -0.4, 0.2), (k, 1, S - TAIL + 12, 40.0, 0.5, 0.5)]
        for k, c in enumerate(channels):
            rows += [(k, 0, S // 2, 20.0, np.nan, 0.3), (k, 0, S // 2, 20.0, 0.3, np.nan),
                     (k, 0, S // 2, np.nan, 0.3, 0.3), (k, 0, S // 2, 0.0, 0.3, 0.3), (k, 0, S // 2, -3.0, 0.3, 0.3)]
        rows += [(-1, 0, 117, 20.0, 0.0, 0.0), (len(channels), 0, 117, 20.0, 0.0, 0.0), (0, -1, 117, 20.0, 0.0, 0.0),
                 (0, P, 117, 20.0, 0.0, 0.0), (0, 0, -5, 20.0, 0.0, 0.0), (0, 0, S, 20.0, 0.0, 0.0),
                 (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 20.0, 0.0, 0.0)]
    cols = list(zip(*rows)) if rows else [[]] * 6
    return dict(channel_index=np.asarray(cols[0], dtype=np.int32), ping_index=np.asarray(cols[1], dtype=np.int32),
                range_sample=np.asarray(cols[2], dtype=np.int32), target_range=np.asarray(cols[3], dtype=np.float64),
                angle_alongship=np.asarray(cols[4], dtype=np.float64),
                angle_athwartship=np.asarray(cols[5], dtype=np.float64))


def n_signal(echoes, replicas, channels=(0, 1)):
    """The number of signal rows ``table`` starts with; the 2 * len(channels) edge rows follow them."""
    return sum(1 for c in channels for (ce, _, s, *_) in echoes if ce == c and s + replicas[c].size <= S)


def reference(B, dtype, h, F, two_intervals=False, channels=(0, 1), extra=True):
    """The oracle on a fixture, computed once per combination and shared (the arrays are read-only)."""
    return _reference(B, str(np.dtype(dtype)), h, F, two_intervals, tuple(channels), extra)


@functools.lru_cache(maxsize=None)
def _reference(B, dtype, h, F, two_intervals, channels, extra):
    d, replicas, echoes = scene(B, dtype)
    fparams, pparams, rep_dt, reps, rid = params(d, F, replicas, two_intervals)
    tab = table(echoes, replicas, channels, extra)
    want = R.spectra(d["backscatter_r"], d["backscatter_i"], reps, rid, rep_dt, fparams, pparams, h, list(channels), tab)
    for v in want.values():
        v.setflags(write=False)
    return want
