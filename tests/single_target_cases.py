"""The scenes the single-target tests share: built once, judged once by the NumPy restatement, never modified.
``test_single_target_host.py`` checks on the restatement alone that every scene exercises what it is there for;
``test_gpu_single_target.py`` compares the device with it."""
import functools

import numpy as np
import single_target_ref as R

from echopype_amd import ops, synth

TILE = ops.SINGLE_TARGET_TILE  # samples of a row the kernel holds at a time: envelopes must cross its multiples
C, P = 2, 37
# sizes with their own path: the edges of a row (1, 2, 3), of a wave (64) and of the tile, a row of several tiles
TINY = (1, 2, 3)
SIZES = TINY + (63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 452)
PARAMS = dict(R.DEFAULTS)
BEAMWIDTH_AL = 7.0 + 0.01 * np.arange(C * P, dtype=np.float64).reshape(C, P)  # (channel, ping_time)
BEAMWIDTH_AT = np.array([7.1, 6.8])                                             # (channel,)
OFFSET_AL = np.array([0.02, -0.05])
OFFSET_AT = np.array([-0.07, 0.04])


def spp_of(S):
    """Samples per pulse (channel, ping_time), different for every channel and ping; one NaN and one 0 (both reject
    every candidate of their row under rule 1).  Rows of up to three samples get pulses short enough to be found."""
    if S in TINY:
        spp = np.array([1.0, 2.0])[:, None] + 0.1 * (np.arange(P) % 3)[None, :]
    else:
        spp = np.array([4.0, 3.0])[:, None] + 0.5 * (np.arange(P) % 3)[None, :] + 0.01 * np.arange(P)[None, :]
    spp[0, 5] = np.nan
    spp[1, 7] = 0.0
    return spp


@functools.lru_cache(maxsize=None)
def scene(S, dtype="float64"):
    """-> dict of read-only arrays: TS and the angles (C, P, S) of ``dtype``, the range as ``range_cube`` (C, P, S, with
    NaNs), ``range_cs`` (C, S) and ``range_s`` (S,), and ``spp`` (C, P)."""
    chans = [synth.single_target_scene(P, S, seed=20261020 + 1000 * c + S, dtype=np.dtype(dtype), seam=TILE)
             for c in range(C)]
    d = {k: np.stack([ch[k] for ch in chans]) for k in ("TS", "angle_alongship", "angle_athwartship")}
    base = chans[0]["echo_range"].astype(np.float64)
    rng = np.random.default_rng(77 + S)
    cube = base[None, None, :] * (1.0 + 0.01 * np.arange(C))[:, None, None] + 0.001 * np.arange(P)[None, :, None]
    cube[rng.random(cube.shape) < 0.05] = np.nan
    d["range_cube"] = cube.astype(dtype)
    d["range_cs"] = np.ascontiguousarray(cube[:, 3, :]).astype(dtype)
    d["range_s"] = base.astype(dtype)
    d["spp"] = spp_of(S)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def expected(S, dtype="float64", range_kind="cube", channels=None):
    """The restatement's verdict on ``scene(S, dtype)`` with the range variant ``range_kind`` ("cube", "cs", "s"),
    on all channels or on the tuple ``channels`` of channel indices."""
    d = scene(S, dtype)
    sel = list(range(C)) if channels is None else list(channels)
    r = d["range_" + range_kind]
    r = {"cube": r[sel] if range_kind == "cube" else None, "cs": r[sel][:, None, :] if range_kind == "cs" else None,
         "s": r}[range_kind]
    return R.detect(d["TS"][sel], d["angle_alongship"][sel], d["angle_athwartship"][sel], r, d["spp"][sel],
                    BEAMWIDTH_AL[sel], BEAMWIDTH_AT[sel], OFFSET_AL[sel], OFFSET_AT[sel], PARAMS)


# ---- long pulses: envelopes past what a lane keeps in registers, and past the halo of the kernel's tile ---------------
KEEP = 8    # samples of an envelope the kernel fetches in one go (kKeep in csrc/single_target.hip): the rest in loops
HALO = 64   # samples beside a tile the kernel holds in LDS (kHalo): a longer walk goes on in global memory
LONG_S = 2 * TILE + 452
LONG_SCALE = (3, 32)  # channel 0: spp about 12, admitted envelopes of 9 .. 19 samples; channel 1: spp about 125, 84 .. 193


def long_spp():
    return np.stack([11.0 + 0.05 * np.arange(P), 120.0 + 0.25 * np.arange(P)])


@functools.lru_cache(maxsize=None)
def long_scene(dtype="float64"):
    """``scene`` with ``synth.single_target_scene(scale=...)``: everything stretched by 3 in channel 0, by 32 in
    channel 1, and the samples per pulse to match."""
    chans = [synth.single_target_scene(P, LONG_S, seed=20261120 + c, dtype=np.dtype(dtype), seam=TILE, scale=k)
             for c, k in enumerate(LONG_SCALE)]
    d = {k: np.stack([ch[k] for ch in chans]) for k in ("TS", "angle_alongship", "angle_athwartship")}
    cube = np.broadcast_to(chans[0]["echo_range"].astype(np.float64), (C, P, LONG_S)).copy()
    cube[np.random.default_rng(78).random(cube.shape) < 0.05] = np.nan
    cube[0, 2] = np.nan  # a ping without a range: its targets have none
    d["range_cube"] = cube.astype(dtype)
    d["spp"] = long_spp()
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def long_expected(dtype="float64"):
    d = long_scene(dtype)
    return R.detect(d["TS"], d["angle_alongship"], d["angle_athwartship"], d["range_cube"], d["spp"], BEAMWIDTH_AL,
                    BEAMWIDTH_AT, OFFSET_AL, OFFSET_AT, PARAMS)


# ---- host-resident inputs with one beam geometry for all channels (test_host_inputs_and_samples_per_pulse_per_channel)
HOST_BEAM = (7.0, 6.5, 0.1, -0.1)  # beamwidth alongship / athwartship, offset alongship / athwartship
HOST_SPP = (4.0, (4.0, 2.5))        # as a scalar, and one per channel


@functools.lru_cache(maxsize=None)
def host_expected(spp):
    d = scene(64, "float32")
    return R.detect(d["TS"], d["angle_alongship"], d["angle_athwartship"], d["range_s"], np.asarray(spp), *HOST_BEAM,
                    PARAMS)
