"""Named raw-sample volumes with +-inf (and overflowing) power samples for the calibrate -> grid routes, and what the
CPU oracle makes of them (pure NumPy: ``synth`` builds the file, ``oracle_chain.ek60`` / ``oracle.commongrid`` /
``oracle.clean`` compute every expectation).

The rule under test (calibrate/range.py:145-147 of the reference, oracle/calibrate.py ``range_ek``): echo_range is NaN
where the raw sample is NULL, nowhere else.  A raw sample of +-inf keeps its range -- it counts in the nanmin / nanmax that
size the MVBS grid, it is no NaN coordinate -- and its Sv is +-inf: 10^(Sv/10) = +inf or 0, a term of its bin's mean.

Shapes: C = 2, P = 24 pings 1 s apart, S in {255, 1024, 1028, 1030}.  255: odd and unaligned, the scalar kernels.  1024:
exactly one chunk of the streaming kernels (4 wavefronts x 256 samples; lane l of a wavefront owns pair A at base + 2l
and pair B at base + 128 + 2l).  1030: a chunk and a 6-sample tail -- not a multiple of 4, so the generic kernels take
it; 1028 is the same tail for the specialised kernels, which need S % 4 == 0.  Time bins of 6 s keep a time bin within
8 pings, the longest the planner reduces in one stage (block_reduce.hip ``make_plan``): the specialised kernels serve.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import oracle_chain as oc
from oracle import clean as oclean
from oracle import commongrid as ogrid

C, P = 2, 24
SIZES = (255, 1024, 1028, 1030)
TBIN = "6s"
RBIN = "4.9m"         # 4.9 m / 0.192 m per sample = 1225 / 48: no sample of these volumes lies on a bin edge
PING_NUM, RSN = 6, 50  # remove_background_noise / index binning blocks (S is no multiple of 50: padded tails)
NAMES = ("last_column", "first_columns", "one_lane", "whole_ping", "bin_classes", "overflow")
F32_MAX_DB = 10 * np.log10(float(np.finfo(np.float32).max))   # 385.3 dB: 10^(Sv/10) overflows float32 above
F64_MAX_DB = 10 * np.log10(np.finfo(np.float64).max)          # 3082.5 dB: ... float64
# Sv the ``overflow`` case aims at, either side of each threshold and far from it (0.3 dB: thousands of float32 ulps)
OVERFLOW_F64 = (3060.0, 3080.0, 3082.0, 3083.0, 3090.0, 3200.0)
OVERFLOW_F32 = (370.0, 384.0, 385.0, 385.6, 390.0, 400.0)
BIN_CLASS_RBINS = dict(only_neg=2, neg_and_finite=4, pos_and_neg=6, pos_and_nan=8)
BIN_CLASS_CELL = (0, 1)   # (channel, time bin) of the cells above


@dataclass
class Case:
    name: str
    S: int
    with_nan: bool
    d: dict                       # the synth file (``backscatter_r`` holds the case)
    range_bin: str
    ping_time_bin: str = TBIN
    marks: dict = field(default_factory=dict)   # where the case put what (per case, see ``build``)

    @property
    def raw(self):
        return self.d["backscatter_r"]

    @property
    def has_nan(self):
        return bool(np.isnan(self.raw).any())

    @property
    def key(self):
        return self.name, self.S, self.with_nan

    # -- the oracle's outputs (float64), computed once per case and never written to ---------------------------------
    def sv_er(self):
        return _sv_er(*self.key)

    def mvbs(self, skipna=True, closed="left", on="Sv"):
        return _mvbs(*self.key, skipna, closed, on)

    def clean(self, noise_max=None):
        return _clean(*self.key, noise_max)

    def mvbs_index(self):
        return _mvbs_index(*self.key)


def _base(S):
    """The synth file with its NaN tails filled: every raw sample finite."""
    from echopype_amd import synth

    d = synth.ek60_numpy(C, P, S, seed=4200 + S)
    raw = d["backscatter_r"]
    raw[np.isnan(raw)] = np.float32(-60.0)
    return d


def _range_of(d):
    """echo_range of the file with every sample valid (the oracle's own: range_ek on a NaN-free array)."""
    return oc.ek60({**d, "backscatter_r": np.zeros_like(d["backscatter_r"])}, "Sv")


def _grid_labels(d, er, range_bin):
    """(time bin of every ping, range bin of every sample) under compute_MVBS's binning."""
    r_edges = ogrid.range_edges(er, ogrid.parse_range_bin(range_bin))
    t_edges = ogrid.ping_edges(d["ping_time"], TBIN)
    return ogrid.bin_index(d["ping_time"], t_edges), ogrid.bin_index(er, r_edges)


def _last_column_bin(er):
    """A range bin for which the largest range of the volume lies beyond a bin edge its neighbour does not reach:
    the edge k * bin is put half-way between the two columns' largest ranges, k = 40."""
    hi, lo = float(er[:, :, -1].max()), float(er[:, :, -2].max())
    b = round((hi + lo) / 2 / 40, 3)
    assert lo < 40 * b < hi
    return f"{b}m"


@functools.lru_cache(maxsize=None)
def build(name, S, with_nan=False):
    d = _base(S)
    raw = d["backscatter_r"]
    inf = np.float32(np.inf)
    marks, range_bin = {}, RBIN
    if name == "last_column":      # the range maximum of the volume, every ping
        raw[:, :, S - 1] = inf
        range_bin = _last_column_bin(_range_of(d)[1])
    elif name == "first_columns":  # the range minimum, next to the R' <= 0 samples (s = 0, 1, 2 for an EK60 row)
        raw[:, :, 0:4] = -inf
    elif name == "one_lane":       # one +inf in pair A, one -inf in pair B of ONE wavefront of ONE ping
        w = 2 if S >= 768 else 0
        marks = dict(channel=1, ping=7, wavefront=w, pos=256 * w + 2 * 17, neg=256 * w + 128 + 2 * 40 + 1)
        raw[1, 7, marks["pos"]] = inf
        raw[1, 7, marks["neg"]] = -inf
    elif name == "whole_ping":
        raw[:, 5, :] = inf
        raw[:, 13, :] = -inf
        marks = dict(pos_ping=5, neg_ping=13)
    elif name == "bin_classes":
        _, er = _range_of(d)
        it, ir = _grid_labels(d, er, RBIN)
        c, tb = BIN_CLASS_CELL
        cell = {k: (it[:, None] == tb) & (ir[c] == rb) for k, rb in BIN_CLASS_RBINS.items()}
        pick = {k: np.argwhere(m) for k, m in cell.items()}          # (ping, sample) pairs, row-major
        raw[c][cell["only_neg"]] = -inf
        for p, s in pick["neg_and_finite"][[1, 7]]:
            raw[c, p, s] = -inf
        (p0, s0), (p1, s1) = pick["pos_and_neg"][[3, 20]]
        raw[c, p0, s0], raw[c, p1, s1] = inf, -inf
        p0, s0 = pick["pos_and_nan"][5]
        raw[c, p0, s0] = inf
        for p, s in pick["pos_and_nan"][[0, 11, 30]]:
            raw[c, p, s] = np.nan
        marks = dict(channel=c, time_bin=tb, **BIN_CLASS_RBINS)
    elif name == "overflow":       # finite raw samples: Sv finite, 10^(Sv/10) beyond the working type
        sv0, er = _range_of(d)     # Sv of raw = 0: the sample's Sv is raw + sv0
        it, ir = _grid_labels(d, er, RBIN)
        spots = []

        def put(c, p, rb, target, k=0):
            s = int(np.flatnonzero(ir[c, p] == rb)[10 + k])          # well inside the bin
            raw[c, p, s] = np.float32(target - sv0[c, p, s])
            spots.append((c, p, s, float(target)))

        for j, t in enumerate(OVERFLOW_F64):                         # one per range bin: time bin 0
            put(0, 2, 1 + j, t)
        for j, t in enumerate(OVERFLOW_F32):                         # time bin 1
            put(0, 8, 1 + j, t)
        for k in (0, 1):                                             # two terms whose SUM overflows: time bins 2, 3
            put(1, 14, 3, 3082.0, k)
            put(1, 20, 3, 385.0, k)
        marks = dict(spots=spots)
    else:
        raise KeyError(name)
    if with_nan:                   # 5 % NaN among the finite samples: the case's own samples stay
        rng = np.random.default_rng(77 + S)
        raw[(rng.random(raw.shape) < 0.05) & np.isfinite(raw)] = np.nan
    raw.setflags(write=False)
    return Case(name, S, with_nan, d, range_bin, marks=marks)


def all_cases(sizes=SIZES):
    return [(n, S, w) for n in NAMES for S in sizes for w in (False, True)]


def case_id(k):
    return f"{k[0]}-S{k[1]}{'-nan' if k[2] else ''}"


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def _sv_er(name, S, with_nan):
    with np.errstate(over="ignore", invalid="ignore"):
        return _ro(*oc.ek60(build(name, S, with_nan).d, "Sv"))


@functools.lru_cache(maxsize=None)
def _clean(name, S, with_nan, noise_max):
    cs = build(name, S, with_nan)
    sv, er = _sv_er(name, S, with_nan)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return _ro(*oclean.remove_background_noise(sv, er, cs.d["absorption_indicative"], PING_NUM, RSN, noise_max,
                                                   "3.0dB"))


@functools.lru_cache(maxsize=None)
def _mvbs(name, S, with_nan, skipna, closed, on):
    cs = build(name, S, with_nan)
    sv, er = _sv_er(name, S, with_nan)
    if on == "Sv_corrected":
        sv = _clean(name, S, with_nan, None)[1]
    with np.errstate(over="ignore", invalid="ignore"):
        return _ro(*ogrid.compute_MVBS(sv, er, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin, skipna=skipna,
                                       closed=closed))


@functools.lru_cache(maxsize=None)
def _mvbs_index(name, S, with_nan):
    sv, er = _sv_er(name, S, with_nan)
    with np.errstate(over="ignore", invalid="ignore"):
        return _ro(*ogrid.compute_MVBS_index_binning(sv, er, RSN, PING_NUM))


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN of every element."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))
