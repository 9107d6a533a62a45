"""The seeded cases of the reversed-time tests, shared by scripts/gen_qc_goldens.py (which runs the reference's own
``_clean_reversed`` on the FIXTURE cases) and the host and GPU tests (which run the restatement and the package on them).
Everything is a function of the case's name: two calls give the same arrays.

A case is ``dict(t=datetime64 array in its own unit, win_len=int)``."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qc_reversed_time.npz")
T0_NS = int(np.datetime64("2023-11-14T22:13:20", "ns").astype(np.int64))  # 1.7e18 ns
MAX_WIN = 1024      # EPA_QC_MAX_WIN: the longest window the kernel serves
SCAN_TILE = 1024    # EPA_QC_SCAN_TILE: differences per workgroup of the rebuild
CARRY_THREADS = 256  # tiles the carry workgroup takes per round
MEDIAN_WAVES = 1024  # EPA_QC_MEDIAN_WAVES: wavefronts of the median launch


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def from_diffs(d, t0=1000, unit="ns"):
    """t0 and the running (wrapping) sum of the differences ``d`` -> datetime64[unit] (len(d) + 1,)."""
    d = np.asarray(d, dtype=np.int64)
    with np.errstate(over="ignore"):
        t = np.int64(t0) + np.concatenate([np.zeros(1, np.int64), np.cumsum(d)])
    return t.view(f"datetime64[{unit}]")


def irregular(rng, n, lo=5):
    """n distinct positive intervals in random order: a window shifted by one gives another median."""
    return rng.permutation(np.arange(lo, lo + 7 * n, 7, dtype=np.int64))


def one_reversal(name, ni, win_len, tail=6, back=-9):
    """A single reversal at difference ``ni`` behind irregular positive intervals, ``tail`` more intervals after it."""
    d = irregular(_rng(name), ni + 1 + tail)
    d[ni] = back
    return dict(t=from_diffs(d), win_len=win_len)


def _clip_cases():
    out = {}
    for w in (1, 4, 5):
        for ni in sorted({1, max(w - 1, 1), w, w + 1}):
            out[f"clip_w{w}_ni{ni}"] = (ni, w)
    return out


CLIP = _clip_cases()            # small windows: in the fixture
CLIP_CAP = {f"clip_w{MAX_WIN}_ni{ni}": (ni, MAX_WIN) for ni in (1, MAX_WIN - 1, MAX_WIN, MAX_WIN + 1)}  # GPU only

# differences written out: what each one is for stands beside it
LITERAL = {
    # the issue's worked example, t = [0, 10, 20, 15, 25, 35, 30, 40]
    "worked_w100": ([10, 10, -5, 10, 10, -5, 10], 100, 0),
    "worked_w2": ([10, 10, -5, 10, 10, -5, 10], 2, 0),
    # two reversals inside each other's windows: the window of reversal 4 holds the ORIGINAL -40 of reversal 2,
    # [7, 21, -40, 30] -> (7 + 21) / 2 = 14; with the substitute of reversal 2 (14) in its place: (14 + 21) / 2 = 17
    "nested_w4": ([7, 21, -40, 30, -2, 11, 13], 4, 1000),
    # ... and the window of reversal 3 holds the original -6 of reversal 2: [9, -6] -> 1; with its substitute 13: 11
    "nested_w2": ([17, 9, -6, -2, 11, 13], 2, 1000),
    # even windows whose middle pair sums to an odd number: positive, negative and both mixed-sign orders
    "even_odd_positive": ([3, 8, -1, 4], 2, 50),              # window [3, 8] -> 11 / 2 -> 5
    "even_odd_negative": ([10, -3, -8, -5, 7], 2, 50),        # window [-3, -8] -> -11 / 2 -> -5 (not -6)
    "even_mixed_positive": ([10, -3, 8, -1, 7], 2, 50),       # window [-3, 8] -> 5 / 2 -> 2
    "even_mixed_negative": ([10, -8, 3, -1, 7], 2, 50),       # window [-8, 3] -> -5 / 2 -> -2 (not -3)
    # a negative median stays negative: the result still steps backwards
    "negative_median": ([10, -30, -20, -25, 12, 9], 3, 500),
    # the reversal is the last difference; the reversal is difference 1 (a window of one)
    "last_difference": ([4, 9, 6, -3], 100, 0),
    "second_difference": ([4, -3, 6, 9], 100, 0),
    # equal values in the window: ties are broken by position, the median is that value
    "ties": ([5, 5, 7, 5, 7, 7, -2, 5], 6, 0),
}
ERRORS = {  # what the reference raises (and, for the first, the package too)
    "first_difference": ([-4, 9, 6, 3], 100),
    "no_reversal": ([4, 9, 6, 3], 100),
}
NAT_CASES = {  # exist_reversed_time only: a difference that touches a NaT does not count
    "nat_hides_the_reversal": ([100, None, 50, 60], False),
    "nat_beside_a_reversal": ([100, None, 50, 40, 60], True),
    "nat_first_and_last": ([None, 10, 20, None], False),
}


def nat_case(name):
    vals, _ = NAT_CASES[name]
    return np.array([np.iinfo(np.int64).min if v is None else v for v in vals], dtype=np.int64).view("datetime64[ns]")


def _seeded(name):
    """Seeded cases: random intervals and reversals."""
    rng = _rng(name)
    if name == "epoch_ns":  # realistic magnitudes: epoch nanoseconds near 1.7e18, a ping a second
        d = rng.integers(900_000_000, 1_100_000_000, 199, dtype=np.int64)
        d[[57, 140]] = [-2_345_678_901, -999_999_999]
        return dict(t=from_diffs(d, T0_NS), win_len=100)
    if name == "epoch_us":  # the same file kept in microseconds: an odd sum truncates in ITS ticks
        d = 2 * rng.integers(450_000, 550_000, 120, dtype=np.int64)  # all even ...
        d[41 + np.argsort(d[41:61], kind="stable")[9]] += 1  # ... but the lower middle of the window of reversal 61
        d[61] = -1_234_567
        return dict(t=from_diffs(d, T0_NS // 1000, "us"), win_len=20)
    if name == "every_third_w7":  # a third of the differences are reversals: every window holds several
        d = rng.integers(20, 90, 100, dtype=np.int64)
        d[2::3] = -rng.integers(1, 15, len(d[2::3]), dtype=np.int64)
        return dict(t=from_diffs(d), win_len=7)
    assert name.startswith("random"), name
    n = int(rng.integers(8, 160))
    d = rng.integers(1, 2000, n, dtype=np.int64)
    k = int(rng.integers(1, 6))
    at = rng.choice(np.arange(1, n), min(k, n - 1), replace=False)
    d[at] = -rng.integers(1, 3000, len(at), dtype=np.int64)
    return dict(t=from_diffs(d, int(rng.integers(-10**6, 10**6))), win_len=int(rng.integers(1, 40)))


SEEDED = ("epoch_ns", "epoch_us", "every_third_w7") + tuple(f"random{i}" for i in range(12))
FIXTURE_CASES = tuple(LITERAL) + tuple(CLIP) + SEEDED


def case(name):
    if name in LITERAL:
        d, w, t0 = LITERAL[name]
        return dict(t=from_diffs(d, t0), win_len=w)
    if name in ERRORS:
        d, w = ERRORS[name]
        return dict(t=from_diffs(d), win_len=w)
    if name in CLIP or name in CLIP_CAP:
        ni, w = (CLIP.get(name) or CLIP_CAP[name])
        return one_reversal(name, ni, w)
    return _seeded(name)


def load_fixture():
    """(records, the npz) of the reference-executed goldens: ``case/<name>/in``, ``/out``, and the records' ``win_len``,
    ``exists`` and ``raised``."""
    z = np.load(GOLDEN)
    return json.loads(z["cases"].item()), z
