"""mask.label_regions / mask.region_statistics on the host (no GPU): tests/region_ref.py (the scipy / NumPy oracle of the
GPU tests) against a brute-force flood fill and per-pixel loop, the argument errors that come before any device access,
the exports, the C-ABI binding, and the decoding of the downloaded tables."""
import math

import numpy as np
import pytest

import region_ref as R


def _brute_labels(mask, connectivity):
    """Flood fill from every unlabelled pixel in raster order: region k is the k-th first pixel met."""
    P, S = mask.shape
    lab = np.zeros((P, S), dtype=np.int32)
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    n = 0
    for p in range(P):
        for s in range(S):
            if not mask[p, s] or lab[p, s]:
                continue
            n += 1
            lab[p, s] = n
            todo = [(p, s)]
            while todo:
                a, b = todo.pop()
                for da, db in steps:
                    u, v = a + da, b + db
                    if 0 <= u < P and 0 <= v < S and mask[u, v] and not lab[u, v]:
                        lab[u, v] = n
                        todo.append((u, v))
    return lab, n


def _scene(P, S, C, seed):
    rng = np.random.default_rng(seed)
    sv = -70.0 + 8.0 * rng.standard_normal((C, P, S))
    sv[rng.random((C, P, S)) < 0.1] = np.nan
    depth = 5.0 + np.cumsum(rng.uniform(0.1, 0.4, (C, P, S)), axis=2)
    depth[1 % C, :, -2:] = np.nan
    mask = rng.random((P, S)) < 0.45
    return sv, depth, mask


@pytest.mark.parametrize("P,S,C,connectivity,seed", [(7, 9, 2, 4, 1), (6, 11, 3, 8, 2)])
def test_oracle_against_a_brute_force_loop(P, S, C, connectivity, seed):
    sv, depth, mask = _scene(P, S, C, seed)
    want_lab, n = _brute_labels(mask, connectivity)
    got = R.statistics(sv, depth, mask, connectivity, ping_time=np.arange(P) * 10)
    assert got["n_regions"] == n and n > 3
    np.testing.assert_array_equal(got["region_label"], want_lab)
    for k in range(n):
        px = [(p, s) for p in range(P) for s in range(S) if want_lab[p, s] == k + 1]
        p0, p1 = min(p for p, _ in px), max(p for p, _ in px)
        assert got["n_samples"][k] == len(px)
        assert (got["ping_first"][k], got["ping_last"][k]) == (p0, p1)
        assert (got["sample_first"][k], got["sample_last"][k]) == (min(s for _, s in px), max(s for _, s in px))
        assert got["n_pings"][k] == p1 - p0 + 1
        assert (got["ping_time_start"][k], got["ping_time_end"][k]) == (10 * p0, 10 * p1)
        for c in range(C):
            lin, r, dz, x = [], [], [], []
            for p, s in px:
                rr = depth[c, p]
                d = (rr[s] - rr[s - 1]) if s > 0 else (rr[1] - rr[0])
                x.append(sv[c, p, s])
                lin.append(10.0 ** (sv[c, p, s] / 10.0))
                r.append(rr[s])
                dz.append(d)
            ok = [not math.isnan(v) for v in x]
            nv = sum(ok)
            assert got["n_valid"][c, k] == nv

            def close(name, want):
                g = got[name][c, k]
                assert (math.isnan(g) and math.isnan(want)) or g == pytest.approx(want, rel=1e-13, abs=0), (name, c, k)

            ssv = math.fsum(v for v, o in zip(lin, ok) if o)
            close("Sv_mean", 10 * math.log10(ssv / nv) if nv else math.nan)
            close("Sv_max", max((v for v, o in zip(x, ok) if o), default=math.nan))
            rv = [v for v in r if not math.isnan(v)]
            close("range_min", min(rv, default=math.nan))
            close("range_max", max(rv, default=math.nan))
            close("range_mean", math.fsum(rv) / len(rv) if rv else math.nan)
            both = [(a, b) for a, b in zip(lin, r) if not math.isnan(a) and not math.isnan(b)]
            den = math.fsum(a for a, _ in both)
            close("center_of_mass", math.fsum(a * b for a, b in both) / den if den else math.nan)
            close("height_mean", math.fsum(v for v in dz if not math.isnan(v)) / (p1 - p0 + 1))
            close("NASC", R.NASC_FACTOR * math.fsum(a * b for a, b in zip(lin, dz)
                                                    if not math.isnan(a) and not math.isnan(b)) / (p1 - p0 + 1))
            val, absum, cnt = (got["sums"]["sum_sv_dz"][j][c, k] for j in range(3))
            assert cnt == sum(1 for a, b in zip(lin, dz) if not math.isnan(a) and not math.isnan(b))
            assert absum >= abs(val)


def test_checkerboard_counts():
    """The checkerboard of the GPU tests: as many regions as the labelling's table holds at connectivity 4, one at 8."""
    from echopype_amd import ops

    pp, ss = np.meshgrid(np.arange(3), np.arange(65), indexing="ij")
    board = (pp + ss) % 2 == 0
    assert R.label(board, 4)[1] == 98 == ops.shoal_table_capacity(3, 65, 4)
    assert R.label(board, 8)[1] == 1
    assert R.label(np.zeros((0, 5), dtype=bool), 8)[1] == 0


def _ds(P=4, S=6, C=2):
    from echopype_amd.xr_lite import Dataset

    ds = Dataset(coords={"channel": np.array([f"c{i}" for i in range(C)]), "ping_time": np.arange(P),
                         "range_sample": np.arange(S)})
    ds["Sv"] = (("channel", "ping_time", "range_sample"), np.zeros((C, P, S)))
    ds["depth"] = (("channel", "range_sample"), np.ones((C, S)))
    return ds


def test_argument_errors_come_before_any_device_access(monkeypatch):
    import torch

    import echopype_amd as ep
    from echopype_amd.xr_lite import DataArray

    for name in ("current_device", "current_stream", "synchronize"):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: pytest.fail("device access"))
    m = np.ones((4, 6), dtype=bool)
    for bad in (6, 0, "8", True, None):
        with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
            ep.mask.label_regions(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
            ep.mask.region_statistics(_ds(), m, connectivity=bad)
    with pytest.raises(ValueError, match="select one"):
        ep.mask.label_regions(DataArray(np.ones((2, 4, 6), dtype=bool), ("channel", "ping_time", "range_sample")))
    with pytest.raises(ValueError, match="plane expected"):
        ep.mask.label_regions(np.ones((1, 4, 6), dtype=bool))
    with pytest.raises(ValueError, match="must have the dimensions"):
        ep.mask.label_regions(DataArray(m, ("ping_time", "depth")))
    with pytest.raises(ValueError, match="does not contain the variable var_name='TS'"):
        ep.mask.region_statistics(_ds(), m, var_name="TS")
    with pytest.raises(ValueError, match="does not contain the variable range_var='echo_range'"):
        ep.mask.region_statistics(_ds(), m, range_var="echo_range")
    with pytest.raises(ValueError, match="'ping_time' has length 5"):
        ep.mask.region_statistics(_ds(), np.ones((5, 6), dtype=bool))
    with pytest.raises(ValueError, match="'range_sample' has length 4"):
        ep.mask.region_statistics(_ds(), DataArray(np.ones((4, 4), dtype=bool), ("range_sample", "ping_time")))
    with pytest.raises(ValueError, match="select one"):
        ep.mask.region_statistics(_ds(), DataArray(np.ones((2, 4, 6), dtype=bool), ("channel", "ping_time", "range_sample")))


def test_exports_and_binding():
    import echopype_amd as ep
    from echopype_amd import _lib, ops
    from echopype_amd.build import SOURCES

    assert ep.mask.__all__[-2:] == ["label_regions", "region_statistics"]
    assert callable(ep.mask.label_regions) and callable(ep.mask.region_statistics)
    assert callable(ops.region_stats) and callable(ops.region_labels) and callable(ops.region_tables)
    assert "epa_region_stats" in _lib.SIGNATURES and "epa_region_labels" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["epa_region_stats"]) == 14 and len(_lib.SIGNATURES["epa_region_labels"]) == 7
    assert "region_stats.hip" in SOURCES
    assert len(_lib.REGION_FIELDS) == _lib.REGION_WORDS == 11 and _lib.REGION_ID_WORDS == 2
    assert (_lib.SHOAL_STATE_ERROR, _lib.SHOAL_STATE_COUNT) == (0, 1)


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    """The argument checks of the two entries run before anything is launched."""
    import ctypes

    from echopype_amd import _lib

    one = ctypes.c_void_p(8)  # (never dereferenced: the calls are refused)
    for args in ((None, 4, 4, None, None, 1, 0, 0, 0, 1, None, one, one, None),      # no code plane
                 (one, 0, 4, None, None, 1, 0, 0, 0, 1, None, one, one, None),       # P == 0
                 (one, 4, 4, None, None, 1, 0, 0, 0, 0, None, one, one, None),       # n == 0
                 (one, 4, 4, None, None, 1, 0, 0, 0, 17, None, one, one, None),      # more regions than pixels
                 (one, 4, 4, one, one, 7, 2, 0, 0, 1, one, one, one, None),          # dtype
                 (one, 4, 4, one, one, 1, 2, -1, 0, 1, one, one, one, None),         # a negative stride
                 (one, 4, 4, one, one, 1, 2, 0, 0, 1, None, one, one, None)):        # C > 0 without a table
        assert _lib.lib.epa_region_stats(*args) == _lib.EPA_EINVAL, args
        assert "epa_region_stats" in _lib.last_error()
    assert _lib.lib.epa_region_labels(one, 4, 4, None, 1, one, None) == _lib.EPA_EINVAL
    assert _lib.lib.epa_region_labels(one, 4, 4, one, 0, one, None) == _lib.EPA_EINVAL


def test_table_decoding():
    """ops.region_tables: counts as they are, sums from their float64 bits, extrema from their order-preserving keys
    (key 0: nothing seen -> NaN), the first pixel from its P*S - index form, the minimum from its negated maximum."""
    from echopype_amd import _lib, ops

    def key(v):
        b = np.array([v], dtype=np.float64).view(np.uint64)[0]
        return (~b if b >> np.uint64(63) else b | (np.uint64(1) << np.uint64(63))).astype(np.uint64)

    vals = [-85.5, -1e-300, -0.0, 0.0, 3.25, 1e300]
    keys = [int(key(v)) for v in vals]
    assert keys == sorted(keys) and all(k != 0 for k in keys)
    np.testing.assert_array_equal(ops._unkey(np.array(keys, dtype=np.uint64).view(np.int64)), np.array(vals))
    assert np.isnan(ops._unkey(np.zeros(1, dtype=np.int64))[0])

    W = {n: j for j, n in enumerate(_lib.REGION_FIELDS)}
    stats = np.zeros((1, 2, 11), dtype=np.uint64)
    stats[0, 0, W["n_valid"]] = 5
    stats[0, 0, W["sv_max"]] = key(-61.5)
    stats[0, 0, W["range_min"]] = key(-12.5)  # the key of max(-r)
    stats[0, 0, W["range_max"]] = key(40.0)
    stats[0, 0, W["sum_sv"]] = np.array([1.5e-6]).view(np.uint64)[0]
    ids = np.array([[5, 100 - 17], [2, 100 - 3]], dtype=np.int64)
    t = ops.region_tables(stats.view(np.int64), ids, 100)
    assert t["n_samples"].tolist() == [5, 2] and t["first"].tolist() == [17, 3]
    assert t["n_valid"].tolist() == [[5, 0]] and t["sum_sv"][0, 0] == 1.5e-6 and t["sum_sv"][0, 1] == 0.0
    assert (t["sv_max"][0, 0], t["range_min"][0, 0], t["range_max"][0, 0]) == (-61.5, 12.5, 40.0)
    assert np.isnan(t["sv_max"][0, 1]) and np.isnan(t["range_min"][0, 1]) and np.isnan(t["range_max"][0, 1])
