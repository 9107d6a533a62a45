"""Every float32 instance of every route of csrc/noise_masks.hip against the float64 oracle, on exactly the float32
values the kernel read, judged by the derived bounds of tests/f32_bounds.py (``pooled_mean_bound``,
``pooled_median_bound`` and the three decision bounds) -- not by a flat 1e-3.

The oracle's windows are the kernel's windows: ``oracle.masks.pool_Sv`` / ``downsample_upsample`` /
``echopy_attenuated_signal_mask`` are called with the range array in float32 and with the bin, ``exclude_above`` and the
layer limits as ``np.float32`` (explicitly, not through NumPy's scalar promotion), and with the float32 Sv upcast to
float64.  That is the reference's own arithmetic on float32 arrays (clean/utils.py:77-92) and what the kernels' header
promises: edges and feasibility in the storage type, sums in double.

Each case asserts, through ``_judge_pooled`` / ``_judge_attenuated`` of test_gpu_masks.py:
  * the pooled / smoothed value within its bound, with the oracle's NaN and inf pattern (and the old 1e-3 bar),
  * at most 0.1 % of the decisions within the bound of the threshold (a condition on the input), and every decision
    outside it equal to the oracle's,
  * a case that is not degenerate (both mask values; finite and NaN pooled elements),
and pins its route with ``launch_trace``.  Routes that are otherwise compared with each other (running sums / window
sums, carried / from memory) are EACH compared with the oracle here: two routes sharing one wrong window do not pass.
"""
import numpy as np
import pytest

import f32_bounds as fb
from oracle import masks as omask
from mask_judges import assert_edges_decide, judge_attenuated as _judge_attenuated, judge_pooled as _judge_pooled, \
    same_bins as _same_bins, value_mean_bound as _value_mean_bound
from test_gpu_masks import _box_mean_db, _dev, _median_filter_db, _scene

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import _lib, ops

    return torch, ops, _lib


def _traced(_lib, fn, *need):
    """Run ``fn`` under launch_trace and require every kernel of ``need`` among the launches."""
    with _lib.launch_trace() as tr:
        out = fn()
    for k in need:
        assert k in tr.kernels, (k, tr.kernels)
    return out


# ------------------------------------------------------------------------------------------ smoothing + impulse mask
def _judge_impulse(torch, ops, _lib, what, up_t, up_exp, b_up, n, thr):
    """impulse_compare_kernel on the kernel's own float32 smoothed Sv against the oracle's comparison of ITS smoothed Sv."""
    got = _traced(_lib, lambda: ops.impulse_mask(up_t, n, thr), "impulse_compare_kernel").cpu().numpy().astype(bool)
    exp = np.stack([omask.echopy_impulse_noise_mask(u.T, n, thr).T for u in up_exp])
    margin, bound = fb.impulse_decision_bound(up_exp, b_up, n, thr)
    fb.assert_few_near(margin, bound, what)
    fb.check_decisions(got, exp, margin, bound, what)
    assert exp.any() and not exp.all(), what


def test_range_bin_smooth_index_mode_and_impulse_mask(env):
    torch, ops, _lib = env
    sv, depth = _scene(3, 17, 203, 1, ragged=True)
    sv, depth = sv.astype(f32), depth.astype(f32)
    # (index binning reads the range only for ceil(bin / mean step), which the API takes from the DOUBLE mean of the steps)
    exp = omask.index_binning_downsample_upsample(sv.astype(np.float64), depth.astype(np.float64), 2.0)
    n = omask.nsamples_per_bin(depth.astype(np.float64), 2.0)
    assert len(set(n.tolist())) == 3
    svt = _dev(torch, sv)
    up = torch.empty_like(svt)
    for c in range(3):
        _traced(_lib, lambda: ops.range_bin_smooth(svt[c:c + 1].contiguous(), nper=int(n[c]), out=up[c:c + 1]),
                "range_bin_smooth_kernel")
    b = fb.pooled_mean_bound(sv, exp)
    fb.assert_f32_close(up.cpu().numpy(), exp, b, "mask: range_bin_smooth, index mode")
    assert np.isnan(exp).any() and np.isfinite(exp).any()
    _judge_impulse(torch, ops, _lib, "impulse mask, index mode", up, exp, b, 2, 10.0)


def test_range_bin_smooth_value_mode_and_impulse_mask(env):
    torch, ops, _lib = env
    sv, depth = _scene(2, 13, 150, 2)
    sv[0, 3, :] = np.nan
    sv, depth = sv.astype(f32), depth.astype(f32)
    down, exp = omask.downsample_upsample(sv.astype(np.float64), depth, f32(5.0))
    r0, hi = float(np.nanmin(depth)), float(np.nanmax(depth))
    nb = len(np.arange(r0, hi + 5.0, 5.0)) - 1
    assert down.shape[-1] == nb and _same_bins(depth, f32(5.0), r0, (r0 + 5.0) - r0, nb)
    up = _traced(_lib, lambda: ops.range_bin_smooth(_dev(torch, sv), range=_dev(torch, depth), r0=r0, bin=5.0, nbins=nb),
                 "range_bin_smooth_kernel")
    b = fb.pooled_mean_bound(sv, exp)
    fb.assert_f32_close(up.cpu().numpy(), exp, b, "mask: range_bin_smooth, value mode")
    assert np.isnan(exp).any() and np.isfinite(exp).any()
    _judge_impulse(torch, ops, _lib, "impulse mask, value mode", up, exp, b, 2, 10.0)


@pytest.mark.parametrize("mode", ["value", "index"])
def test_range_bin_smooth_more_bins_than_the_lds_holds(env, mode):
    """More than 13 500 bins in a ping: the bins are taken in segments.  Value mode on a grid float32 holds exactly
    (samples every 2^-4 m, bins of 2^-6 m from 4 m on: every fourth edge lies ON a sample, which opens its bin)."""
    torch, ops, _lib = env
    rng = np.random.default_rng(3)
    if mode == "value":
        S = 3700
        depth = np.tile(4.0 + 0.0625 * np.arange(S), (1, 3, 1)).astype(f32)
        sv = (-60 + 5 * rng.standard_normal((1, 3, S))).astype(f32)
        sv[0, 1, 100:140] = np.nan
        dbin = 2.0 ** -6
        down, exp = omask.downsample_upsample(sv.astype(np.float64), depth, f32(dbin))
        r0, hi = float(depth.min()), float(depth.max())
        nb = len(np.arange(r0, hi + dbin, dbin)) - 1
        assert nb > 13500 and down.shape[-1] == nb and _same_bins(depth, f32(dbin), r0, dbin, nb)
        got = _traced(_lib, lambda: ops.range_bin_smooth(_dev(torch, sv), range=_dev(torch, depth), r0=r0, bin=dbin,
                                                         nbins=nb), "range_bin_smooth_kernel")
    else:
        S = 30_001
        sv = (-60 + 5 * rng.standard_normal((1, 2, S))).astype(f32)
        sv[0, 0, 7::11] = np.nan
        sv[0, 1, 1000:1002] = np.nan                      # a bin without a value
        depth = np.tile(np.arange(S, dtype=f32), (1, 2, 1))
        exp = omask.index_binning_downsample_upsample(sv.astype(np.float64), depth.astype(np.float64), 2.0)  # 15 001 bins
        got = _traced(_lib, lambda: ops.range_bin_smooth(_dev(torch, sv), nper=2), "range_bin_smooth_kernel")
    fb.assert_f32_close(got.cpu().numpy(), exp, fb.pooled_mean_bound(sv, exp), f"mask: segmented bins, {mode} mode")
    assert np.isnan(exp).any() and np.isfinite(exp).any()


# ------------------------------------------------------------------------------------------ index windows, nanmean
@pytest.mark.parametrize("P,S,n,m,s0,kernel", [
    (700, 1100, 25, 53, 100, "box_range_scan_kernel"),   # two ping segments, two range tiles
    (513, 2300, 1, 4, 3, "box_range_scan_kernel"),       # w = 9 >= kScanMinW: the smallest scanned window; a segment join
    (33, 64, 1, 3, 40, "box_range_kernel"),              # w = 7 < kScanMinW: the grouped kernel
    (40, 1500, 600, 255, 7, "box_range_scan_kernel"),    # w = 511 <= kScanMaxW: the largest scanned window
    (90, 1300, 3, 256, 2, "box_range_kernel"),           # w = 513 > kScanMaxW: grouped again
    (1030, 35, 2, 20, 3, "box_range_scan_kernel"),       # window wider than the row, three ping segments
])
def test_pool_sv_index_windows(env, P, S, n, m, s0, kernel):
    torch, ops, _lib = env
    rng = np.random.default_rng(P + S + n + m)
    sv = -80 + 8 * rng.standard_normal((1, P, S))
    sv[0, rng.random((P, S)) < 0.03] += 50
    sv[0, rng.random((P, S)) < 0.05] = np.nan
    sv[0, P // 2, :] = np.nan
    sv = sv.astype(f32)
    exp = _box_mean_db(sv[0].astype(np.float64), n, m, s0)
    pooled, mask = _traced(_lib, lambda: ops.pool_sv(_dev(torch, sv), s0, n, m, threshold=9.0), kernel,
                           "box_ping_slide_kernel")
    b = fb.pooled_mean_bound(sv, exp, carried_terms=(2 * n + 1) * (2 * m + 1), carried_ops=P)
    _judge_pooled("float32", f"index window {2 * n + 1}x{2 * m + 1} on {P}x{S}", sv[0], pooled.cpu().numpy()[0],
                  mask.cpu().numpy()[0], exp, 9.0, b)


# ------------------------------------------------------------------------------------------ index windows, nanmedian
def test_pool_sv_median_carried_window(env):
    """pool_median_slide_kernel across two 512-ping joins (the scene of test_gpu_masks' carried-median test)."""
    torch, ops, _lib = env
    rng = np.random.default_rng(21)
    P, S, n, m = 1100, 24, 6, 4
    sv = -80 + 3 * rng.standard_normal((1, P, S))
    sv[0, rng.random((P, S)) < 0.04] = -300 - 20 * rng.random()
    sv[0, rng.random((P, S)) < 0.04] = 5 + 20 * rng.random()
    sv[0, 200:260, 3:9] = -330 + 30 * rng.random((60, 6))
    sv[0, 600:650, 12:20] = 10 + 30 * rng.random((50, 8))
    sv[0, 505:520, 5] = np.inf
    sv[0, 900, 10:14] = -np.inf
    sv[0, rng.random((P, S)) < 0.08] = np.nan
    sv[0, 300:320, :] = np.nan
    sv = sv.astype(f32)
    pooled, mask = _traced(_lib, lambda: ops.pool_sv(_dev(torch, sv), 2, n, m, func="nanmedian", threshold=6.0),
                           "pool_median_slide_kernel")
    got = pooled.cpu().numpy()[0]
    assert np.isnan(got[:, :2]).all() and not mask.cpu().numpy()[0, :, :2].any()
    exp = _median_filter_db(sv[0, :, 2:], n, m)
    _judge_pooled("float32", "carried median", sv[0, :, 2:], got[:, 2:], mask.cpu().numpy()[0, :, 2:], exp, 6.0,
                  fb.pooled_median_bound(exp))


def test_pool_sv_median_every_window_from_memory(env):
    """2m + 1 > 256 columns: pool_median_kernel sweeps every window."""
    torch, ops, _lib = env
    sv, _ = _scene(1, 12, 40, 12, nan_frac=0.1)
    sv[0, 4:7, :] = np.nan                              # n = 1: ping 5 has no valid value in its window
    sv = sv.astype(f32)
    pooled, mask = _traced(_lib, lambda: ops.pool_sv(_dev(torch, sv), 0, 1, 130, func="nanmedian", threshold=3.0),
                           "pool_median_kernel")
    exp = _median_filter_db(sv[0], 1, 130)
    _judge_pooled("float32", "median, wide window", sv[0], pooled.cpu().numpy()[0], mask.cpu().numpy()[0], exp, 3.0,
                  fb.pooled_median_bound(exp))


# ------------------------------------------------------------------------------------------ value windows
def _finish(sv, depth, rng, C, P, S):
    """The additions every value-window scene of test_gpu_masks carries: NaN tails, a +60 dB spike, a +inf sample."""
    depth[:, 7 % P, S - 20:] = np.nan
    sv[np.isnan(depth)] = np.nan
    sv[0, 10 % P, 100 % S] = 60.0
    sv[C - 1, (P // 2) % P, 50 % S] = np.inf
    return sv.astype(f32), depth.astype(f32)


def _rows_scene(same_rows, seed=12):
    """test_pool_sv_value_running_sums_equal_window_sums: 0.3 m steps, a 1.45 m bin (no window edge on a sample)."""
    rng = np.random.default_rng(8)
    C, P, S = 2, 40, 300
    sv, depth = _scene(C, P, S, seed, step=0.3)
    if same_rows is False:
        depth = depth * (1 + 0.01 * rng.random((C, P, 1)))
    elif same_rows == "mixed":
        depth[1] = depth[1] * (1 + 0.01 * rng.random((P, 1)))
    depth[0, 30, S - 55:] = np.nan
    sv, depth = _finish(sv, depth, rng, C, P, S)
    return sv, depth, 4, 1.45, 2.0


def _staged_scene(case):
    """test_pool_sv_value_staged_neighbour_rows."""
    rng = np.random.default_rng(23)
    if case in ("blocks_of_pings", "rows_not_affine", "a_shallow_neighbour_row"):
        C, P, S, n, dbin, step = 2, 43, 700, 6, 3.1, 0.3
    elif case == "span_beyond_the_lds_copy":
        C, P, S, n, dbin, step = 1, 21, 1500, 3, 85.0, 0.3
    elif case == "span_in_the_third_slot":
        C, P, S, n, dbin, step = 1, 21, 1500, 3, 50.0, 0.3
    else:  # more_neighbours_than_span_slots: 41 feasible pings, each with 1061 neighbours
        C, P, S, n, dbin, step = 1, 1100, 70, 530, 1.3, 0.3
    sv, _ = _scene(C, P, S, 12, step=step)
    block = 5 if case == "blocks_of_pings" else 1
    scale = 1 + 0.01 * rng.random((C, (P + block - 1) // block, 1))
    depth = (1.5 + step * np.arange(S))[None, None, :] * np.repeat(scale, block, axis=1)[:, :P]
    if case == "rows_not_affine":
        k = np.arange(S)
        uneven = np.cumsum(step * (0.2 + 1.6 * rng.random(S)))
        depth = (1.5 + uneven + 2e-4 * k * k + 3.0 * (k > 300))[None, None, :] * np.repeat(scale, block, axis=1)[:, :P] \
            + 0.7 * rng.random((C, P, 1))
    if case == "a_shallow_neighbour_row":
        depth[:, 20] *= 0.3
        depth[0, 31] *= 0.05
    sv[rng.random((C, P, S)) < 0.03] = np.nan
    sv, depth = _finish(sv, depth, rng, C, P, S)
    assert (np.diff(depth, axis=-1)[np.isfinite(np.diff(depth, axis=-1))] >= 0).all()
    return sv, depth, n, dbin, 2.0


def _runs_scene(case):
    """test_pool_sv_value_runs_of_one_range_vector (260 samples per ping: half the oracle's triple loop)."""
    rng = np.random.default_rng(41)
    C, S, dbin, step, n = 2, 260, 2.3, 0.3, 9
    lens = [60, 23, 90, 40]
    P = sum(lens)
    sv, _ = _scene(C, P, S, 12, step=step)
    scale = np.repeat(1 + 0.004 * np.arange(len(lens)), lens)
    depth = (1.5 + step * np.arange(S))[None, None, :] * scale[None, :, None] * np.ones((C, 1, 1))
    depth[1] *= 1.0 + 0.0007 * rng.random((P, 1))
    depth[0, 30, S - 55:] = np.nan
    depth[0, 100, :] = np.nan
    if case == "bridged":
        depth[0, 60:83] = depth[0, 0] + 0.0
        depth[0, 61:83, 10:] += 0.004 * (np.arange(S - 10) + 1)
        depth[0, 60, 3:] = np.nan
    sv[rng.random((C, P, S)) < 0.03] = np.nan
    sv, depth = _finish(sv, depth, rng, C, P, S)
    sv[0, 75, 50] = np.inf
    return sv, depth, n, dbin, 2.0


def _grid_scene(kind, seed=13):
    """Window edges ON samples: every range value is np.float32(k * 0.3) for an integer k and the bin is 1.5 m = 5 steps,
    so d - bin and d + bin are (up to their float32 rounding) samples of the rows -- whether such a sample is in the
    window is decided by the last bit of a float32 addition.  ``one_vector``: one row per channel; ``shifted``: the grid
    moves by one step every 3 pings (no run of 2n+1 = 5: the staged kernels); ``runs``: every 10 pings (the run form)."""
    rng = np.random.default_rng(seed)
    C, P, S, n = 2, 30, 300, 2
    sv = -70 + 4 * rng.standard_normal((C, P, S)) - 10 * np.linspace(0, 1, S)
    sv[rng.random((C, P, S)) < 0.02] += 30
    sv[rng.random((C, P, S)) < 0.03] = np.nan
    sv[1, 12, 200:260] = -71.25                         # a flat stretch (its own value is 6 dB from no threshold)
    every = {"one_vector": 10**9, "shifted": 3, "runs": 10}[kind]
    k = np.arange(S)[None, None, :] + (np.arange(P) // every)[None, :, None] + np.array([5, 11])[:, None, None]
    depth = (k * 0.3).astype(f32)
    depth[0, 20, S - 30:] = np.nan
    sv[np.isnan(depth)] = np.nan
    sv[0, 10, 100] = 60.0
    sv[1, 15, 50] = np.inf
    return sv.astype(f32), depth, n, 1.5, 2.0


def _oracle_value(sv, depth, func, dbin, n, excl):
    return omask.pool_Sv(sv.astype(np.float64), depth, np.nanmean if func == "nanmean" else np.nanmedian, f32(dbin), n,
                         f32(excl))


def _assert_edges_decide(sv, depth, func, dbin, n, excl, exp, bound):
    return assert_edges_decide(sv, depth, np.nanmean if func == "nanmean" else np.nanmedian, dbin, n, excl, exp, bound)


def _run_value(env, sv, depth, n, dbin, excl, func, running_sums, thr=6.0):
    torch, ops, _lib = env
    svt, rgt = _dev(torch, sv), _dev(torch, depth)
    nvalid, bad = ops.range_rows_check(rgt)
    assert bad == 0
    lo, hi = ops.nanminmax(rgt)
    with _lib.launch_trace() as tr:
        pooled, mask = ops.pool_sv_value(svt, rgt, nvalid, dbin, n, excl, lo, hi, func=func, threshold=thr,
                                         running_sums=running_sums)
    return pooled.cpu().numpy(), mask.cpu().numpy(), tr.kernels


MEAN_ROUTES = {
    "one_vector": ("row_interval_blocks_kernel", "value_slide_kernel"),
    "rows_differ": ("row_running_sum_kernel", "pool_value_mean_lean_kernel", "pool_value_mean_staged_kernel"),
    "mixed": ("row_interval_blocks_kernel", "value_slide_kernel", "pool_value_mean_lean_kernel"),
}


def _check_mean(env, what, scene, routes, edges=False, need_inf=True):
    sv, depth, n, dbin, excl = scene
    exp = _oracle_value(sv, depth, "nanmean", dbin, n, excl)
    bound = _value_mean_bound(sv, exp, n)
    if edges:
        _assert_edges_decide(sv, depth, "nanmean", dbin, n, excl, exp, bound)
    a, ma, ka = _run_value(env, sv, depth, n, dbin, excl, "nanmean", True)
    for k in routes:
        assert k in ka, (k, ka)
    _judge_pooled("float32", f"{what}: running sums", sv, a, ma, exp, 6.0, bound)
    b, mb, kb = _run_value(env, sv, depth, n, dbin, excl, "nanmean", False)
    assert kb == ["pool_value_mean_kernel"], kb
    _judge_pooled("float32", f"{what}: every window summed", sv, b, mb, exp, 6.0, bound)
    assert np.isposinf(exp).any() or not need_inf


@pytest.mark.parametrize("same_rows", ["one_vector", "rows_differ", "mixed"])
def test_pool_sv_value_mean_routes(env, same_rows):
    scene = _rows_scene({"one_vector": True, "rows_differ": False, "mixed": "mixed"}[same_rows])
    _check_mean(env, same_rows, scene, MEAN_ROUTES[same_rows])


def test_pool_sv_value_mean_rows_longer_than_the_lds_copy(env):
    """8200 samples per ping: the unfused running sums and interval sums through the workspace
    (row_running_sum_kernel + row_interval_sum_kernel), with the +60 dB spike in a row whose later windows are 10^15
    times weaker than the running sums they are differences of."""
    rng = np.random.default_rng(17)
    C, P, S, n, dbin = 1, 6, 8200, 2, 2.2
    depth = ((1.0 + 0.05 * np.arange(S))[None, None, :] + np.zeros((C, P, 1))).astype(f32)
    sv = -75 + 5 * rng.standard_normal((C, P, S))
    sv[rng.random((C, P, S)) < 0.05] = np.nan
    sv[0, 2, 300] = 60.0
    sv[0, 3, 4000] = np.inf
    # 0.05 m steps, a 2.2 m bin = 44 steps: window edges on samples (float32 and float64 membership differ at half the
    # outputs, asserted)
    _check_mean(env, "long rows", (sv.astype(f32), depth, n, dbin, 5.0),
                ("row_running_sum_kernel", "row_interval_sum_kernel", "value_slide_kernel"), edges=True)


@pytest.mark.parametrize("case", ["blocks_of_pings", "span_beyond_the_lds_copy", "span_in_the_third_slot",
                                  "more_neighbours_than_span_slots", "rows_not_affine", "a_shallow_neighbour_row"])
def test_pool_sv_value_mean_staged_and_lean(env, case):
    """The lean kernel and the staged one.  Both are launched whatever the input, so the trace does not show WHICH groups
    the lean kernel handed back through ``todo``; that rests on the source (a row with a +inf Sv -- every scene has one --,
    a span beyond the LDS copy, a ping window beyond the span slots make it flag the group) and on those groups' outputs,
    +inf windows among them, matching the oracle like all the others."""
    _check_mean(env, case, _staged_scene(case), ("row_running_sum_kernel", "pool_value_mean_lean_kernel",
                                                 "pool_value_mean_staged_kernel"))


@pytest.mark.parametrize("case", ["runs", "bridged"])
def test_pool_sv_value_mean_run_form(env, case):
    _check_mean(env, case, _runs_scene(case), ("run_verify_kernel", "value_slide_runs_kernel", "row_interval_blocks_kernel",
                                               "pool_value_mean_staged_kernel"))


@pytest.mark.parametrize("kind,routes", [
    ("one_vector", ("row_interval_blocks_kernel", "value_slide_kernel")),
    ("shifted", ("row_running_sum_kernel", "pool_value_mean_lean_kernel", "pool_value_mean_staged_kernel")),
    ("runs", ("run_verify_kernel", "value_slide_runs_kernel", "pool_value_mean_staged_kernel")),
])
def test_pool_sv_value_mean_window_edges_on_samples(env, kind, routes):
    _check_mean(env, f"edges on samples, {kind}", _grid_scene(kind), routes, edges=True)


def _check_median(env, what, scene, edges=False, carried=True):
    sv, depth, n, dbin, excl = scene
    exp = _oracle_value(sv, depth, "nanmedian", dbin, n, excl)
    bound = fb.pooled_median_bound(exp)
    if edges:
        _assert_edges_decide(sv, depth, "nanmedian", dbin, n, excl, exp, bound)
    a, ma, ka = _run_value(env, sv, depth, n, dbin, excl, "nanmedian", True)
    assert ka[-1] == "pool_value_median_slide_kernel", ka
    _judge_pooled("float32", f"{what}: carried window", sv, a, ma, exp, 6.0, bound)
    b, mb, kb = _run_value(env, sv, depth, n, dbin, excl, "nanmedian", False)
    assert kb == ["pool_value_median_kernel"], kb
    _judge_pooled("float32", f"{what}: windows from memory", sv, b, mb, exp, 6.0, bound)


@pytest.mark.parametrize("same_rows", ["one_vector", "rows_differ", "mixed"])
def test_pool_sv_value_median_routes(env, same_rows):
    _check_median(env, same_rows, _rows_scene({"one_vector": True, "rows_differ": False, "mixed": "mixed"}[same_rows], 13))


@pytest.mark.parametrize("kind", ["one_vector", "shifted"])
def test_pool_sv_value_median_window_edges_on_samples(env, kind):
    _check_median(env, f"edges on samples, {kind}", _grid_scene(kind), edges=True)


def test_pool_sv_value_median_segments_and_flat_field(env):
    """600 pings (two 512-ping segments) of one range vector on a grid float32 holds exactly (0.25 m steps, a 1 m bin:
    every window edge on a sample); a flat stretch of 40 pings (Sv - median = 0 there, 3.5 dB below the threshold),
    and an all-NaN stretch."""
    rng = np.random.default_rng(10)
    C, P, S, n, dbin = 1, 600, 36, 3, 1.0
    sv = -75 + 3 * rng.standard_normal((C, P, S))
    sv[0, 100:140, :] = -70.0
    sv[0, 300:320, :] = np.nan
    sv[0, rng.random((P, S)) < 0.05] = np.nan
    depth = np.broadcast_to(2.0 + 0.25 * np.arange(S), (C, P, S)).astype(f32)
    sv = sv.astype(f32)
    exp = _oracle_value(sv, depth, "nanmedian", dbin, n, 3.0)
    a, ma, ka = _run_value(env, sv, depth, n, dbin, 3.0, "nanmedian", True, thr=3.5)
    assert ka[-1] == "pool_value_median_slide_kernel", ka
    _judge_pooled("float32", "600 pings", sv, a, ma, exp, 3.5, fb.pooled_median_bound(exp))
    assert np.isnan(exp[0, 305:315, 10]).all() and np.isfinite(exp[0, 500:520, 10]).all()


# ------------------------------------------------------------------------------------------ attenuated signal
def _att_scene(depth_kind):
    """test_attenuated_mask_carried_block_equals_medians_from_memory."""
    rng = np.random.default_rng(31)
    C, P, S = 2, 1300, 400
    sv = -70 + 4 * rng.standard_normal((C, P, S)) - 10 * np.linspace(0, 1, S)
    att = rng.random((C, P)) < 0.05
    sv[att] -= rng.uniform(3, 30, size=att.sum())[:, None]
    sv[rng.random((C, P, S)) < 0.03] = np.nan
    sv[0, 500:520] = np.nan
    sv[1, 900:960, 60:300] = -71.25                      # flat: ping median = block median, 6 dB from the threshold
    depth = np.broadcast_to(1.0 + 0.5 * np.arange(S), (C, P, S)).copy()
    if depth_kind == "limits change":
        depth[1, 700:] *= 1.1
        depth[0, 1000:1010] *= 1 + 0.05 * rng.random((10, 1))
    elif depth_kind == "heave":
        depth = depth + 3.0 * np.sin(np.arange(P) / 7.0)[None, :, None]
    return sv.astype(f32), depth.astype(f32)


@pytest.mark.parametrize("depth_kind", ["one vector", "limits change", "heave"])
def test_attenuated_mask_carried_block_and_medians_from_memory(env, depth_kind):
    """attenuated_prepare_kernel + attenuated_walk_kernel, and attenuated_mask_kernel (reached with S % 4 != 0: one
    padding sample far below the layer), each against the oracle on the float32 range and layer limits.  With 0.5 m
    steps the limits 40 m and 140 m lie ON samples of the ``one vector`` rows: np.argmin's first minimum decides."""
    torch, ops, _lib = env
    sv, depth = _att_scene(depth_kind)
    n, thr = 7, -6.0
    svt, rgt = _dev(torch, sv), _dev(torch, depth)
    new = _traced(_lib, lambda: ops.attenuated_mask(svt, rgt, 40.0, 140.0, n, thr), "attenuated_prepare_kernel",
                  "attenuated_walk_kernel")
    _judge_attenuated(f"carried block, {depth_kind}", new.cpu().numpy(), sv, depth, 40.0, 140.0, n, thr)
    pad = torch.nn.functional.pad
    with _lib.launch_trace() as tr:
        ref = ops.attenuated_mask(pad(svt, (0, 1), value=float("nan")).contiguous(),
                                  pad(rgt, (0, 1), value=1.0e6).contiguous(), 40.0, 140.0, n, thr)[:, :, :sv.shape[2]]
    assert tr.kernels == ["attenuated_mask_kernel"]
    _judge_attenuated(f"medians from memory, {depth_kind}", ref.cpu().numpy(), sv, depth, 40.0, 140.0, n, thr)


def test_attenuated_mask_limits_off_the_samples(env):
    """Layer limits no float32 range value equals (30.1 m, 90.3 m in float32), a ragged channel, NaN pings, -inf."""
    torch, ops, _lib = env
    sv, depth = _scene(3, 80, 300, 5, step=0.5, ragged=True)
    sv[1, 40:44, :] = np.nan
    sv[0, 10, 20:60] = -np.inf
    sv, depth = sv.astype(f32), depth.astype(f32)
    got = _traced(_lib, lambda: ops.attenuated_mask(_dev(torch, sv), _dev(torch, depth), 30.1, 90.3, 6, -5.0),
                  "attenuated_walk_kernel")
    _judge_attenuated("attenuated mask", got.cpu().numpy(), sv, depth, 30.1, 90.3, 6, -5.0)
