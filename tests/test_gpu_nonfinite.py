"""+-inf (and overflowing) raw power samples through every Sv -> MVBS route against the oracle (tests/nonfinite_cases.py):
echo_range is NaN where the raw sample is NaN and NOWHERE else (calibrate/range.py:145-147 of the reference), so an
infinite sample keeps its place in the range statistics that size the grid, is no NaN coordinate, and its 10^(Sv/10)
-- +inf or 0 -- is a term of its bin.

float64 outputs: the ``close`` of test_gpu_api.py (NaN pattern, finite values to 1e-9; 1e-7 after the noise removal,
as test_gpu_fuzz.py has it) plus equal +-inf; echo_range and depth bit for bit.  float32 outputs: the class (finite /
+inf / -inf / NaN) of EVERY element is the float64 oracle's and the finite ones lie within the derived bounds of
tests/f32_bounds.py; the ``overflow`` case alone takes its MVBS classes from NumPy's own float32 evaluation
(test_underflow_class_matches_float32_reference's contract, at the other end of the range).
"""
import logging

import numpy as np
import pytest

import f32_bounds as fb
import nonfinite_cases as nc
import oracle_chain as oc
from oracle import calibrate as ocal
from oracle import clean as oclean
from oracle import commongrid as ogrid
from oracle import nasc as onasc
from test_gpu_api import close

pytestmark = pytest.mark.gpu

KEYS = nc.all_cases()
FUSED_KEYS = [k for k in KEYS if k[1] % 4 == 0]     # the specialised kernels need S % 4 == 0
DTYPES = ("float64", "float32")
NAN_WARNING = "coordinate array contain NaNs"


@pytest.fixture(scope="module")
def ep():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU")
    import echopype_amd

    return echopype_amd


# ---- judges -----------------------------------------------------------------------------------------------------------
def same_classes(got, exp, what):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    g, e = nc.classes(got), nc.classes(exp)
    bad = np.argwhere(g != e)
    assert bad.size == 0, (f"{what}: {len(bad)} elements of another class (0 finite, 1 +inf, 2 -inf, 3 NaN); first at "
                           f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, oracle {exp[tuple(bad[0])]!r}")


def judge(got, exp, dtype, what, rtol=1e-9, bound=None, class_ref=None):
    """``got`` against the float64 oracle ``exp``.  ``class_ref``: the array the classes are taken from instead (the
    overflow case in float32); finite values are then compared where both are finite."""
    same_classes(got, exp if class_ref is None else class_ref, what)
    if dtype == "float64":
        close(got, exp, rtol, what)
        return
    if class_ref is not None:
        both = np.isfinite(np.asarray(got, np.float64)) & np.isfinite(exp)
        got, exp = np.where(both, got, np.nan), np.where(both, exp, np.nan)
    fb.assert_f32_close(got, exp, bound, what)


def member_stats(sv, lab, nb, b_sv=0.0):
    """``f32_bounds.bin_stats`` for bins that hold +-inf members: exp10f(-inf) = 0 and exp10f(+inf) = +inf are exact, so
    an infinite member carries no error of its own -- a -inf counts in n (its zero is a term of the mean), a bin with a
    +inf member has no finite mean to bound.  -> (n, exact linear mean, L-weighted relative error of the finite terms)."""
    sv, lab = np.asarray(sv, np.float64), np.asarray(lab)
    fin = np.isfinite(sv)
    b = np.where(fin, np.broadcast_to(np.asarray(b_sv, np.float64), sv.shape), 0.0)
    n_f, mean_f, rho = fb.bin_stats(np.where(fin, lab, -1), nb, np.where(fin, sv, np.nan), b)
    zero = (lab >= 0) & np.isneginf(sv)
    n = n_f + np.bincount(lab[zero].ravel(), minlength=nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n, mean_f * n_f / n, np.where(n_f > 0, rho, 0.0)   # (a bin of zeros only: an exact 0)


def mvbs_bound(sv, lab, nb, exp, b_sv=0.0):
    n, m, r = member_stats(sv, lab, nb, b_sv)
    return fb.mean_db_bound(n, m, r, np.asarray(exp, np.float64).ravel()).reshape(np.shape(exp))


def f32_mvbs_classes(sv32, lab, nb, shape):
    """NumPy's own float32 evaluation of 10 * log10(mean(10 ** (Sv / 10))) per bin (NaN skipped), for its classes."""
    sv32 = np.asarray(sv32, np.float32).ravel()
    lab = np.asarray(lab).ravel()
    use = (lab >= 0) & ~np.isnan(sv32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lin = np.float32(10.0) ** (sv32[use] / np.float32(10.0))
        acc, n = np.zeros(nb, np.float32), np.bincount(lab[use], minlength=nb)
        np.add.at(acc, lab[use], lin)
        mean = np.where(n > 0, acc / np.maximum(n, 1).astype(np.float32), np.float32(np.nan)).astype(np.float32)
        return (np.float32(10.0) * np.log10(mean)).reshape(shape)


def coord_stats(x, dtype):
    """{nanmin, nanmax, NaN count} of the oracle's coordinate as an array of ``dtype`` holds it."""
    x = np.asarray(x).astype(dtype)
    return float(np.nanmin(x)), float(np.nanmax(x)), int(np.isnan(x).sum())


def sv_bound(cs):
    sv, _ = cs.sv_er()
    with np.errstate(invalid="ignore", over="ignore"):
        return fb.sv_power_bound(ocal.cal_power_ek_terms(cs.raw, **oc.ek60_kw(cs.d, "Sv")), sv)


def grid_labels(cs, range_var, range_bin=None):
    """Labels of every sample over the oracle's grid on ``range_var`` -> (labels, number of bins, range edges)."""
    rb = ogrid.parse_range_bin(range_bin or cs.range_bin)
    r_edges = ogrid.range_edges(range_var, rb)
    t_edges = ogrid.ping_edges(cs.d["ping_time"], cs.ping_time_bin)
    lab, nb = fb.labels_range(range_var, cs.d["ping_time"], t_edges, r_edges)
    return lab, nb, r_edges


# ---- inputs -----------------------------------------------------------------------------------------------------------
def echodata(ep, cs):
    return ep.echodata.from_ek60_arrays({**cs.d, "backscatter_r": cs.raw.copy()})


def power_inputs(ep, cs, dtype):
    cal = ep.calibrate.api.CALIBRATOR["EK60"](echodata(ep, cs), None, None, None, dtype=dtype)
    raw, coef, flags, _ = cal._power_inputs("Sv")
    return raw, coef, flags


def time_bins(ep, cs):
    from echopype_amd import ops

    ns = cs.d["ping_time"].astype("datetime64[ns]").astype(np.int64)
    e0, dt = int(ns[0]), 6 * 10**9
    n_t = int((ns[-1] - e0) // dt) + 1
    return ops.time_bin_offsets(ops.to_device(ns), e0, dt, n_t), n_t


def dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(getattr(torch, dtype)) if dtype else t


def warned(caplog):
    return any(NAN_WARNING in r.getMessage() for r in caplog.records)


def check_mvbs_dataset(mv, cs, dtype, what, coord="echo_range", on="Sv", rtol=1e-9, b_sv=None, sv_members=None):
    """An MVBS dataset against the oracle's: shape, both coordinates, values."""
    exp, t_left, r_left = cs.mvbs(on=on)
    got = mv["Sv"].values
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_array_equal(mv[coord].values, r_left, err_msg=f"{what}: range coordinate")
    np.testing.assert_array_equal(mv["ping_time"].values, t_left, err_msg=f"{what}: time coordinate")
    if dtype == "float64":
        judge(got, exp, dtype, what, rtol)
        return
    members = cs.sv_er()[0] if sv_members is None else sv_members
    lab, nb, _ = grid_labels(cs, cs.sv_er()[1])
    ref = f32_mvbs_classes(members, lab, nb, exp.shape) if cs.name == "overflow" else None
    judge(got, exp, dtype, what, bound=mvbs_bound(members, lab, nb, exp, sv_bound(cs) if b_sv is None else b_sv), class_ref=ref)


# ---- compute_Sv: the Sv array, echo_range and its statistics; ops.range_power ------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_compute_sv_and_echo_range(ep, key, dtype, monkeypatch):
    from echopype_amd import _lib, ops

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    # the forms of K1 (sv_power.hip): S not a multiple of 4 -- the scalar kernel, then a sweep of the echo_range array
    # for its statistics; float32 -- one-piece workgroups with the statistics; float64 -- the strided-rows kernel with the
    # statistics, and the pieces with them under EPA_K1_F64_STATS_PIECES=1
    forms = [(None, "sv_power_piece_kernel" if dtype == "float32" and cs.S % 4 == 0 else "sv_power_kernel")]
    if dtype == "float64" and cs.S % 4 == 0:
        forms.append(("1", "sv_power_piece_kernel"))
    for pieces, kernel in forms:
        if pieces:
            monkeypatch.setenv("EPA_K1_F64_STATS_PIECES", pieces)
        with _lib.launch_trace() as tr:
            ds = ep.calibrate.compute_Sv(echodata(ep, cs), dtype=dtype)
            got_sv = ds["Sv"].values
            st = ds["echo_range"].data.cached_stats()
        served = [k for k in tr.kernels if k in ("sv_power_kernel", "sv_power_piece_kernel")]
        assert served == [kernel], tr.kernels
        judge(got_sv, sv, dtype, f"compute_Sv {dtype} ({kernel})", bound=sv_bound(cs))
        assert st == coord_stats(er, dtype), (f"echo_range statistics left by {kernel}", st, coord_stats(er, dtype))
        np.testing.assert_array_equal(ds["echo_range"].values, er.astype(dtype))
    raw, coef, flags = power_inputs(ep, cs, dtype)
    with _lib.launch_trace() as tr:
        rng = ops.range_power(raw, coef, dtype=ops.torch_dtype(dtype))
    assert "range_power_kernel" in tr.kernels or "rows_piece_kernel" in tr.kernels, tr.kernels
    np.testing.assert_array_equal(rng.cpu().numpy(), er.astype(dtype))


# ---- the fused kernel: ops.sv_mvbs_fused (Sv + bins, bins only) with the statistics; compute_Sv_MVBS ------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_fused_sv_mvbs(ep, key, dtype, caplog):
    from echopype_amd import _lib, ops

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    exp, t_left, r_left = cs.mvbs()
    raw, coef, flags = power_inputs(ep, cs, dtype)
    bs, n_t = time_bins(ep, cs)
    rb = ogrid.parse_range_bin(cs.range_bin)
    lab, nb, _ = grid_labels(cs, er)
    b_sv = sv_bound(cs) if dtype == "float32" else None
    b_mv = mvbs_bound(sv, lab, nb, exp, b_sv) if dtype == "float32" else None
    ref = f32_mvbs_classes(sv, lab, nb, exp.shape) if (dtype == "float32" and cs.name == "overflow") else None
    fused = cs.S % 4 == 0
    for want_sv in (True, False):
        with _lib.launch_trace() as tr:
            res = ops.sv_mvbs_fused(raw, coef, bs, n_t, rb, exp.shape[2], cal_flags=flags, dtype=ops.torch_dtype(dtype),
                                    want_sv=want_sv, want_range_stats=True)
        assert ("fused_sv_mvbs_kernel" in tr.kernels) == fused and ("block_reduce_kernel" in tr.kernels) != fused, tr.kernels
        what = f"ops.sv_mvbs_fused {dtype} want_sv={want_sv}"
        judge(res["MVBS"].cpu().numpy(), exp, dtype, what + ": MVBS", bound=b_mv, class_ref=ref)
        if want_sv:
            judge(res["Sv"].cpu().numpy(), sv, dtype, what + ": Sv", bound=b_sv)
        assert res["range_stats_filled"] == fused
        if fused:   # (the statistics of the echo_range array that is not written, as an array of ``dtype`` would hold it)
            got = res["range_stats"].cpu().tolist()
            assert (got[0], got[1], int(got[2])) == coord_stats(er, dtype), (what, got, coord_stats(er, dtype))
    caplog.clear()
    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING):
        ds, mv = ep.compute_Sv_MVBS(echodata(ep, cs), range_bin=cs.range_bin, ping_time_bin=cs.ping_time_bin, dtype=dtype)
        mv["Sv"].values
    assert ("fused_sv_mvbs_kernel" in tr.kernels) == fused, tr.kernels
    check_mvbs_dataset(mv, cs, dtype, f"compute_Sv_MVBS {dtype}")
    judge(ds["Sv"].values, sv, dtype, f"compute_Sv_MVBS {dtype}: Sv", bound=b_sv)
    np.testing.assert_array_equal(ds["echo_range"].values, er.astype(dtype))
    assert warned(caplog) == cs.has_nan, [r.getMessage() for r in caplog.records]


# ---- compute_Sv -> compute_MVBS: Sv deferred, written by the binning pass (the statistics variant) ---------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_two_calls(ep, key, dtype, caplog):
    from echopype_amd import _lib

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING):
        ds = ep.calibrate.compute_Sv(echodata(ep, cs), dtype=dtype)
        mv = ep.commongrid.compute_MVBS(ds, range_bin=cs.range_bin, ping_time_bin=cs.ping_time_bin)
        got_shape = mv["Sv"].shape
    deferred = dtype == "float64" and cs.S % 4 == 0          # (a float32 Sv, an odd S: K1 first, then the binning kernels)
    assert ("fused_sv_mvbs_kernel" in tr.kernels) == deferred, tr.kernels
    assert got_shape == cs.mvbs()[0].shape
    if dtype == "float64":
        check_mvbs_dataset(mv, cs, dtype, "compute_Sv -> compute_MVBS")
    else:  # the bins were decided on the float32 echo_range and summed from the float32 Sv: the oracle on exactly those
        sv32, er32 = ds["Sv"].values.astype(np.float64), ds["echo_range"].values.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            exp32, t_left, r_left = ogrid.compute_MVBS(sv32, er32, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin)
        lab, nb, _ = grid_labels(cs, er32)
        got = mv["Sv"].values
        np.testing.assert_array_equal(mv["echo_range"].values, r_left)
        ref = f32_mvbs_classes(sv32, lab, nb, exp32.shape) if cs.name == "overflow" else None
        judge(got, exp32, dtype, "compute_Sv -> compute_MVBS float32", bound=mvbs_bound(sv32, lab, nb, exp32), class_ref=ref)
        if cs.name != "overflow":
            same_classes(got, cs.mvbs()[0], "compute_Sv -> compute_MVBS float32 against the float64 oracle")
    judge(ds["Sv"].values, sv, dtype, f"Sv after compute_MVBS {dtype}", bound=sv_bound(cs))
    assert ds["echo_range"].data.cached_stats() == coord_stats(er, dtype)
    np.testing.assert_array_equal(ds["echo_range"].values, er.astype(dtype))
    assert warned(caplog) == cs.has_nan, [r.getMessage() for r in caplog.records]


# ---- binned on depth: ops.sv_mvbs_fused_depth (DEPTH 1 and 2), add_depth -> compute_MVBS ------------------------------
def _depth_rows(cs):
    tilt = np.linspace(0.0, 20.0, nc.P)
    scale = np.tile(np.cos(np.deg2rad(tilt)), (nc.C, 1))
    off = np.tile(np.linspace(3.0, 4.0, nc.P), (nc.C, 1))
    return tilt, scale, off


def _exp_depth(cs, dtype):
    """consolidate/api.py:221 in ``dtype``: the product rounded, then the sum (on the echo_range as ``dtype`` holds it)."""
    _, scale, off = _depth_rows(cs)
    er = cs.sv_er()[1].astype(dtype)
    return off.astype(dtype)[:, :, None] + scale.astype(dtype)[:, :, None] * er


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", FUSED_KEYS, ids=nc.case_id)
def test_fused_depth(ep, key, dtype):
    from echopype_amd import _lib, ops

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    _, scale, off = _depth_rows(cs)
    depth = _exp_depth(cs, dtype)
    d64 = depth.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        exp, _, r_left = ogrid.compute_MVBS(sv, d64, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin)
    lab, nb, _ = grid_labels(cs, d64)
    b_sv = sv_bound(cs) if dtype == "float32" else None
    b_mv = mvbs_bound(sv, lab, nb, exp, b_sv) if dtype == "float32" else None
    ref = f32_mvbs_classes(sv, lab, nb, exp.shape) if (dtype == "float32" and cs.name == "overflow") else None
    raw, coef, flags = power_inputs(ep, cs, dtype)
    bs, n_t = time_bins(ep, cs)
    rb = ogrid.parse_range_bin(cs.range_bin)
    tdt = ops.torch_dtype(dtype)
    for want_depth in (False, True):
        with _lib.launch_trace() as tr:
            res = ops.sv_mvbs_fused_depth(raw, coef, dev(scale), dev(off), bs, n_t, rb, exp.shape[2], dtype=tdt,
                                          want_depth=want_depth)
        assert "fused_sv_mvbs_kernel" in tr.kernels and "block_reduce_kernel" not in tr.kernels, tr.kernels
        what = f"ops.sv_mvbs_fused_depth {dtype} DEPTH={2 if want_depth else 1}"
        judge(res["MVBS"].cpu().numpy(), exp, dtype, what + ": MVBS", bound=b_mv, class_ref=ref)
        judge(res["Sv"].cpu().numpy(), sv, dtype, what + ": Sv", bound=b_sv)
        got = res["range_stats"].cpu().tolist()
        assert (got[0], got[1], int(got[2])) == coord_stats(depth, dtype), (what, got, coord_stats(depth, dtype))
        if want_depth:   # finite at the infinite samples, NaN exactly at the NaN samples: the oracle's bits, depth_rows' bits
            got_d = res["depth"].cpu().numpy()
            np.testing.assert_array_equal(np.isnan(got_d), np.isnan(cs.raw), err_msg=what + ": NaN pattern of depth")
            np.testing.assert_array_equal(got_d, depth, err_msg=what + ": depth")
            rows, st = ops.depth_rows(dev(scale), dev(off), coef=coef, mask_raw=raw, shape=raw.shape, dtype=tdt)
            np.testing.assert_array_equal(got_d, rows.cpu().numpy(), err_msg=what + ": depth against ops.depth_rows")
            np.testing.assert_array_equal(res["range_stats"].cpu().numpy(), st.cpu().numpy())


@pytest.mark.parametrize("written", [False, True], ids=["DEPTH1", "DEPTH2"])
@pytest.mark.parametrize("key", FUSED_KEYS, ids=nc.case_id)
def test_add_depth_then_mvbs(ep, key, written, caplog, monkeypatch):
    from echopype_amd import _lib

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    tilt, _, off = _depth_rows(cs)
    depth = _exp_depth(cs, "float64")
    with np.errstate(over="ignore", invalid="ignore"):
        exp, t_left, r_left = ogrid.compute_MVBS(sv, depth, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin)
    if written:
        monkeypatch.setenv("EPA_DEPTH_WITH_MVBS", "1")
    pt = cs.d["ping_time"]
    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING):
        ds = ep.calibrate.compute_Sv(echodata(ep, cs))
        ep.consolidate.add_depth(ds, depth_offset=ep.DataArray(off[0], ("ping_time",), coords={"ping_time": pt}),
                                 tilt=ep.DataArray(tilt, ("ping_time",), coords={"ping_time": pt}))
        mv = ep.commongrid.compute_MVBS(ds, range_var="depth", range_bin=cs.range_bin, ping_time_bin=cs.ping_time_bin)
        got = mv["Sv"].values
    assert "fused_sv_mvbs_kernel" in tr.kernels and "block_reduce_kernel" not in tr.kernels, tr.kernels
    assert ds["depth"].data.materialized == written
    np.testing.assert_array_equal(mv["depth"].values, r_left)
    np.testing.assert_array_equal(mv["ping_time"].values, t_left)
    judge(got, exp, "float64", "add_depth -> compute_MVBS")
    judge(ds["Sv"].values, sv, "float64", "add_depth -> compute_MVBS: Sv")
    assert ds["depth"].data.cached_stats() == coord_stats(depth, "float64")
    np.testing.assert_array_equal(ds["depth"].values, depth)
    assert warned(caplog) == cs.has_nan, [r.getMessage() for r in caplog.records]


# ---- compute_Sv_clean_MVBS: sv_noise_fast_kernel, sv_denoise_mvbs_* -----------------------------------------------------
def noise_block_bound(sv, x, a2, exp_blocks):
    """``f32_bounds.noise_estimate_bound`` with ``member_stats`` under it: a block may hold +-inf members."""
    Cn, Pn, Sn = sv.shape
    a2c = fb._a2(a2, Cn, Pn)
    with np.errstate(invalid="ignore", divide="ignore"):
        arg = sv - (20 * np.log10(np.where(x >= 1, x, 1.0)) + a2c * x)
        b_arg = fb.tl_bound(x, a2c) + fb.U * np.abs(arg)
    lab, nb = fb.labels_index(Cn, Pn, Sn, nc.PING_NUM, nc.RSN)
    per = mvbs_bound(arg, lab, nb, exp_blocks, b_arg)
    return np.max(np.where(np.isfinite(exp_blocks), per, -np.inf), axis=2)


def check_chain_f32(cs, ds, mv):
    """The float32 chain against the oracle run on exactly the float32 Sv and echo_range the route returns
    (test_gpu_kernels.py ``_check_noise_f32``'s scheme): Sv_noise under ``noise_bounds``, the SNR decision within the
    bound of its margin, Sv_corrected under ``noise_bounds`` where both keep the sample, the MVBS under ``mvbs_bound`` on
    the Sv_corrected members.  Pass 2 forms 10^(Sv/10) from the raw sample, not from the stored float32 Sv: its own Sv
    and the stored one both lie within ``sv_power_bound`` of the exact one, 2 b_sv apart at most, and Sv_corrected =
    10 log10(Ls - Ln) moves by kappa = Ls / (Ls - Ln) times that -- added to the bound and to the decision's.
    ``overflow``: where NumPy's own float32 evaluation of the same formula is +inf, that is the expected value."""
    f32 = np.float32
    sv32, er32 = ds["Sv"].values.astype(np.float64), ds["echo_range"].values.astype(np.float64)
    a2 = 2 * cs.d["absorption_indicative"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore", RuntimeWarning)
        exp_n, exp_c = oclean.remove_background_noise(sv32, er32, cs.d["absorption_indicative"], nc.PING_NUM, nc.RSN, None, "3.0dB")
        tl = 20 * np.log10(np.where(er32 >= 1, er32, 1)) + fb._a2(a2, nc.C, nc.P) * er32
        blocks = 10 * np.log10(oclean.coarsen_mean(10 ** ((sv32 - tl) / 10), nc.PING_NUM, nc.RSN))
        nb_exp = np.nanmin(blocks, axis=2)
        b_nb = noise_block_bound(sv32, er32, a2, blocks)
        lin_exp = 10 ** (sv32 / 10) - 10 ** (exp_n / 10)
        b_sn, b_c = fb.noise_bounds(sv32, er32, a2, nb_exp, b_nb, nc.PING_NUM, exp_n, lin_exp)
        kappa = 10 ** (sv32 / 10) / np.abs(lin_exp)
        b_c = b_c + fb.db_of_rel(kappa * fb.rel_of_db(2 * sv_bound(cs)))
        corr = 10 * np.log10(np.where(lin_exp > 0, lin_exp, np.nan))
        margin = np.where(np.isnan(corr), -np.inf, corr - exp_n - 3.0)
        if cs.name == "overflow":
            l32 = f32(10) ** (sv32.astype(f32) / f32(10)) - f32(10) ** (exp_n.astype(f32) / f32(10))
            exp_c = np.where(np.isposinf(l32) & ~np.isnan(exp_c), np.inf, exp_c)
    sn_got, sc_got = ds["Sv_noise"].values, ds["Sv_corrected"].values
    same_classes(sn_got, exp_n, "chain Sv_noise float32")
    fb.assert_f32_close(sn_got, exp_n, b_sn, "chain Sv_noise float32")
    keep_g, keep_e = ~np.isnan(sc_got), ~np.isnan(exp_c)
    fb.check_decisions(keep_g, keep_e, margin, b_c + b_sn + fb.U * np.abs(corr - exp_n), "chain float32: SNR decision",
                       max_frac=1e-3)
    both = keep_g & keep_e
    same_classes(np.where(both, sc_got, np.nan), np.where(both, exp_c, np.nan), "chain Sv_corrected float32")
    fb.assert_f32_close(np.where(both, sc_got, np.nan), np.where(both, exp_c, np.nan), b_c, "chain Sv_corrected float32")
    # the bins: the oracle's on the Sv_corrected and echo_range the route returned; a bin's terms are the kernel's own
    # Ls - Ln, which the stored Sv_corrected = fl(10 log10f(.)) gives back to (2 E_LOG + 1) u |Sv_corrected| + 1/2 ulp
    sc64 = sc_got.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        exp_mv, _, r_left = ogrid.compute_MVBS(sc64, er32, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin)
        b_m = (2 * fb.E_LOG + 1) * fb.U * np.abs(sc64) + fb.half_ulp(sc64)
    np.testing.assert_array_equal(mv["echo_range"].values, r_left)
    lab, nb, _ = grid_labels(cs, er32)
    ref = f32_mvbs_classes(sc64, lab, nb, exp_mv.shape) if cs.name == "overflow" else None
    judge(mv["Sv"].values, exp_mv, "float32", "chain MVBS float32", bound=mvbs_bound(sc64, lab, nb, exp_mv, b_m), class_ref=ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_chain(ep, key, dtype, caplog):
    """Sv, Sv_noise, Sv_corrected, their MVBS, the echo_range statistics pass 1 leaves and the NaN-coordinate warning of
    the two-pass chain.  (``overflow`` holds Sv of 3060 .. 3082 dB: 10^(g raw / 10) (s - d)^2 alone is beyond float64
    there, 10^(Sv/10) is not.)"""
    from echopype_amd import _lib

    cs = nc.build(*key)
    sv, er = cs.sv_er()
    exp_n, exp_c = cs.clean()
    caplog.clear()
    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING):
        ds, mv = ep.compute_Sv_clean_MVBS(echodata(ep, cs), nc.PING_NUM, nc.RSN, range_bin=cs.range_bin,
                                          ping_time_bin=cs.ping_time_bin, dtype=dtype)
        got_mv = mv["Sv"].values
    fast = cs.S % 4 == 0
    assert ("sv_noise_fast_kernel" in tr.kernels) == fast, tr.kernels
    assert any(k.startswith("sv_denoise_mvbs_") for k in tr.kernels) == fast, tr.kernels
    assert warned(caplog) == cs.has_nan, [r.getMessage() for r in caplog.records]
    if fast:   # (the generic kernel leaves the maximum only)
        assert ds["echo_range"].data.cached_stats() == coord_stats(er, dtype)
    exp_mv, t_left, r_left = cs.mvbs(on="Sv_corrected")
    assert got_mv.shape == exp_mv.shape, (got_mv.shape, exp_mv.shape)
    np.testing.assert_array_equal(mv["echo_range"].values, r_left)
    np.testing.assert_array_equal(mv["ping_time"].values, t_left)
    np.testing.assert_array_equal(ds["echo_range"].values, er.astype(dtype))
    if dtype == "float64":
        judge(ds["Sv"].values, sv, dtype, "chain Sv")
        judge(ds["Sv_noise"].values, exp_n, dtype, "chain Sv_noise")
        judge(ds["Sv_corrected"].values, exp_c, dtype, "chain Sv_corrected", rtol=1e-7)
        judge(got_mv, exp_mv, dtype, "chain MVBS", rtol=1e-7)
    else:
        judge(ds["Sv"].values, sv, dtype, "chain Sv float32", bound=sv_bound(cs))
        check_chain_f32(cs, ds, mv)


# ---- the materialised Sv: commongrid.compute_MVBS (block_reduce_kernel), ops.mvbs_index, ops.nasc ----------------------
def _as_stored(cs, dtype):
    """The oracle's Sv and echo_range as arrays of ``dtype`` hold them, and their float64 copies (what a kernel reads)."""
    sv, er = cs.sv_er()
    sv_t, er_t = sv.astype(dtype), er.astype(dtype)
    return sv_t, er_t, sv_t.astype(np.float64), er_t.astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("skipna", [True, False])
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_mvbs_of_the_sv_array(ep, key, skipna, dtype, caplog):
    from echopype_amd import _lib

    cs = nc.build(*key)
    sv_t, er_t, sv64, er64 = _as_stored(cs, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        exp, t_left, r_left = ogrid.compute_MVBS(sv64, er64, cs.d["ping_time"], cs.range_bin, cs.ping_time_bin, skipna=skipna)
    dims = ("channel", "ping_time", "range_sample")
    ds = ep.Dataset(coords={"channel": cs.d["channel"], "ping_time": cs.d["ping_time"], "range_sample": np.arange(cs.S)})
    ds["Sv"], ds["echo_range"] = (dims, sv_t), (dims, er_t)
    with _lib.launch_trace() as tr, caplog.at_level(logging.WARNING):
        mv = ep.commongrid.compute_MVBS(ds, range_bin=cs.range_bin, ping_time_bin=cs.ping_time_bin, skipna=skipna)
        got = mv["Sv"].values
    assert "block_reduce_kernel" in tr.kernels, tr.kernels
    np.testing.assert_array_equal(mv["echo_range"].values, r_left)
    np.testing.assert_array_equal(mv["ping_time"].values, t_left)
    lab_all, nb, _ = grid_labels(cs, er64)
    lab, nan_bins = lab_all, np.zeros(0, np.int64)
    if not skipna:   # a NaN member makes the bin NaN: no finite mean to bound there
        nan_bins = np.unique(lab_all[np.isnan(sv64) & (lab_all >= 0)])
        lab = np.where(np.isin(lab_all, nan_bins), -1, lab_all)
    ref = None
    if dtype == "float32" and cs.name == "overflow":
        ref = f32_mvbs_classes(sv64, lab_all, nb, exp.shape)
        ref.reshape(-1)[nan_bins] = np.nan
    judge(got, exp, dtype, f"compute_MVBS of the Sv array {dtype} skipna={skipna}",
          bound=mvbs_bound(sv64, lab, nb, exp) if dtype == "float32" else None, class_ref=ref)
    assert warned(caplog) == cs.has_nan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_mvbs_index(ep, key, dtype):
    from echopype_amd import _lib, ops

    cs = nc.build(*key)
    sv_t, er_t, sv64, er64 = _as_stored(cs, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        exp, exp_r = ogrid.compute_MVBS_index_binning(sv64, er64, nc.RSN, nc.PING_NUM)
    with _lib.launch_trace() as tr:
        got, rmin = ops.mvbs_index(dev(sv_t), nc.PING_NUM, nc.RSN, range=dev(er_t))
    assert "block_reduce_kernel" in tr.kernels, tr.kernels
    lab, nb = fb.labels_index(nc.C, nc.P, cs.S, nc.PING_NUM, nc.RSN)
    ref = f32_mvbs_classes(sv64, lab, nb, exp.shape) if (dtype == "float32" and cs.name == "overflow") else None
    judge(got.cpu().numpy(), exp, dtype, f"ops.mvbs_index {dtype}",
          bound=mvbs_bound(sv64, lab, nb, exp) if dtype == "float32" else None, class_ref=ref)
    np.testing.assert_array_equal(rmin.cpu().numpy(), exp_r.astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", KEYS, ids=nc.case_id)
def test_nasc(ep, key, dtype):
    from echopype_amd import _lib, ops

    cs = nc.build(*key)
    sv_t, er_t, sv64, er64 = _as_stored(cs, dtype)
    rb = ogrid.parse_range_bin(cs.range_bin)
    r_edges = ogrid.range_edges(er64, rb)
    dist = np.arange(nc.P, dtype=np.float64)             # one distance bin per 6 pings: the time bins
    d_edges = np.arange(0.0, nc.P + 6.0, 6.0)
    with np.errstate(over="ignore", invalid="ignore"):
        exp, _ = onasc.compute_raw_NASC(sv64, er64, dist, cs.d["ping_time"], r_edges, d_edges)
    bs, n_d = time_bins(ep, cs)
    assert n_d == len(d_edges) - 1
    with _lib.launch_trace() as tr:
        got = ops.nasc(dev(sv_t), dev(er_t), bs, n_d, rb, len(r_edges) - 1)
    assert "nasc_accumulate_kernel" in tr.kernels and "nasc_finalize_kernel" in tr.kernels, tr.kernels
    got = got.cpu().numpy()
    if dtype == "float64":
        same_classes(got, exp, "ops.nasc")
        fin = np.isfinite(exp)
        np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-10)     # (test_gpu_fuzz.py's bar for NASC)
        return
    lab, nb, _ = grid_labels(cs, er64)
    n, _, rho = member_stats(sv64, lab, nb)
    with np.errstate(invalid="ignore"):
        bound = fb.nasc_rel_bound(n, rho).reshape(exp.shape) * np.abs(exp)
    if cs.name == "overflow":   # float32 terms summed in double (a term beyond float32 is +inf, a sum of finite ones is
        # not), and the cell itself rounded to float32: 10^37 / n * 4 pi 1852^2 h is beyond it, too
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            lin32 = (np.float32(10.0) ** (sv_t / np.float32(10.0))).astype(np.float64)
            ref, _ = onasc.compute_raw_NASC(10 * np.log10(lin32), er64, dist, cs.d["ping_time"], r_edges, d_edges)
            ref = ref.astype(np.float32)
        judge(got, exp, dtype, "ops.nasc float32", bound=bound, class_ref=ref)
    else:
        judge(got, exp, dtype, "ops.nasc float32", bound=bound)
