"""float32 kernels where float32 goes wrong, against the float64 oracle under the derived bounds of tests/f32_bounds.py:
long accumulations (bins of 10^4 ... 10^6 samples, a constant field and one 60 dB above the rest of its bin), far
range, strong targets near and above 0 dB, cancellation in noise removal, and underflow of 10^(Sv/10).
``epa_launch_trace`` pins the kernel that served each case.  Needs a real MI355X: `pytest -m gpu`."""
import warnings

import numpy as np
import pytest

import f32_bounds as fb
from oracle import calibrate as ocal

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import _lib, ops, synth

    return torch, ops, synth, _lib


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def _kw(d, cal_type="Sv"):
    gain = ocal.vend_cal_params_power(d["transmit_duration_nominal"], d["pulse_length"], d["gain_correction"])
    sa = ocal.vend_cal_params_power(d["transmit_duration_nominal"], d["pulse_length"], d["sa_correction"])
    return dict(sonar="EK60", cal_type=cal_type, sample_interval=d["sample_interval"],
                sound_speed=d["sound_speed_indicative"], absorption=d["absorption_indicative"],
                transmit_power=d["transmit_power"], tau_nominal=d["transmit_duration_nominal"], gain=gain,
                sa_correction=sa, psi=d["equivalent_beam_angle"], f_nominal=d["frequency_nominal"],
                tau_eff=d["transmit_duration_nominal"][:, 0])


def _coef(torch, ops, d, cal_type="Sv"):
    f64 = torch.float64
    return ops.power_coef_ek(
        _dev(torch, d["sample_interval"], f64), _dev(torch, d["transmit_duration_nominal"], f64),
        _dev(torch, d["transmit_power"], f64), _dev(torch, d["sound_speed_indicative"], f64),
        _dev(torch, d["absorption_indicative"], f64), _dev(torch, d["gain_correction"], f64),
        _dev(torch, d["sa_correction"], f64), _dev(torch, d["equivalent_beam_angle"], f64),
        _dev(torch, d["frequency_nominal"], f64), _dev(torch, d["transmit_duration_nominal"][:, 0].copy(), f64),
        sonar="EK60", cal_type=cal_type, pulse_length=_dev(torch, d["pulse_length"], f64),
        gain_is_table=True, sa_is_table=True)


# ------------------------------------------------------------------------------------------------ long accumulations
P_LONG, S_LONG = 1000, 1000


def _field(kind):
    """(1, 1000, 1000) float32 Sv: constant, or one sample per 10^4-sample tile 60 dB above the rest."""
    sv = np.full((1, P_LONG, S_LONG), -72.3, np.float32)
    if kind == "spike60":
        sv[0, ::10, 500] = np.float32(-12.3)   # one per 10 pings x 1000 samples = every 10^4-sample bin has one
    return sv


def _exact_mean_db(sv, lab, nb):
    L = 10.0 ** (sv.astype(np.float64).ravel() / 10)
    lab = lab.ravel()
    return 10 * np.log10(np.bincount(lab, L, minlength=nb) / np.bincount(lab, minlength=nb))


@pytest.mark.parametrize("kind", ["constant", "spike60"])
@pytest.mark.parametrize("ping_num", [10, 100, 1000])          # bins of 10^4, 10^5, 10^6 samples
def test_long_bins_index_binned(env, kind, ping_num):
    torch, ops, synth, _lib = env
    sv = _field(kind)
    lab, nb = fb.labels_index(1, P_LONG, S_LONG, ping_num, S_LONG)
    exp = _exact_mean_db(sv, lab, nb).reshape(1, -1, 1)
    with _lib.launch_trace() as tr:
        got, _ = ops.mvbs_index(_dev(torch, sv), ping_num, S_LONG)
    assert "block_reduce_kernel" in tr.kernels, tr.kernels
    b = fb.mvbs_bound(sv.astype(np.float64), lab, nb, exp)
    fb.assert_f32_close(got.cpu().numpy(), exp, b, f"index-binned {kind} n={ping_num * S_LONG}")
    if kind == "constant":  # the known answer
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - float(sv[0, 0, 0])) <= b)


@pytest.mark.parametrize("kind", ["constant", "spike60"])
@pytest.mark.parametrize("ping_num", [10, 100, 1000])
def test_long_bins_block_reduce_generic(env, kind, ping_num):
    """ops.mvbs (epa_mvbs) on an Sv array with its echo_range array: the generic block_reduce kernel; one range bin
    spans every sample of ping_num pings."""
    torch, ops, synth, _lib = env
    sv = _field(kind)
    er = np.broadcast_to((np.arange(S_LONG) * 0.25).astype(np.float32), sv.shape).copy()
    ns = np.arange(P_LONG, dtype=np.int64) * 10**9
    n_t = P_LONG // ping_num
    bs = ops.time_bin_offsets(_dev(torch, ns), 0, ping_num * 10**9, n_t)
    lab, nb = fb.labels_index(1, P_LONG, S_LONG, ping_num, S_LONG)
    exp = _exact_mean_db(sv, lab, nb).reshape(1, n_t, 1)
    with _lib.launch_trace() as tr:
        res = ops.mvbs(_dev(torch, sv), bs, n_t, 1000.0, 1, range=_dev(torch, er))
    assert "block_reduce_kernel" in tr.kernels, tr.kernels
    b = fb.mvbs_bound(sv.astype(np.float64), lab, nb, exp)
    fb.assert_f32_close(res["MVBS"].cpu().numpy(), exp, b, f"block_reduce {kind} n={ping_num * S_LONG}")


@pytest.mark.parametrize("kind", ["constant", "spike60"])
@pytest.mark.parametrize("ping_num", [10, 100, 1000])
def test_long_bins_fused(env, kind, ping_num):
    """The fused Sv -> MVBS kernel: raw samples chosen so that the oracle's Sv is the field (to float32 rounding of
    raw); one range bin spans the ping's samples, time bins of ping_num pings."""
    torch, ops, synth, _lib = env
    d = synth.ek60_numpy(1, P_LONG, S_LONG, seed=4)
    d["backscatter_r"][:] = 0.0
    kw = _kw(d)
    t = ocal.cal_power_ek_terms(d["backscatter_r"].astype(np.float64), **kw)
    raw = (_field(kind).astype(np.float64) - t["spreading"] - t["absorb"] - t["const"]).astype(np.float32)
    raw[np.isnan(raw)] = np.float32(-100.0)          # samples 0..2 (R' <= 0): NaN Sv whatever raw is
    d["backscatter_r"] = raw
    exp_sv, er = ocal.cal_power_ek(raw, **kw)
    ns = np.arange(P_LONG, dtype=np.int64) * 10**9
    n_t = P_LONG // ping_num
    bs = ops.time_bin_offsets(_dev(torch, ns), 0, ping_num * 10**9, n_t)
    rbin = float(np.nanmax(er)) + 1.0
    lab, nb = fb.labels_index(1, P_LONG, S_LONG, ping_num, S_LONG)
    lab = np.where(np.isnan(exp_sv), -1, lab)
    b_sv = fb.sv_power_bound(ocal.cal_power_ek_terms(raw, **kw), exp_sv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        L = 10.0 ** (exp_sv.ravel() / 10)
        use = lab.ravel() >= 0
        exp = (10 * np.log10(np.bincount(lab.ravel()[use], L[use], minlength=nb)
                             / np.bincount(lab.ravel()[use], minlength=nb))).reshape(1, n_t, 1)
    coef = _coef(torch, ops, d)
    b_mv = fb.mvbs_bound(exp_sv, lab, nb, exp, b_sv)
    # few output cells: the planner splits the samples over workgroups and takes the two-stage generic kernel; with
    # the range maximum it keeps one stage, and the fused kernel serves
    for want_max, kernel in ((True, "fused_sv_mvbs_kernel"), (False, "block_reduce_kernel")):
        with _lib.launch_trace() as tr:
            res = ops.sv_mvbs_fused(_dev(torch, raw), coef, bs, n_t, rbin, 1, dtype=torch.float32,
                                    want_range_max=want_max)
        assert kernel in tr.kernels and ("fused_sv_mvbs_kernel" in tr.kernels) == want_max, tr.kernels
        fb.assert_f32_close(res["Sv"].cpu().numpy(), exp_sv, b_sv, f"{kernel} Sv {kind}")
        fb.assert_f32_close(res["MVBS"].cpu().numpy(), exp, b_mv, f"{kernel} MVBS {kind} n={ping_num * S_LONG}")


@pytest.mark.parametrize("kind", ["constant", "spike60"])
@pytest.mark.parametrize("ping_num", [10, 100, 1000])
def test_long_bins_depth_binned(env, kind, ping_num):
    """The fused kernel binned on depth = offset + scale * echo_range (add_depth fused into the pass, float32 depth):
    one depth bin spans the ping's samples, time bins of ping_num pings.  Bin membership is decided on the float32
    depth; the oracle bins on exactly that depth (offset + scale * float32(echo_range), two float32 roundings)."""
    torch, ops, synth, _lib = env
    d = synth.ek60_numpy(1, P_LONG, S_LONG, seed=4)
    d["backscatter_r"][:] = 0.0
    kw = _kw(d)
    t = ocal.cal_power_ek_terms(d["backscatter_r"].astype(np.float64), **kw)
    raw = (_field(kind).astype(np.float64) - t["spreading"] - t["absorb"] - t["const"]).astype(np.float32)
    raw[np.isnan(raw)] = np.float32(-100.0)
    d["backscatter_r"] = raw
    exp_sv, er = ocal.cal_power_ek(raw, **kw)
    scale, off = np.full((1, P_LONG), np.cos(np.deg2rad(7.0))), np.full((1, P_LONG), 1.5)
    depth = off.astype(np.float32)[:, :, None] + scale.astype(np.float32)[:, :, None] * er.astype(np.float32)
    ns = np.arange(P_LONG, dtype=np.int64) * 10**9
    n_t = P_LONG // ping_num
    bs = ops.time_bin_offsets(_dev(torch, ns), 0, ping_num * 10**9, n_t)
    rbin = float(np.nanmax(depth)) + 1.0
    lab, nb = fb.labels_index(1, P_LONG, S_LONG, ping_num, S_LONG)
    lab = np.where(np.isnan(exp_sv) | np.isnan(depth), -1, lab)
    b_sv = fb.sv_power_bound(ocal.cal_power_ek_terms(raw, **kw), exp_sv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        L = 10.0 ** (exp_sv.ravel() / 10)
        use = lab.ravel() >= 0
        exp = (10 * np.log10(np.bincount(lab.ravel()[use], L[use], minlength=nb)
                             / np.bincount(lab.ravel()[use], minlength=nb))).reshape(1, n_t, 1)
    coef = _coef(torch, ops, d)
    with _lib.launch_trace() as tr:
        res = ops.sv_mvbs_fused_depth(_dev(torch, raw), coef, _dev(torch, scale), _dev(torch, off), bs, n_t, rbin, 1,
                                      dtype=torch.float32, want_depth=True)
    assert "fused_sv_mvbs_kernel" in tr.kernels and "block_reduce_kernel" not in tr.kernels, tr.kernels
    np.testing.assert_array_equal(res["depth"].cpu().numpy(), depth)     # the float32 depth the bins were decided on
    fb.assert_f32_close(res["Sv"].cpu().numpy(), exp_sv, b_sv, f"depth-binned Sv {kind}")
    fb.assert_f32_close(res["MVBS"].cpu().numpy(), exp, fb.mvbs_bound(exp_sv, lab, nb, exp, b_sv),
                        f"depth-binned MVBS {kind} n={ping_num * S_LONG}")


@pytest.mark.parametrize("kind", ["constant", "spike60"])
@pytest.mark.parametrize("ping_num", [10, 100, 1000])
def test_long_bins_nasc(env, kind, ping_num):
    """compute_raw_NASC's kernel on a float32 Sv and depth: one depth bin spans the ping's samples, distance bins of
    ping_num pings.  NASC = mean(10^(Sv/10)) * h_mean * 4 pi 1852^2 with h_mean = (S - 1) * 0.25 m exactly."""
    torch, ops, synth, _lib = env
    sv = _field(kind)
    depth = np.broadcast_to((np.arange(S_LONG) * 0.25).astype(np.float32), sv.shape).copy()
    n_d = P_LONG // ping_num
    bs = _dev(torch, np.arange(0, P_LONG + 1, ping_num, dtype=np.int32))
    lab, nb = fb.labels_index(1, P_LONG, S_LONG, ping_num, S_LONG)
    n, m, rho = fb.bin_stats(lab, nb, sv.astype(np.float64))
    exp = (m * ((S_LONG - 1) * 0.25) * 4 * np.pi * 1852.0**2).reshape(1, n_d, 1)
    with _lib.launch_trace() as tr:
        got = ops.nasc(_dev(torch, sv), _dev(torch, depth), bs, n_d, 1000.0, 1)
    assert "nasc_accumulate_kernel" in tr.kernels and "nasc_finalize_kernel" in tr.kernels, tr.kernels
    b = fb.nasc_rel_bound(n, rho).reshape(exp.shape) * np.abs(exp)
    fb.assert_f32_close(got.cpu().numpy(), exp, b, f"NASC {kind} n={ping_num * S_LONG}")


# ------------------------------------------------------------------------------------------------ far range, strong targets
@pytest.mark.parametrize("cal_type", ["Sv", "TS"])
def test_far_range_and_strong_targets(env, cal_type):
    """A sample interval twice the usual takes 20 000 samples to ~7.6 km of echo_range: 20 log10 r and 2 alpha r
    dominate the terms.  Ping 0 holds strong targets (raw +40 dB): TS above 0 dB, where the old bar is 1e-3 dB.
    Neither planner limits S: K1 tiles any row in 1024-sample pieces, and the fused kernel's limit is its range grid
    (sum + count of every range bin in 64 KiB of LDS).  So the fused call bins the whole 7.6 km on 2 m bins
    (3 800 bins, 30 KiB), well inside that grid, and both the K1 piece kernel and the fused kernel are pinned."""
    torch, ops, synth, _lib = env
    C, P, S = 2, 8, 20000
    d = synth.ek60_numpy(C, P, S, seed=8)
    d["sample_interval"] = d["sample_interval"] * 2
    # 0.01 dB/m (38 kHz water): 2 alpha r reaches 150 dB.  (With the generator's higher-frequency absorption Sv passes
    # +385 dB at 7.6 km, where 10^(Sv/10) overflows float32 and the float32 MVBS is +inf by its own arithmetic.)
    d["absorption_indicative"] = np.full_like(d["absorption_indicative"], 0.01)
    d["backscatter_r"][:, 0, :] = np.float32(40.0)
    kw = _kw(d, cal_type)
    exp, er = ocal.cal_power_ek(d["backscatter_r"], **kw)
    b = fb.sv_power_bound(ocal.cal_power_ek_terms(d["backscatter_r"], **kw), exp)
    coef = _coef(torch, ops, d, cal_type)
    raw = _dev(torch, d["backscatter_r"])
    with _lib.launch_trace() as tr:
        out, _ = ops.sv_power(raw, coef, cal_type=cal_type, dtype=torch.float32)
    assert tr.kernels.count("sv_power_piece_kernel") == 1 and "sv_power_kernel" not in tr.kernels, tr.kernels
    got = out.cpu().numpy()
    fb.assert_f32_close(got, exp, b, f"far range {cal_type}")
    last = np.isfinite(exp[:, :, -64:])
    assert last.any() and np.nanmax(er) > 3000
    assert np.nanmax(exp) < 380.0                 # 10^(Sv/10) stays inside float32's range
    fb.assert_f32_close(got[:, :, -64:], exp[:, :, -64:], b[:, :, -64:], f"far range {cal_type}: last samples")
    if cal_type == "TS":
        assert np.nanmax(exp[:, 0]) > 0.0         # the strong targets do reach positive dB
    # the fused kernel on the same samples: its Sv and the MVBS of 2 m x 4-ping bins
    ns = np.arange(P, dtype=np.int64) * 10**9
    bs = ops.time_bin_offsets(_dev(torch, ns), 0, 4 * 10**9, 2)
    n_r = int(np.nanmax(er) // 2.0) + 1
    with _lib.launch_trace() as tr:
        res = ops.sv_mvbs_fused(raw, coef, bs, 2, 2.0, n_r, cal_type=cal_type, dtype=torch.float32,
                                want_range_max=True)
    assert "fused_sv_mvbs_kernel" in tr.kernels and "block_reduce_kernel" not in tr.kernels, tr.kernels
    fb.assert_f32_close(res["Sv"].cpu().numpy(), exp, b, f"far range fused {cal_type}")
    edges = np.arange(0, n_r + 1) * 2.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        from oracle import commongrid as ogrid

        ir = ogrid.bin_index(er, edges)
        it = (np.arange(P) // 4)[None, :, None]
        c = np.arange(C)[:, None, None]
        lab = np.where((ir >= 0) & ~np.isnan(exp), (c * 2 + it) * n_r + ir, -1)
        nb = C * 2 * n_r
        L = 10.0 ** (exp.ravel() / 10)
        use = lab.ravel() >= 0
        mexp = (10 * np.log10(np.bincount(lab.ravel()[use], L[use], minlength=nb)
                              / np.bincount(lab.ravel()[use], minlength=nb))).reshape(C, 2, n_r)
    fb.assert_f32_close(res["MVBS"].cpu().numpy(), mexp, fb.mvbs_bound(exp, lab, nb, mexp, b),
                        f"far range fused MVBS {cal_type}")


# ------------------------------------------------------------------------------------------------ noise removal
def test_noise_removal_cancellation(env):
    """noise_apply on a given per-block noise: samples at Sv_noise + 3 dB +- {0.1, 1e-3, 1e-5} dB (at the SNR
    threshold) and at Sv_noise + 0.01 dB (condition number ~430)."""
    torch, ops, synth, _lib = env
    C, P, S, ping_num = 2, 40, 2048, 20
    rng = np.random.default_rng(12)
    er = np.broadcast_to((np.arange(S) * 0.19).astype(np.float32), (C, P, S)).astype(np.float64)
    a2 = np.full((C, P), 2 * 0.0098)
    nb = np.array([[-131.0, -129.7], [-133.2, -130.1]])
    with np.errstate(divide="ignore"):
        tl = 20 * np.log10(np.where(er >= 1, er, 1)) + a2[:, :, None] * er
    sn_exp = nb[:, np.arange(P) // ping_num][:, :, None] + tl
    off = rng.uniform(-10, 20, (C, P, S))
    deltas = np.array([3.1, 2.9, 3.001, 2.999, 3.00001, 2.99999, 0.01])
    off[:, :, 100:100 + 7 * 128] = np.tile(deltas, 128)[None, None, :]
    sv = (sn_exp + off).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        lin_exp = 10 ** (sv / 10) - 10 ** (sn_exp / 10)
        corr = 10 * np.log10(np.where(lin_exp > 0, lin_exp, np.nan))
        exp_c = np.where(corr - sn_exp > 3.0, corr, np.nan)
    with _lib.launch_trace() as tr:
        sn, sc = ops.noise_apply(_dev(torch, sv, torch.float32), _dev(torch, a2), _dev(torch, nb), ping_num, 3.0,
                                 range=_dev(torch, er, torch.float32))
    assert "noise_apply_kernel" in tr.kernels, tr.kernels
    b_sn, b_c = fb.noise_bounds(sv, er, a2, nb, np.zeros_like(nb), ping_num, sn_exp, lin_exp)
    fb.assert_f32_close(sn.cpu().numpy(), sn_exp, b_sn, "cancellation: Sv_noise")
    g = sc.cpu().numpy().astype(np.float64)
    margin = np.where(np.isnan(corr), -np.inf, corr - sn_exp - 3.0)
    nflip = fb.check_decisions(~np.isnan(g), ~np.isnan(exp_c), margin, b_c + b_sn + fb.U * np.abs(corr - sn_exp),
                               "cancellation: SNR decision")
    both = ~np.isnan(g) & ~np.isnan(exp_c)
    fb.assert_f32_close(np.where(both, g, np.nan), np.where(both, exp_c, np.nan), b_c, "cancellation: Sv_corrected")
    # the condition number reaches the bound: Sv_noise + 0.01 dB carries ~430 x the relative error of 10^(Sv/10)
    kappa = 10 ** (sv / 10) / lin_exp
    assert np.nanmax(kappa[:, :, 100:996]) > 400
    # flips, if any, lie among the samples placed within 1e-3 dB of the threshold
    flip_s = np.nonzero(np.isnan(g) != np.isnan(exp_c))[2]
    assert nflip == flip_s.size and np.all((flip_s >= 100) & (flip_s < 100 + 7 * 128)), flip_s
    assert np.all(np.isin((flip_s - 100) % 7, [2, 3, 4, 5])), flip_s


# ------------------------------------------------------------------------------------------------ underflow
def test_underflow_class_matches_float32_reference(env):
    """Sv <= -380 dB into a float32 MVBS: 10^(Sv/10) is subnormal or 0 in float32.  The contract is the reference's
    own float32 NumPy arithmetic on a float32 Sv: the class (finite / -inf / NaN) of every bin as NumPy's float32
    evaluation of 10 * log10(mean(10 ** (Sv / 10))) gives it."""
    torch, ops, synth, _lib = env
    levels = np.array([-380.0, -390.0, -400.0, -420.0, -440.0, -455.0, -470.0, -600.0, -80.0], np.float32)
    C, P, S, rsn = 1, 4, 64 * len(levels), 64
    sv = np.repeat(levels, rsn)[None, None, :].repeat(P, axis=1).astype(np.float32)
    sv[0, 1, ::3] = np.float32(-1000.0)            # a bin of mixed subnormal and zero terms
    with np.errstate(divide="ignore", under="ignore"):
        lin = np.float32(10.0) ** (sv / np.float32(10.0))
        m = lin.reshape(C, 1, P, len(levels), rsn).mean(axis=(2, 4), dtype=np.float32)
        ref = (np.float32(10.0) * np.log10(m)).astype(np.float32)
    with _lib.launch_trace() as tr:
        got, _ = ops.mvbs_index(_dev(torch, sv), P, rsn)
    assert "block_reduce_kernel" in tr.kernels, tr.kernels
    g = got.cpu().numpy()

    def cls(a):
        return np.where(np.isnan(a), 2, np.where(np.isneginf(a), 1, 0))

    np.testing.assert_array_equal(cls(g), cls(ref), err_msg=f"class of float32 MVBS: got {g}, NumPy float32 {ref}")
    assert (cls(ref) == 1).any() and (cls(ref) == 0).sum() >= 5
