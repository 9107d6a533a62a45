"""CPU self-test of the float32 error bounds of tests/f32_bounds.py.

Soundness: a NumPy float32 emulation of each kernel's operation order stays within its bound on random and adversarial
inputs.  An fma is emulated as the float64 product-sum rounded once to float32; that double rounding is off from a true
fma by at most 2^-53 relative, which the bounds' float64 slack absorbs.  Order-free sums are emulated in several orders.
Sharpness: each perturbation the float32 bar of 1e-3 could not see FAILS the new check and still PASSES the old bar."""
import warnings

import numpy as np
import pytest

import f32_bounds as fb
from echopype_amd import synth
from oracle import calibrate as ocal
from oracle import clean as oclean

f32 = np.float32


def _old_ok(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    f = np.isfinite(exp)
    return bool(np.all(np.abs(got[f] - exp[f]) / np.maximum(np.abs(exp[f]), 1.0) <= fb.OLD_RTOL))


def _new_ok(got, exp, bound):
    """False only when the check fails on the bound itself (NaN pattern, a missing bound or the old bar re-raise)."""
    try:
        fb.assert_f32_close(got, exp, bound)
        return True
    except AssertionError as e:
        if "dB > bound" in str(e):
            return False
        raise


def _ek60_case(C=2, P=12, S=3000, cal_type="Sv", si_scale=1.0, seed=5):
    d = synth.ek60_numpy(C, P, S, seed=seed)
    d["sample_interval"] = d["sample_interval"] * si_scale
    gain = ocal.vend_cal_params_power(d["transmit_duration_nominal"], d["pulse_length"], d["gain_correction"])
    sa = ocal.vend_cal_params_power(d["transmit_duration_nominal"], d["pulse_length"], d["sa_correction"])
    kw = dict(sonar="EK60", cal_type=cal_type, sample_interval=d["sample_interval"],
              sound_speed=d["sound_speed_indicative"], absorption=d["absorption_indicative"],
              transmit_power=d["transmit_power"], tau_nominal=d["transmit_duration_nominal"], gain=gain,
              sa_correction=sa, psi=d["equivalent_beam_angle"], f_nominal=d["frequency_nominal"],
              tau_eff=d["transmit_duration_nominal"][:, 0])
    return d, kw


def _emulate_cal_power(raw, kw):
    """cal_power_sample<float> (csrc/sample_math.h:62-75) over the row constants power_coef_ek_kernel computes in
    double (csrc/power_coef.hip:51-92), EK60 (d = 2, g = 1)."""
    C, P, S = raw.shape
    terms = ocal.cal_power_ek_terms(raw.astype(np.float64), **kw)
    si = np.broadcast_to(np.asarray(kw["sample_interval"], np.float64).reshape(C, -1), (C, P))[:, :, None]
    cw = np.broadcast_to(np.asarray(kw["sound_speed"], np.float64).reshape(C, -1), (C, P))[:, :, None]
    k = si * cw / 2
    shift = 2 * si * cw / 2
    A = terms["const"][:, :, :1]
    n = terms["nspread"]
    A0 = (A + n * np.log10(k)).astype(f32)
    alpha2 = (2 * np.broadcast_to(np.asarray(kw["absorption"], np.float64).reshape(C, -1), (C, P))[:, :, None]).astype(f32)
    s = np.arange(S, dtype=np.float64)[None, None, :]
    R = (s * si) * (cw / 2)
    rtd = R - shift
    with np.errstate(invalid="ignore", divide="ignore"):
        nL = (f32(n) * np.log10((s - 2.0).astype(f32))).astype(f32)
        a = (raw.astype(np.float64) + nL.astype(np.float64)).astype(f32)                            # fma(g, raw, nL)
        b = (alpha2.astype(np.float64) * rtd.astype(f32) + A0.astype(np.float64)).astype(f32)        # fma(a2, rt, A0)
        out = (a + b).astype(f32)
    out = np.where(rtd > 0, out, np.nan)
    return out, terms


@pytest.mark.parametrize("cal_type", ["Sv", "TS"])
@pytest.mark.parametrize("si_scale", [1.0, 40.0])     # 40 x: 3000 samples reach ~4.4 km
def test_sv_power_emulation_within_bound(cal_type, si_scale):
    d, kw = _ek60_case(cal_type=cal_type, si_scale=si_scale)
    raw = d["backscatter_r"].copy()
    raw[0, 0, :] = np.float32(60.0)          # strong targets: positive dB, where the old bar is absolute
    raw[1, 1, ::7] = np.float32(-150.0)
    out, terms = _emulate_cal_power(raw, kw)
    exp, _ = ocal.cal_power_ek(raw.astype(np.float64), **kw)
    exp = np.where(np.isnan(raw), np.nan, exp)
    b = fb.sv_power_bound(terms, exp)
    err, ratio = fb.assert_f32_close(np.where(np.isnan(raw), np.nan, out), exp, b, f"emulated {cal_type}")
    assert 0 < ratio <= 1.0


def _emulate_mean(sv32, labels, nbins, order):
    """lin = exp10f(v * 0.1f) (rounded float64 10^x: 0.5 ulp), float32 sums in the given member order, s / n,
    10 * log10f."""
    v = sv32.ravel()
    lab = labels.ravel()
    use = (lab >= 0) & ~np.isnan(v)
    arg = (v.astype(np.float64) * np.float64(f32(0.1))).astype(f32)
    lin = (10.0 ** arg.astype(np.float64)).astype(f32)
    idx = np.flatnonzero(use)
    if order == "reverse":
        idx = idx[::-1]
    elif order == "random":
        idx = np.random.default_rng(1).permutation(idx)
    s = np.zeros(nbins, f32)
    n = np.zeros(nbins, np.int64)
    if order == "pairwise":  # tree: sort by bin, sum each bin pairwise in float32
        for bi in np.unique(lab[idx]):
            m = lin[idx[lab[idx] == bi]].astype(f32)
            while m.size > 1:
                if m.size % 2:
                    m = np.append(m, f32(0))
                m = (m[0::2] + m[1::2]).astype(f32)
            s[bi] = m[0]
            n[bi] = int((lab[idx] == bi).sum())
    else:
        for i in idx:  # float32 accumulation, one term at a time
            s[lab[i]] = f32(s[lab[i]] + lin[i])
            n[lab[i]] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (s / n.astype(f32)).astype(f32)
        out = (f32(10) * np.log10(mean)).astype(f32)
    return np.where(n > 0, out, np.nan)


@pytest.mark.parametrize("field", ["random", "spike60", "constant", "deep"])
@pytest.mark.parametrize("order", ["forward", "reverse", "random", "pairwise"])
def test_bin_mean_emulation_within_bound(field, order):
    rng = np.random.default_rng(7)
    C, P, S = 1, 8, 2500
    if field == "random":
        sv = rng.uniform(-120, 10, (C, P, S))
    elif field == "spike60":
        sv = np.full((C, P, S), -90.0)
        sv[:, :, ::500] = -30.0                      # 60 dB above the rest of its bin
    elif field == "constant":
        sv = np.full((C, P, S), -63.3)
    else:
        sv = rng.uniform(-330, -300, (C, P, S))     # 10^(Sv/10) near the float32 normal floor
    sv32 = sv.astype(f32)
    lab, nb = fb.labels_index(C, P, S, 4, 500)      # 2000-sample bins
    got = _emulate_mean(sv32, lab, nb, order)
    with np.errstate(divide="ignore"):
        exp = np.array([10 * np.log10(np.mean(10.0 ** (sv32.astype(np.float64).ravel()[lab.ravel() == i] / 10)))
                        for i in range(nb)])
    b = fb.mvbs_bound(sv32.astype(np.float64), lab, nb, exp)
    fb.assert_f32_close(got, exp, b, f"bin mean {field} {order}")
    if field == "constant":  # the known answer
        assert np.all(np.abs(got - float(sv32[0, 0, 0])) <= b)


def test_gamma_is_order_free_and_grows_with_n():
    assert fb.gamma(0) == 0.0
    assert fb.gamma(10**6 - 1) > 1000 * fb.gamma(999)
    assert np.isinf(fb.gamma(2**25))


def _noise_case():
    d, kw = _ek60_case(C=2, P=40, S=400)
    sv, er = ocal.cal_power_ek(d["backscatter_r"], **kw)
    sv = sv.astype(f32).astype(np.float64)       # the float32 values a kernel reads
    er = er.astype(f32).astype(np.float64)
    alpha = d["absorption_indicative"]
    return sv, er, alpha


def test_noise_removal_emulation_within_bound():
    sv, er, alpha = _noise_case()
    C, P, S = sv.shape
    nb = np.array([[-140.0, -138.3], [-141.1, -139.9]])                     # the noise per 20-ping block
    a2 = 2 * np.asarray(alpha, np.float64)[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = 20 * np.log10(np.where(er >= 1, er, 1)) + a2 * er
        sn_exp = nb[:, np.arange(P) // 20][:, :, None] + tl
        # place samples just above the threshold: cancellation
        sv[0, 3, 100:110] = sn_exp[0, 3, 100:110] + 3.0 + np.array([0.1, -0.1, 1e-3, -1e-3, 1e-5, -1e-5, -2.99, -2.99,
                                                                    0.5, 6.0])
        sv = sv.astype(f32).astype(np.float64)
        lin_exp = 10 ** (sv / 10) - 10 ** (sn_exp / 10)
        corr = 10 * np.log10(np.where(lin_exp > 0, lin_exp, np.nan))
        corr_exp = np.where(corr - sn_exp > 3.0, corr, np.nan)
        # emulation (noise_apply.hip:58-63)
        x = er.astype(f32)
        tlf = (f32(20) * np.log10(np.where(x >= 1, x, f32(1))).astype(f32)).astype(f32)
        tlf = (tlf.astype(np.float64) + a2.astype(f32).astype(np.float64) * x).astype(f32)
        snf = (nb[:, np.arange(P) // 20][:, :, None].astype(f32) + tlf).astype(f32)

        def lin(v):
            return (10.0 ** (v.astype(np.float64) * np.float64(f32(0.1))).astype(f32).astype(np.float64)).astype(f32)

        linf = (lin(sv.astype(f32)) - lin(snf)).astype(f32)
        cf = np.where(linf > 0, (f32(10) * np.log10(linf)).astype(f32), np.nan).astype(f32)
        cf = np.where(cf - snf > f32(3.0), cf, np.nan)
    b_sn, b_c = fb.noise_bounds(sv, er, a2, nb, np.zeros_like(nb), 20, sn_exp, lin_exp)
    fb.assert_f32_close(snf, sn_exp, b_sn, "emulated Sv_noise")
    keep_g, keep_e = ~np.isnan(cf), ~np.isnan(corr_exp)
    margin = corr - sn_exp - 3.0
    fb.check_decisions(keep_g, keep_e, margin, b_c + b_sn + fb.U * np.abs(corr - sn_exp))
    both = keep_g & keep_e
    fb.assert_f32_close(np.where(both, cf, np.nan), np.where(both, corr_exp, np.nan), b_c, "emulated Sv_corrected")
    # the condition number shows: 3 dB above the noise costs a factor 2, 0.01 dB (index 106) a factor ~430
    kappa = 10 ** (sv / 10) / lin_exp
    assert kappa[0, 3, 106] > 400 and b_c[0, 3, 106] > 100 * b_c[0, 3, 109]


def test_cw_complex_emulation_within_bound():
    rng = np.random.default_rng(3)
    C, P, S, B = 1, 3, 2000, 4
    re = (rng.standard_normal((C, P, S, B)) * 1e-3).astype(f32)
    im = (rng.standard_normal((C, P, S, B)) * 1e-3).astype(f32)
    re[0, 0, :50] = np.array([1e-2, -1e-2 + 1e-7, 1e-6, 0], f32)            # sectors that nearly cancel
    im[0, 0, :50] = np.array([1e-2, -1e-2, 0, 1e-8], f32)
    pscale, alpha2, A, shift, si, cw, n = 4 / 8 * 1.3, 0.02, 150.0, 0.5, 2e-4, 1500.0, 20.0
    s = np.arange(S, dtype=np.float64)[None, None, :]
    R = (s * si) * (cw / 2)
    Rt = np.where(R - shift > 0, R - shift, np.nan)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    prx = pscale * np.abs(x.mean(-1)) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = 10 * np.log10(prx) + n * np.log10(Rt) + alpha2 * Rt + A
        sr = np.zeros((C, P, S), f32)
        si_ = np.zeros((C, P, S), f32)
        for b in range(B):
            sr = (sr + re[..., b]).astype(f32)
            si_ = (si_ + im[..., b]).astype(f32)
        invn = f32(1) / f32(B)
        mr, mi = (sr * invn).astype(f32), (si_ * invn).astype(f32)
        q = (mr.astype(np.float64) * mr + (mi * mi).astype(f32)).astype(f32)
        pf = (f32(pscale) * q).astype(f32)
        rt = (R.astype(f32) - f32(shift)).astype(f32)
        rt = np.where(rt > 0, rt, np.nan).astype(f32)
        val = (f32(10) * np.log10(pf)).astype(f32) + (f32(n) * np.log10(rt)).astype(f32)
        val = val.astype(f32)
        val = (val + (f32(alpha2) * rt).astype(f32)).astype(f32)
        val = (val + f32(A)).astype(f32)
    val = np.where(np.isnan(Rt), np.nan, val)
    b = fb.cw_complex_bound(re.astype(np.float64), im.astype(np.float64), prx, exp, Rt, R, shift, alpha2,
                            np.full(exp.shape, A), n)
    fb.assert_f32_close(val, exp, b, "emulated CW")
    assert b[0, 0, 10] > 100 * np.nanmedian(b)        # the cancelling sectors carry the condition number


# ---------------------------------------------------------------------------------------------------- sharpness
def _sv_oracle_and_bound(cal_type="Sv"):
    d, kw = _ek60_case(cal_type=cal_type)
    raw = d["backscatter_r"].astype(np.float64)
    exp, _ = ocal.cal_power_ek(raw, **kw)
    terms = ocal.cal_power_ek_terms(raw, **kw)
    return exp, terms, fb.sv_power_bound(terms, exp)


def _assert_sharp(bad, exp, bound):
    # perturbed where |exp| >= 50 dB (the Sv / TS of real data): closer to 0 dB the old bar is 1e-3 dB absolute
    bad = np.where(np.abs(exp) >= 50, bad, exp)
    assert _old_ok(bad, exp), "the perturbation must pass the old 1e-3 bar"
    assert not _new_ok(bad, exp, bound), "the perturbation must fail the derived bound"


def test_sharp_absorption_at_previous_sample():
    exp, terms, b = _sv_oracle_and_bound()
    bad = exp - terms["absorb"] + terms["absorb"] * (terms["Rt"] - terms["k"]) / terms["Rt"]
    _assert_sharp(bad, exp, b)


def test_sharp_range_one_sample_beyond_50m():
    exp, terms, b = _sv_oracle_and_bound()
    Rt, k, n = terms["Rt"], terms["k"], terms["nspread"]
    far = Rt > 50
    with np.errstate(invalid="ignore"):
        moved = exp - terms["spreading"] - terms["absorb"] + n * np.log10(Rt + k) + terms["absorb"] * (Rt + k) / Rt
    _assert_sharp(np.where(far, moved, exp), exp, b)


def test_sharp_constant_offset():
    exp, terms, b = _sv_oracle_and_bound("TS")
    _assert_sharp(exp + 0.01, exp, b)


def test_sharp_linear_power_times_1_plus_1e_3():
    exp, terms, b = _sv_oracle_and_bound()
    _assert_sharp(exp + 10 * np.log10(1 + 1e-3), exp, b)


def test_sharp_bin_drops_one_sample():
    rng = np.random.default_rng(11)
    C, P, S = 1, 1, 400
    sv = (-70 + rng.normal(0, 0.3, (C, P, S))).astype(f32).astype(np.float64)   # non-flat field, 20-sample bins
    lab, nb = fb.labels_index(C, P, S, 1, 20)
    L = 10 ** (sv.ravel() / 10)
    exp = 10 * np.log10(np.bincount(lab.ravel(), L) / np.bincount(lab.ravel()))
    drop = L.reshape(nb, 20)[:, :-1]                                           # the last sample of every bin lost
    bad = 10 * np.log10(drop.mean(1))
    _assert_sharp(bad, exp, fb.mvbs_bound(sv, lab, nb, exp))


def test_sharp_noise_flip_half_a_db_from_threshold():
    rng = np.random.default_rng(2)
    sv, er, alpha = _noise_case()
    exp_n, exp_c = oclean.remove_background_noise(sv, er, alpha, 20, 50, SNR_threshold="3.0dB")
    with np.errstate(invalid="ignore"):
        margin = (10 * np.log10(np.maximum(10 ** (sv / 10) - 10 ** (exp_n / 10), 1e-300))) - exp_n - 3.0
    keep = ~np.isnan(exp_c)
    cand = np.flatnonzero(np.isfinite(margin) & (np.abs(np.abs(margin) - 0.5) < 0.05))
    assert cand.size
    flipped = keep.copy().ravel()
    i = rng.choice(cand)
    flipped[i] = ~flipped[i]
    flipped = flipped.reshape(keep.shape)
    assert (flipped != keep).mean() < 1e-3                                      # the old fraction limit passes
    # the derived bound of the compared quantity corr - Sv_noise, as the GPU tests compute it
    C, P, S = sv.shape
    a2 = 2 * np.asarray(alpha, np.float64)[:, :, None]
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tl = 20 * np.log10(np.where(er >= 1, er, 1)) + a2 * er
        blocks = 10 * np.log10(oclean.coarsen_mean(10 ** ((sv - tl) / 10), 20, 50))
        nb_exp = np.nanmin(blocks, axis=2)
        b_nb = fb.noise_estimate_bound(sv, er, a2, 20, 50, blocks)
        lin_exp = 10 ** (sv / 10) - 10 ** (exp_n / 10)
        b_sn, b_c = fb.noise_bounds(sv, er, a2, nb_exp, b_nb, 20, exp_n, lin_exp)
        corr = 10 * np.log10(np.where(lin_exp > 0, lin_exp, np.nan))
    bound = b_c + b_sn + fb.U * np.abs(corr - exp_n)
    assert np.isfinite(bound.ravel()[i]) and bound.ravel()[i] < 0.5
    fb.check_decisions(keep, keep, margin, bound)                               # no flip: passes
    with pytest.raises(AssertionError, match="outside the bound"):
        fb.check_decisions(flipped, keep, margin, bound)


def test_old_bar_is_implied():
    exp = np.array([-70.0, 0.5, 30.0])
    with pytest.raises(AssertionError, match="old bar"):
        fb.assert_f32_close(exp + np.array([0.0, 0.0, 0.04]), exp, np.array([1.0, 1.0, 1.0]))


def test_power_terms_add_up_to_the_oracle():
    """cal_power_ek_terms returns the terms cal_power_ek adds: their sum is its output (a drift would skew every Sv
    bound)."""
    for cal_type in ("Sv", "TS"):
        d, kw = _ek60_case(cal_type=cal_type)
        raw = d["backscatter_r"].astype(np.float64)
        exp, _ = ocal.cal_power_ek(raw, **kw)
        t = ocal.cal_power_ek_terms(raw, **kw)
        tot = t["raw"] + t["spreading"] + t["absorb"] + t["const"]
        np.testing.assert_array_equal(np.isnan(tot), np.isnan(exp))
        f = np.isfinite(exp)
        assert np.max(np.abs(tot[f] - exp[f])) <= 1e-12
        assert t["nspread"] == (20.0 if cal_type == "Sv" else 40.0)


# ---------------------------------------------------------------------------------------------------- noise masks
def _lin32(v32):
    """exp10f(v * 0.1f) widened to double (csrc/fast_math.h:65): the rounded float64 10^x is within 1/2 ulp."""
    arg = (np.asarray(v32, f32).astype(np.float64) * np.float64(f32(0.1))).astype(f32)
    with np.errstate(over="ignore"):
        return (10.0 ** arg.astype(np.float64)).astype(f32).astype(np.float64)


def _db32(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (10.0 * np.log10(x)).astype(f32)


def _windows(a, n, m):
    """Every interior (2n+1) x (2m+1) window of a (P, S) array, flattened: (P - 2n, S - 2m, W)."""
    w = np.lib.stride_tricks.sliding_window_view(a, (2 * n + 1, 2 * m + 1))
    return w.reshape(w.shape[0], w.shape[1], -1)


def _mask_field(kind, P=30, S=600, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "scene":
        from test_gpu_masks import _scene

        sv = _scene(1, P, S, 7)[0][0]
    elif kind == "spike60":
        sv = -90 + 0.5 * rng.standard_normal((P, S))
        sv[P // 2, S // 2] = -30.0
    elif kind == "near0":
        sv = rng.uniform(-0.01, 0.01, (P, S))
    else:
        sv = rng.uniform(-151, -149, (P, S))
    if kind != "scene":
        sv[rng.random((P, S)) < 0.02] = np.nan
    return sv.astype(f32)


@pytest.mark.parametrize("field", ["scene", "spike60", "near0", "deep"])
@pytest.mark.parametrize("n,m", [(0, 0), (2, 7), (10, 250)])     # windows of 1, 75 and 10 521 values
def test_pooled_mean_emulation_within_bound(field, n, m):
    sv32 = _mask_field(field)
    w64 = _windows(sv32.astype(np.float64), n, m)
    with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        exp = 10 * np.log10(np.nanmean(10.0 ** (w64 / 10), axis=-1))
        lin = _windows(_lin32(sv32), n, m)
        cnt = (~np.isnan(lin)).sum(-1)
        for order in ("forward", "reverse"):       # double sums: the order is below the slack
            ll = lin if order == "forward" else lin[..., ::-1]
            s = np.cumsum(np.where(np.isnan(ll), 0.0, ll), axis=-1)[..., -1]
            got = np.where(cnt > 0, _db32(s / cnt), np.nan)
            b = fb.pooled_mean_bound(sv32, exp)
            err, ratio = fb.assert_f32_close(got, exp, b, f"emulated pooled mean {field} {order}")
            assert ratio <= 1.0 and (ratio > 0 or (n, m) == (0, 0))   # (one value: the round trip may be exact)
    # the decision x - out > thr in float32
    thr = 6.0
    x = sv32[n:sv32.shape[0] - n, m:sv32.shape[1] - m]
    with np.errstate(invalid="ignore"):
        keep = (x - got.astype(f32)).astype(f32) > f32(thr)
        margin = x.astype(np.float64) - exp - thr
    fb.check_decisions(keep, margin > 0, margin, fb.threshold_decision_bound(x, exp, b, thr), f"decisions {field}")


class _Dd:
    """``Dd`` of csrc/noise_masks.hip:952-966, operation by operation in float64."""

    def __init__(self, hi=0.0, lo=0.0):
        self.hi, self.lo = np.float64(hi), np.float64(lo)

    def add(self, x):
        t = self.hi + x
        bb = t - self.hi
        self.lo = self.lo + ((self.hi - (t - bb)) + (x - bb))
        self.hi = t

    def add_dd(self, b, sign):
        bh, bl = sign * b.hi, sign * b.lo
        t = self.hi + bh
        bb = t - self.hi
        e = (self.hi - (t - bb)) + (bh - bb) + self.lo + bl
        hi = t + e
        self.hi, self.lo = hi, e - (hi - t)


def test_running_sum_emulation_within_bound():
    """Per-row double-double running sums and their differences (:943-951): a +60 dB sample early in a row of 3000
    values near -100 dB; every window after it is 10^16 times weaker than the running sums it is the difference of."""
    rng = np.random.default_rng(4)
    S, m = 3000, 6
    sv32 = (-100 + 2 * rng.standard_normal(S)).astype(f32)
    sv32[40] = f32(60.0)
    lin = _lin32(sv32)
    W = []
    acc = _Dd()
    for x in lin:
        acc.add(np.float64(x))
        W.append(_Dd(acc.hi, acc.lo))
    got = np.empty(S - 2 * m, f32)
    for i, s in enumerate(range(m, S - m)):
        d = _Dd(W[s + m].hi, W[s + m].lo)
        if s - m - 1 >= 0:
            d.add_dd(W[s - m - 1], -1.0)
        got[i] = _db32(np.float64((d.hi + d.lo) / (2 * m + 1)))
    exp = 10 * np.log10(_windows((10.0 ** (sv32.astype(np.float64) / 10))[None], 0, m)[0].mean(-1))
    b = fb.pooled_mean_bound(sv32, exp, carried_terms=S, carried_ops=S)
    fb.assert_f32_close(got, exp, b, "emulated running sums")
    assert np.all(b[100:] < 2 * fb.pooled_mean_bound(sv32, exp)[100:])   # the subtraction costs less than the final rounding
    # plain double running sums would not do: the same differences in float64 are off by far more than the bound
    cs = np.concatenate([[0.0], np.cumsum(lin)])
    plain = _db32((cs[2 * m + 1:] - cs[:-(2 * m + 1)]) / (2 * m + 1))
    assert (np.abs(plain.astype(np.float64) - exp)[100:] > b[100:]).mean() > 0.9


@pytest.mark.parametrize("field", ["scene", "spike60", "near0", "deep"])
@pytest.mark.parametrize("n,m", [(0, 0), (2, 7), (1, 12)])        # 1, 75 (odd) values; NaNs make even counts as well
def test_pooled_median_emulation_within_bound(field, n, m):
    sv32 = _mask_field(field, P=12, S=200)
    w32 = _windows(sv32, n, m)
    with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        exp = 10 * np.log10(np.nanmedian(10.0 ** (w32.astype(np.float64) / 10), axis=-1))
        srt = np.sort(w32, axis=-1)                       # NaN last: the keys are the float32 values themselves
        cnt = (~np.isnan(srt)).sum(-1)
        k1, k2 = np.maximum(cnt - 1, 0) // 2, cnt // 2
        a = np.take_along_axis(srt, k1[..., None], -1)[..., 0].astype(np.float64)
        c = np.take_along_axis(srt, np.minimum(k2, srt.shape[-1] - 1)[..., None], -1)[..., 0].astype(np.float64)
        med = np.where(k1 == k2, 10.0 ** (a / 10), (10.0 ** (a / 10) + 10.0 ** (c / 10)) * 0.5)   # the double table
        got = np.where(cnt > 0, _db32(med), np.nan)
    assert (cnt % 2 == 0).any() or (n, m) == (0, 0)
    fb.assert_f32_close(got, exp, fb.pooled_median_bound(exp), f"emulated median {field}")


def test_impulse_and_attenuated_decision_emulation_within_bound():
    rng = np.random.default_rng(6)
    sv32 = _mask_field("scene", P=40, S=200)
    # smoothing: 10-sample bins, forward-filled (range_bin_smooth_kernel), then up[p] - up[p +- n] > thr in float32
    nper, n, thr = 10, 2, 10.0
    lin = _lin32(sv32).reshape(40, 20, nper)
    with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        up32 = np.repeat(_db32(np.nanmean(lin, -1)), nper, axis=1)
        up = np.repeat(10 * np.log10(np.nanmean(10.0 ** (sv32.astype(np.float64).reshape(40, 20, nper) / 10), -1)), nper, 1)
    b_up = fb.pooled_mean_bound(sv32, up)
    fb.assert_f32_close(up32, up, b_up, "emulated smoothing")
    from oracle import masks as omask

    exp = omask.echopy_impulse_noise_mask(up.T, n, thr).T
    fwd = np.full(up32.shape, np.inf, f32)
    bwd = np.full(up32.shape, np.inf, f32)
    with np.errstate(invalid="ignore"):
        fwd[:-n] = up32[:-n] - up32[n:]
        bwd[n:] = up32[n:] - up32[:-n]
    fwd[np.isnan(fwd)] = np.inf
    bwd[np.isnan(bwd)] = np.inf
    got = (fwd > f32(thr)) & (bwd > f32(thr))
    margin, bound = fb.impulse_decision_bound(up, b_up, n, thr)
    fb.check_decisions(got, exp, margin, bound, "emulated impulse mask")
    assert exp.any() and not exp.all()
    # attenuated: two medians cast to float32, one subtraction
    ping = rng.uniform(-90, -60, 5000)
    block = ping + rng.uniform(-8.001, -7.999, 5000)
    athr = 8.0
    got = (ping.astype(f32) - block.astype(f32)).astype(f32) < f32(athr)
    fb.check_decisions(got, ping - block < athr, ping - block - athr, fb.attenuated_decision_bound(ping, block, athr))


# ------------------------------------------------------------------------------------------ noise masks: sharpness
def _pool_case(n=2, m=12, seed=8):
    """A non-flat field (0.3 dB) pooled over 5 x 25 = 125-value windows: (sv32 interior, linear windows, exp, bound)."""
    rng = np.random.default_rng(seed)
    sv32 = (-70 + 0.3 * rng.standard_normal((12, 120))).astype(f32)
    lin = _windows(10.0 ** (sv32.astype(np.float64) / 10), n, m)
    exp = 10 * np.log10(lin.mean(-1))
    return sv32, lin, exp, fb.pooled_mean_bound(sv32, exp)


def test_sharp_pooled_value_times_1_plus_1e_3():
    sv32, lin, exp, b = _pool_case()
    _assert_sharp(exp + 10 * np.log10(1 + 1e-3), exp, b)


def test_sharp_window_loses_or_gains_an_edge_sample():
    sv32, lin, exp, b = _pool_case()
    assert lin.shape[-1] >= 50
    _assert_sharp(10 * np.log10(lin[..., :-1].mean(-1)), exp, b)                      # the last edge sample dropped
    extra = 10.0 ** (np.roll(sv32, -1, axis=1)[2:-2, 12:-12].astype(np.float64) / 10)  # one sample beyond the edge added
    _assert_sharp(10 * np.log10((lin.sum(-1) + extra) / (lin.shape[-1] + 1)), exp, b)


@pytest.mark.parametrize("func", [np.nanmean, np.nanmedian])
def test_sharp_membership_on_the_float64_depth(func):
    """Window edges that fall on samples (0.3 m steps, a 1.5 m bin): d +- bin rounds differently in float32 and float64,
    so the two memberships differ at some outputs -- where they differ by no more than the old bar, only the derived
    bound tells them apart."""
    from oracle import masks as omask

    rng = np.random.default_rng(5)
    C, P, S, n = 1, 7, 160, 1
    sv32 = (-70 + 0.3 * rng.standard_normal((C, P, S))).astype(f32)
    d32 = np.broadcast_to((0.3 * (np.arange(S) + 5)).astype(f32), (C, P, S)).copy()
    sv64 = sv32.astype(np.float64)
    exp = omask.pool_Sv(sv64, d32, func, f32(1.5), n, f32(2.0))
    bad = omask.pool_Sv(sv64, d32.astype(np.float64), func, 1.5, n, 2.0)
    b = fb.pooled_mean_bound(sv32, exp) if func is np.nanmean else fb.pooled_median_bound(exp)
    np.testing.assert_array_equal(np.isnan(bad), np.isnan(exp))
    fin = np.isfinite(exp)
    differ = np.abs(bad - exp)[fin] > b[fin]
    assert differ.mean() >= 0.01, differ.mean()
    with np.errstate(invalid="ignore"):   # (a median may jump by more than the old bar: those the old bar sees too)
        quiet = np.abs(bad - exp) <= fb.OLD_RTOL * np.maximum(np.abs(exp), 1.0)
    bad = np.where(quiet, bad, exp)
    assert (np.abs(bad - exp)[fin] > b[fin]).any()
    assert _old_ok(bad, exp), "0.3 dB of spread keeps these wrong windows inside the old bar"
    assert not _new_ok(bad, exp, b)


def test_sharp_median_takes_the_upper_middle_value():
    rng = np.random.default_rng(9)
    w = np.sort((-70 + 0.3 * rng.standard_normal((500, 50))).astype(f32).astype(np.float64), axis=-1)   # even counts
    exp = 10 * np.log10((10.0 ** (w[:, 24] / 10) + 10.0 ** (w[:, 25] / 10)) / 2)
    np.testing.assert_allclose(exp, 10 * np.log10(np.median(10.0 ** (w / 10), axis=-1)), rtol=0, atol=1e-12)
    _assert_sharp(w[:, 25], exp, fb.pooled_median_bound(exp))


def test_sharp_mask_decision_flipped_1e_3_db_from_its_threshold():
    sv32, lin, exp, b = _pool_case()
    x = sv32[2:-2, 12:-12].astype(np.float64)
    thr = 0.25
    exp = exp.copy()
    exp[3, 40] = x[3, 40] - thr - 1e-3                      # this decision sits 1e-3 dB above its threshold
    margin = x - exp - thr
    keep = margin > 0
    bd = fb.threshold_decision_bound(x, exp, b, thr)
    assert fb.assert_few_near(margin, bd) == 0
    fb.check_decisions(keep, keep, margin, bd)
    flipped = keep.copy()
    flipped[3, 40] = ~flipped[3, 40]
    sure = ~(np.abs(margin) < 2e-3)                         # the old margin leaves this decision out
    np.testing.assert_array_equal(flipped[sure], keep[sure])
    with pytest.raises(AssertionError, match="outside the bound"):
        fb.check_decisions(flipped, keep, margin, bd)
    with pytest.raises(AssertionError, match="within the bound"):
        fb.assert_few_near(np.zeros(10), bd.ravel()[:10])


# ------------------------------------------------------------------------------------------------ EK80 broadband
import bb_ref  # noqa: E402
import splitbeam_ref as sbr  # noqa: E402


def test_bb_constants_are_the_derived_ones():
    """The constants the docstrings state: 157 u for the complex64 tile (77 forward, 3 product, 77 inverse)."""
    c = fb.fft_constants(fb.U)
    assert 77.0 <= c["fwd"] / fb.U < 77.01 and 3.0 <= c["prod"] / fb.U < 3.01 and 157.0 <= c["total"] / fb.U < 157.01
    assert fb.fft_constants(fb.U64)["total"] / fb.U64 < 230


@pytest.mark.parametrize("precision", ["complex64", "complex128"])
def test_bb_tile_bound_passes_an_ordinary_transform(precision):
    """A scipy complex64 (NumPy complex128) transform correlation of the self-test's tiles lies within
    ``fft_tile_bound``: the bound is not unreachable -- and not vacuous: a result off by 1e-4 of the tile fails."""
    u = fb.U if precision == "complex64" else fb.U64
    for name, tiles, h in bb_ref.transform_cases():
        x, exp, bound = bb_ref.transform_expected(tiles, h, u)
        if u == fb.U:
            got = bb_ref.fft32_tiles(x, h)
        else:
            got = np.fft.ifft(np.fft.fft(x, axis=-1) * np.conj(np.fft.fft(h.astype(np.complex128), bb_ref.N)), axis=-1)
        fb.assert_norm_close(got, exp, bound, name)
        with pytest.raises(AssertionError, match="bound"):
            fb.assert_norm_close(got * (1 + 1e-4), exp, bound, name)


def _emulated(kind, *key):
    case = bb_ref.sv_case(kind, *key)
    out = {}
    for form in ("fft", "direct"):
        y = bb_ref.emulate_y(case["o"], form, case["inputs"][3][0])
        out[form] = (y, *bb_ref.epilogue32(case["o"], y, form))
    return case, out


@pytest.mark.parametrize("kind,key", [("flat", ()), ("path", (177, 5000, True, 4)), ("path", (31, 300, True, 2)),
                                      ("path", (40, 1000, False, 1)), ("zeros", (177,)), ("zeros", (16,))])
def test_bb_sample_bound_passes_a_float32_emulation(kind, key):
    """Either form emulated in NumPy float32 (the direct form's fma chains; an ordinary complex64 transform, the sector
    sums, the per-sector route and the epilogue in the kernels' order) passes the judge of the GPU tests: amplitude of
    the summed sectors, linear amplitude of every sample, the dB values, the exact footprint."""
    case, em = _emulated(kind, *key)
    o = case["o"]
    for form in ("fft", "direct"):
        y, out, prx = em[form]
        assert np.all(np.abs(y - o["y"]) <= case[form][0])
        r = bb_ref.judge_sv(out, prx, case, form, f"{kind} {form}")
        assert r["judged_db"] > 0.5
        bb_ref.check_footprint(case, prx, form)


def test_bb_inputs_meet_their_conditions():
    """Conditions on the inputs, checked on the oracle alone: the flat case gives every finite sample a finite dB bound
    in both forms; at most 1 % of the zero cases' footprint lies under the amplitude bound and thousands of samples lie
    outside the footprint; most samples of the 140 dB cases are judged in dB."""
    case = bb_ref.sv_case("flat")
    fin = np.isfinite(case["o"]["exp"])
    assert fin.mean() > 0.9 and all(np.isfinite(case[f][1][fin]).all() for f in ("fft", "direct"))
    for taps in (177, 16):
        z = bb_ref.sv_case("zeros", taps)
        has, sure = bb_ref.footprint(z)
        assert sure.sum() >= 0.99 * has.sum() and (~has & (z["o"]["nvalid"] > 0)).sum() > 1000
    p = bb_ref.sv_case("path", 177, 5000, True, 4)
    fin = np.isfinite(p["o"]["exp"])
    assert all(np.isfinite(p[f][1][fin]).mean() > 0.5 for f in ("fft", "direct"))


@pytest.mark.parametrize("how,q", [("twiddle", 1), ("twiddle", 3), ("swap", 2)])
def test_bb_sharp_one_disturbed_butterfly_element(how, q):
    """One element of one pass with the twiddle power of the neighbouring table index, or with its real and imaginary
    halves exchanged, in an otherwise exact transform of a white tile and of a tone: outside ``fft_tile_bound``."""
    name, tiles, h = [c for c in bb_ref.transform_cases() if c[0].startswith("white")][2]
    tone = [c for c in bb_ref.transform_cases() if c[0] == "tones"][0][1][q:q + 1]
    for xt in (tiles[:1], tone):
        x, exp, bound = bb_ref.transform_expected(xt, h, fb.U)
        good = bb_ref.fft32_tiles(x, h)
        fb.assert_norm_close(good, exp, bound, name)
        bad = (good[0] + bb_ref.pass0_perturbed(x[0], h, 300, q, how)).astype(np.complex64)[None]
        with pytest.raises(AssertionError, match="bound"):
            fb.assert_norm_close(bad, exp, bound, name)


def test_bb_sharp_output_from_the_circular_wrap():
    """The first sample of the second tile taken from the first tile's transform (its wrapped output N - taps + 1):
    outside the bound in linear amplitude and in dB."""
    case, em = _emulated("flat")
    o = case["o"]
    taps = case["inputs"][3][0]
    opt = bb_ref.N - taps + 1
    y = em["fft"][0].copy()
    xs = o["xz"][0, 0].sum(-1)
    y[0, 0, opt] = bb_ref.circ_correlate(xs[None, :bb_ref.N], o["reps"][0])[0, opt]
    out, prx = bb_ref.epilogue32(o, y, "fft")
    with pytest.raises(AssertionError, match="amplitude off"):
        bb_ref.judge_sv(out, prx, case, "fft", "wrap")


def test_bb_sharp_footprint_edge_sample_zeroed():
    """The zero restoration reaching one sample too far: the first sample of a footprint set to an exact 0 (prx NaN)
    fails the footprint check and the linear judgement."""
    case, em = _emulated("zeros", 177)
    has, sure = bb_ref.footprint(case)
    edge = np.argwhere(sure[0, 0, 1:] & ~has[0, 0, :-1])[0, 0] + 1
    for form in ("fft", "direct"):
        y, out, prx = em[form]
        out, prx = out.copy(), prx.copy()
        out[0, 0, edge], prx[0, 0, edge] = np.nan, np.nan
        with pytest.raises(AssertionError, match="footprint|NaN pattern"):
            bb_ref.check_footprint(case, prx, form)
        with pytest.raises(AssertionError, match="amplitude off"):
            bb_ref.judge_sv(out, prx, case, form, "edge")
        grown = em[form][2].copy()                 # ... and one sample too few: a number outside the footprint
        grown[0, 0, edge - 1] = 1e-20
        with pytest.raises(AssertionError):
            bb_ref.check_footprint(case, grown, form)


def _sba_golden(tag):
    import os

    g = sbr.load_goldens(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", sbr.GOLDEN))
    prm = [g[f"{tag}_{k}"] for k in ("sens_al", "sens_at", "off_al", "off_at")]
    re, im, bt = g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"]
    reps = [g[f"{tag}_replica0_{c}"] for c in range(re.shape[0])]
    return re, im, bt, prm, reps


def test_bb_sharp_two_sectors_exchanged_before_the_splitbeam_combination():
    """The split-beam broadband judge with the DERIVED bound alone (no cap): the oracle's own angles rounded to float32
    pass the electrical-angle bound of a float32 output, the angles of the same samples with sectors 0 and 1 exchanged
    do not -- for the complex64 transform's bound (the widest) as for the complex128 one."""
    re, im, bt, prm, reps = _sba_golden("pc_fft")
    sw = [1, 0, 2, 3]
    th2, ph2, _, _ = sbr.complex_angles(re[..., sw], im[..., sw], bt, *prm,
                                        [np.asarray(r).astype(np.complex64) for r in reps])
    for u_f in (fb.U, fb.U64):
        th, ph, b_al, b_at, weak = sbr.complex_angle_bounds(re, im, bt, *prm, reps, form="fft", u_f=u_f, u_t=fb.U)
        ok = ~np.isnan(th) & ~weak
        assert np.isfinite(b_al[ok]).all() and np.isfinite(b_at[ok]).all()
        sbr.assert_complex_bound(th.astype(f32), th, prm[0], prm[2], weak, b_al, np.inf)
        sbr.assert_complex_bound(ph.astype(f32), ph, prm[1], prm[3], weak, b_at, np.inf)
        # (type 1: fore = 2 + 3 and aft = 0 + 1 do not see the exchange, starboard = 0 + 3 and port = 1 + 2 do)
        sbr.assert_complex_bound(th2, th, prm[0], prm[2], weak, b_al, np.inf)
        with pytest.raises(AssertionError, match="electrical angle differs"):
            sbr.assert_complex_bound(ph2, ph, prm[1], prm[3], weak, b_at, np.inf)


def test_bb_splitbeam_bound_governs_where_stated():
    """Where the derived angle bound, and where the 0.05 deg cap beside it, judges the split-beam goldens -- a property
    of the inputs, stated in README / DESIGN and kept visible here.  A complex128 transform under a float32 output and
    the float64 direct form: the derived bound is the smaller one at EVERY compared sample.  The float32 direct form:
    at more than nine in ten.  The complex64 transform: the tile's normwise bound, taken per sample, exceeds the cap
    at most samples (it governs the strongest 3 - 15 % only); there the cap is what judges."""
    shares = {}
    for tag in ("pc_fft", "pc_short"):
        re, im, bt, prm, reps = _sba_golden(tag)
        for name, form, u_f, u_t in (("c64", "fft", fb.U, fb.U64), ("c128->f32", "fft", fb.U64, fb.U),
                                     ("direct f32", "direct", fb.U, fb.U), ("direct f64", "direct", fb.U64, fb.U64)):
            th, ph, b_al, b_at, weak = sbr.complex_angle_bounds(re, im, bt, *prm, reps, form=form, u_f=u_f, u_t=u_t)
            ok = ~np.isnan(th) & ~weak
            shares[tag, name] = min(float((b_al[ok] <= 0.05).mean()), float((b_at[ok] <= 0.05).mean()))
    for tag in ("pc_fft", "pc_short"):
        assert shares[tag, "c128->f32"] == 1.0 and shares[tag, "direct f64"] == 1.0
        assert shares[tag, "direct f32"] > 0.9
        assert 0.0 < shares[tag, "c64"] < 0.5


def test_bb_tolerance_most_samples_judged_on_the_synthetic_files():
    """``assert_bb_close(..., most=True)`` of test_gpu_api.py / test_gpu_fuzz.py: the oracle alone judges most float32
    samples of every synthetic broadband file those tests build (the condition their callers enforce on the GPU)."""
    import echopype_amd as ep
    import oracle_chain as oc
    from bb_tolerance import judged_fraction
    from test_gpu_api import _ek80

    cases = [dict(C=2, P=12, S=1200, mixed_nan=m) for m in (False, True)]
    cals = ["Sv", "Sv"]
    for seed in range(12):                       # test_random_ek80_complex's draws
        rng = np.random.default_rng(9000 + seed)
        P, S = int(rng.choice([1, 3, 6])), int(rng.choice([300, 1200, 1872, 1873, 2500, 4100]))
        rng.choice(["float64", "float32"])
        mixed = bool(rng.integers(0, 2))
        if seed % 3:
            cases.append(dict(C=2, P=P, S=S, mixed_nan=mixed, seed=seed))
            cals.append(str(rng.choice(["Sv", "TS"])))
    assert len(cases) == 10
    for kw, cal in zip(cases, cals):
        d, filt = _ek80(ep, "BB", **kw)
        (exp, _, prx), _ = oc.ek80_complex(d, filt, cal)
        assert judged_fraction(exp, "float32", prx) > 0.5, kw
