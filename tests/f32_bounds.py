"""How float32 kernel outputs are judged against the float64 oracle: per-element ABSOLUTE dB bounds derived a priori
from each kernel's operation sequence (pure NumPy, no GPU).

The oracle runs on exactly the float32 values the kernel read (upcast to float64), so input rounding is never charged
to a kernel.  u = 2^-24 (float32 unit roundoff); every elementary float operation returns op(x)(1 + d), |d| <= u, and a
fused multiply-add rounds once.  ocml's ``log10f`` / ``exp10f`` are taken at E_LOG / E_EXP ulp of their result (the
accuracy HIP documents for the single-precision functions); ulp(y) <= 2u|y| for a normal y.  Each bound ends with the
oracle's own float64 evaluation (a few 2^-53 of the terms it adds), which is negligible but kept so that a bound is a
bound.  Nothing here is fitted to measured errors.

Quantities (kernel lines cited where each bound is derived):

* ``sv_power_bound``    per-sample Sv / TS from power samples (``cal_power_sample<float>``, csrc/sample_math.h;
                         the fused, block-reduce, int16 and chain kernels call the same function).
* ``cw_complex_bound``  EK80 CW complex Sv / TS (``sv_complex_cw_kernel``, csrc/ek80_complex.hip).
* ``mean_db_bound``     a bin mean in dB: MVBS (fused ``lin_bins``, ``block_reduce`` ``lin_from_db``, finalize
                         ``10*log10(s/n)``), NASC-style sums, the noise estimate's block means.
* ``tl_bound`` / ``noise_bounds``  Sv_noise and Sv_corrected (csrc/noise_apply.hip, the SRC_SV_DENOISE branch of
                         csrc/block_reduce.hip), with the condition number of the subtraction.
* ``pooled_mean_bound`` / ``pooled_median_bound``  the pooled and smoothed Sv of the noise masks (csrc/noise_masks.hip:
                         float32 ``exp10f`` terms, double sums, one final rounding; medians double throughout), and
                         ``threshold_`` / ``impulse_`` / ``attenuated_decision_bound`` for the comparisons made on them.
* ``check_decisions``   a keep/remove or membership decision may differ only where the oracle's margin to the
                         threshold is within the bound of the quantity compared.
* ``fft_tile_bound`` / ``direct_form_bound`` / ``bb_sample_bound`` / ``splitbeam_angle_bound``  the EK80 broadband
                         routes: a normwise bound of one tile of the LDS transform's correlation (csrc/lds_fft.h, pass
                         by pass), the per-sample bound of the direct form's fma chains, from either amplitude bound to
                         Sv / TS in dB and to linear amplitude, and to the split-beam electrical angles.

``assert_f32_close`` also asserts the old north-star bar (|got - exp| / max(|exp|, 1) <= 1e-3), so a passing check
implies the old one at every element.
"""
import json
import os

import numpy as np

U = 2.0**-24                      # float32 unit roundoff
U64 = 2.0**-53                    # float64 unit roundoff (the oracle's own arithmetic)
E_LOG = 2.0                       # log10f: ulp of its result
E_EXP = 2.0                       # exp10f: ulp of its result
TINY = 2.0**-149                  # float32 subnormal spacing: exp10f's absolute error floor below 2^-126
LN10 = np.log(10.0)
DB = 10.0 / LN10                  # d(10 log10 x) / (dx / x)
D01 = abs(float(np.float32(0.1)) - 0.1) / 0.1   # relative error of the constant 0.1f (0.25 u)
OLD_RTOL = 1e-3                   # the north-star bar every float32 check still asserts


def gamma(m):
    """gamma_m = m u / (1 - m u): relative error of a sum of m+1 same-sign float terms, in ANY order."""
    m = np.asarray(m, np.float64)
    return np.where(m * U < 1.0, m * U / np.maximum(1.0 - m * U, 1e-300), np.inf)


def half_ulp(x):
    """1/2 ulp of float32(x): the rounding of a float32 result."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64) / 2.0


def db_of_rel(r):
    """|10 log10(1 + e)| <= DB * -ln(1 - r) for |e| <= r (inf for r >= 1)."""
    r = np.asarray(r, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r < 1.0, -DB * np.log1p(-np.minimum(r, 1.0 - 1e-16)), np.inf)


def rel_of_db(b):
    """A dB error <= b as a relative error of the linear value: 10^(b/10) - 1."""
    return np.expm1(np.asarray(b, np.float64) / DB)


def exp10_rel(sv_abs):
    """Relative error of the float32 ``exp10f(v * 0.1f)`` (csrc/fast_math.h:65,87; fused_sv_mvbs.hip:111) for an
    argument |v| <= sv_abs: 0.1f carries D01, the product rounds once (u), so the argument is off by
    |v|/10 (D01 + u + D01 u), a relative error ln10 times that in the result; exp10f adds E_EXP ulp <= 2 E_EXP u.
    (Below 2^-126 the result is subnormal: see ``mean_db_bound``'s absolute term.)"""
    a = np.asarray(sv_abs, np.float64) / 10.0 * (D01 + U + D01 * U)
    return np.expm1(LN10 * a) * (1.0 + 2 * E_EXP * U) + 2 * E_EXP * U


# ------------------------------------------------------------------------------------------------ per-sample Sv
def sv_power_bound(terms, exp):
    """Absolute dB bound of one float32 power sample's Sv / TS against the float64 oracle.

    ``cal_power_sample<float>`` (csrc/sample_math.h:62-75) with the row constants of ``RowK<float>`` (:16-20):
        out = fma(g, raw, nL) + fma(alpha2, rt, A0),     nL = nspread * log10f((float)(s - d))  (ColumnLog, :38)
    T1 = g*raw, T2 = nspread*log10(s - d) = spreading - nspread*log10(k), T3 = alpha2*R', T4 = A0 = const +
    nspread*log10(k) (power_coef.hip: A0 = A + n log10 k in double, then rounded to float).  Roundings:
      T1: float(g) (u), the first fma (u)                                           -> 2 u |T1|
      T2: (float)(s - d) (relative u -> |n| u / ln10 absolute), log10f (2 E_LOG u |T2|), * nspread (u),
          the first fma (u)                                                         -> (2 E_LOG + 2) u |T2| + |n| u/ln10
      T3: float(alpha2) (u), float(R') (u), the second fma (u)                     -> 3 u |T3|
      T4: float(A0) (u), the second fma (u)                                         -> 2 u |T4|
      the final add: 1/2 ulp of the float32 result.
    ``terms`` = ``oracle.calibrate.cal_power_ek_terms(...)`` on the float32 samples the kernel read."""
    n = terms["nspread"]
    with np.errstate(invalid="ignore", divide="ignore"):
        nlogk = n * np.log10(terms["k"])
        T1 = np.abs(terms["raw"])
        T2 = np.abs(terms["spreading"] - nlogk)
        T3 = np.abs(terms["absorb"])
        T4 = np.abs(terms["const"] + nlogk)
    tot = T1 + T2 + T3 + T4
    b = U * (2 * T1 + (2 * E_LOG + 2) * T2 + 3 * T3 + 2 * T4) + abs(n) * U / LN10
    return b * (1 + 8 * U) + half_ulp(exp) + 8 * U64 * (tot + np.abs(terms["spreading"]) + np.abs(nlogk))


def cw_complex_bound(re, im, prx, exp, Rt, R, shift, alpha2, const, nspread):
    """Absolute dB bound of ``sv_complex_cw_kernel`` (csrc/ek80_complex.hip:352-391), float32 arithmetic:
      (T)x_b (u, float64 planes only), sr = sum_b x_b (float, any order: gamma_{B-1} sum|x_b|), mr = sr * fl(1/n)
          (2 u)   -> |dm| <= D = ((1 + gamma_{B-1})(1 + u)^3 - 1) sum|x_b| / n
      q = mr*mr + mi*mi (2 roundings), prx = fl(pscale) * q (2 roundings)
          -> relative error of the received power (1 + (2|m_r| D_r + D_r^2 + 2|m_i| D_i + D_i^2) / |m|^2)(1+u)^4 - 1:
             the sector mean's cancellation makes it large where |mean| << mean|x_b| (the condition number of |.|^2)
      10*log10(prx): DB * -ln(1 - e_p), log10f (2 E_LOG u |log10 prx| * 10), * 10 (u)
      rt = fl(fl(R) - fl(shift)): |drt| <= u (R + shift + rt) -> n * log10: |n| drt/rt / ln10 / (1 - drt/rt),
          log10f (2 E_LOG u), * nspread (u);  alpha2 * rt: fl(alpha2) (u), drt, the product (u);  fl(A) (u)
      the three adds: 3 u sum|term|.
    re, im (C, P, S, B) float64 copies of the float32 planes; prx, exp, Rt, R (C, P, S); shift, alpha2, const broadcast
    to (C, P, S)."""
    ok = ~(np.isnan(re) | np.isnan(im))
    nv = ok.sum(-1).astype(np.float64)
    B = re.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        sabs_r = np.where(ok, np.abs(re), 0.0).sum(-1) / nv
        sabs_i = np.where(ok, np.abs(im), 0.0).sum(-1) / nv
        mr = np.where(ok, re, 0.0).sum(-1) / nv
        mi = np.where(ok, im, 0.0).sum(-1) / nv
        f = (1 + gamma(B - 1)) * (1 + U) ** 3 - 1
        Dr, Di = f * sabs_r, f * sabs_i
        q = mr * mr + mi * mi
        eq = (2 * np.abs(mr) * Dr + Dr * Dr + 2 * np.abs(mi) * Di + Di * Di) / q
        ep = (1 + eq) * (1 + U) ** 4 - 1
        Tp = np.abs(10 * np.log10(prx))
        b_p = db_of_rel(ep) + (2 * E_LOG + 1) * U * Tp
        drt = U * (np.abs(R) + np.abs(shift) + np.abs(Rt))
        rel_rt = drt / Rt
        Ts = np.abs(nspread * np.log10(Rt))
        b_s = abs(nspread) / LN10 * rel_rt / (1 - rel_rt) + (2 * E_LOG + 1) * U * Ts
        Ta = np.abs(alpha2 * Rt)
        b_a = 2 * U * Ta + np.abs(alpha2) * drt
        Tc = np.abs(const)
        tot = Tp + Ts + Ta + Tc
        b = b_p + b_s + b_a + U * Tc + 3 * U * tot
    return b * (1 + 8 * U) + 8 * U64 * tot


# ------------------------------------------------------------------------------------------------ bin means
def bin_stats(labels, nbins, sv, b_sv=0.0):
    """Per-bin statistics of the members for ``mean_db_bound``: n, the exact linear mean and the L-weighted mean of
    each member's relative error bound rho_i = (1 + exp10_rel(|Sv_i| + b_i)) 10^(b_i/10) - 1 (the float Sv is off by
    at most b_i dB before ``exp10f``).  ``labels`` >= 0: bin of each sample, -1: not aggregated; NaN Sv is skipped."""
    sv = np.asarray(sv, np.float64).ravel()
    lab = np.asarray(labels).ravel()
    b = np.broadcast_to(np.asarray(b_sv, np.float64), np.shape(sv)).ravel() if np.ndim(b_sv) == 0 else \
        np.asarray(b_sv, np.float64).ravel()
    use = (lab >= 0) & ~np.isnan(sv)
    L = 10.0 ** (sv[use] / 10.0)
    rho = (1 + exp10_rel(np.abs(sv[use]) + b[use])) * (1 + rel_of_db(b[use])) - 1
    n = np.bincount(lab[use], minlength=nbins).astype(np.float64)
    sL = np.bincount(lab[use], weights=L, minlength=nbins)
    sLr = np.bincount(lab[use], weights=L * rho, minlength=nbins)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n, sL / n, sLr / sL


def mean_db_bound(n, mean_lin, rho_bar, exp):
    """Absolute dB bound of a float32 bin mean 10*log10((sum_i lin_i) / n) (fused_sv_mvbs.hip:166,240,541;
    block_reduce.hip lin_from_db + mvbs_finalize_kernel; noise_rowmin_kernel:452):
      each term is off by rho_i relative (``bin_stats``) plus E_EXP * 2^-149 absolute where exp10f is subnormal;
      the n positive terms are summed in float in ANY order (lane accumulators, LDS and global atomics): relative
      gamma_{n-1}, whatever the order; s / n (u); log10f (E_LOG ulp = 2 E_LOG u |MVBS| / 10 after * 10); * 10 (u).
      -> DB * -ln(1 - R) + (2 E_LOG + 1) u |MVBS|,  1 + R = (1 + rho_bar + n E_EXP 2^-149 / sum)(1 + gamma_{n-1})(1 + u)
    ``exp`` = the oracle's bin mean in dB (the order-free bound does not depend on which kernel summed)."""
    n = np.asarray(n, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        R = (1 + rho_bar + E_EXP * TINY / mean_lin) * (1 + gamma(np.maximum(n - 1, 0))) * (1 + U) - 1
        b1 = db_of_rel(R)
        return (b1 + (2 * E_LOG + 1) * U * (np.abs(exp) + b1)) * (1 + 8 * U) + 8 * U64 * np.abs(exp)


def nasc_rel_bound(n, rho_bar):
    """Relative bound of a float32 NASC cell (csrc/nasc.hip): the linear terms are float32 ``exp10f`` values (rho_bar,
    ``bin_stats``) summed in DOUBLE (gamma_{n-1} at 2^-53); each height is the float32 difference of two float32 depths
    (u) summed in double; sv_mean * h_mean * 4 pi 1852^2 in double, then the float32 output (u).
    -> (1 + rho_bar)(1 + gamma64_{n-1})(1 + u)^2 (1 + 8 * 2^-53) - 1."""
    n = np.asarray(n, np.float64)
    g64 = np.maximum(n - 1, 0) * U64 / (1 - np.maximum(n - 1, 0) * U64)
    return (1 + rho_bar) * (1 + g64) * (1 + U) ** 2 * (1 + 8 * U64) - 1


def labels_range(range_var, ping_time, t_edges, r_edges, closed="left"):
    """Bin of every sample of a (C, P, S) range variable under compute_MVBS's binning (oracle.commongrid.bin_index):
    (C, P, S) labels over C * nt * nr bins (channel-major)."""
    from oracle import commongrid as ogrid

    C = range_var.shape[0]
    nt, nr = len(t_edges) - 1, len(r_edges) - 1
    it = ogrid.bin_index(ping_time, t_edges, closed)[None, :, None]
    ir = ogrid.bin_index(range_var, r_edges, closed)
    c = np.arange(C)[:, None, None]
    return np.where((it >= 0) & (ir >= 0), (c * nt + it) * nr + ir, -1), C * nt * nr


def labels_index(C, P, S, ping_num, rsn):
    """Bin of every sample under index binning (coarsen ping_num x range_sample_num, padded tails)."""
    Pb, Sb = -(-P // ping_num), -(-S // rsn)
    c = np.arange(C)[:, None, None]
    p = (np.arange(P) // ping_num)[None, :, None]
    s = (np.arange(S) // rsn)[None, None, :]
    return (c * Pb + p) * Sb + s, C * Pb * Sb


def mvbs_bound(sv, labels, nbins, exp_mvbs, b_sv=0.0):
    """``mean_db_bound`` of every bin, reshaped as ``exp_mvbs``."""
    n, m, r = bin_stats(labels, nbins, sv, b_sv)
    return mean_db_bound(n, m, r, np.asarray(exp_mvbs, np.float64).ravel()).reshape(np.shape(exp_mvbs))


# ------------------------------------------------------------------------------------------------ noise removal
def _a2(a2, C, P):
    """2 * alpha as (C, P, 1) from a scalar, (C,) or (C, P)."""
    a2 = np.asarray(a2, np.float64)
    if a2.ndim == 1:
        a2 = a2[:, None]
    if a2.ndim <= 2:
        a2 = np.broadcast_to(a2, (C, P))[:, :, None]
    return a2


def tl_bound(x, a2):
    """Transmission loss in float32, 20*log10f(max(x, 1)) + alpha2*x (noise_apply.hip:59, block_reduce.hip:258,289):
    log10f (2 E_LOG u), * 20 (u); float(alpha2) (u), the product (u); the add (u).  ``x`` = the float32 range read."""
    with np.errstate(invalid="ignore", divide="ignore"):
        Ts = np.abs(20 * np.log10(np.where(x >= 1, x, 1.0)))
        Ta = np.abs(a2 * x)
    return (2 * E_LOG + 1) * U * Ts + 2 * U * Ta + U * (Ts + Ta) + 8 * U64 * (Ts + Ta)


def noise_estimate_bound(sv, x, a2, ping_num, rsn, exp_blocks):
    """Bound of the per-(channel, ping block) noise ``epa_noise_estimate`` returns (block_reduce.hip OP_NOISE:
    v = exp10f((Sv - tl) * 0.1f), block sums, ``noise_rowmin_kernel``), before the noise_max clamp.
    The argument Sv - tl is off by tl_bound + u |Sv - tl|; each block mean follows ``mean_db_bound``; the minimum over
    range blocks (and the clamp) is 1-Lipschitz in the max norm -> the largest bound over the row's finite blocks.
    ``exp_blocks`` (C, Pb, Sb) = the oracle's 10 log10 of the block means."""
    C, P, S = sv.shape
    a2 = _a2(a2, C, P)
    with np.errstate(invalid="ignore", divide="ignore"):
        tl = 20 * np.log10(np.where(x >= 1, x, 1.0)) + a2 * x
        arg = sv - tl
    b_arg = tl_bound(x, a2) + U * np.abs(arg)
    lab, nb = labels_index(C, P, S, ping_num, rsn)
    per = mvbs_bound(arg, lab, nb, exp_blocks, b_arg)
    per = np.where(np.isfinite(exp_blocks), per, -np.inf)
    return np.max(per, axis=2)


def noise_bounds(sv, x, a2, nb_exp, b_nb, ping_num, sn_exp, corr_lin_exp):
    """Bounds of the float32 Sv_noise and Sv_corrected of ``noise_apply_kernel`` (noise_apply.hip:58-63):
      sn = fl(float(noise) + tl):          b_nb + u |nb| + tl_bound + u |sn|
      lin = exp10f(v 0.1f) - exp10f(sn 0.1f), rounded (u); v is the float Sv read (exact for the oracle)
          relative error of lin: (Ls eta_s + Ln rho_n) / (Ls - Ln) + u -- the condition number Ls / (Ls - Ln)
      corr = 10 log10f(lin): DB * -ln(1 - e) + (2 E_LOG + 1) u |corr|
    nb_exp (C, Pb) the oracle's noise per ping block, b_nb its bound; sn_exp, corr_lin_exp (= 10^(Sv/10) -
    10^(Sv_noise/10), the oracle's linear difference) (C, P, S).  Returns (b_sn, b_corr)."""
    C, P, S = sv.shape
    a2 = _a2(a2, C, P)
    blk = np.arange(P) // ping_num
    nbp = nb_exp[:, blk][:, :, None]
    bnb = b_nb[:, blk][:, :, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b_sn = (bnb + U * np.abs(nbp) + tl_bound(x, a2) + U * np.abs(sn_exp)) * (1 + 8 * U)
        Ls, Ln = 10.0 ** (sv / 10.0), 10.0 ** (sn_exp / 10.0)
        rho_n = (1 + exp10_rel(np.abs(sn_exp) + b_sn)) * (1 + rel_of_db(b_sn)) - 1
        e = (Ls * exp10_rel(np.abs(sv)) + Ln * rho_n + 2 * E_EXP * TINY) / np.abs(corr_lin_exp) + U
        corr = 10 * np.log10(np.where(corr_lin_exp > 0, corr_lin_exp, np.nan))
        b1 = db_of_rel(e)
        b_corr = (b1 + (2 * E_LOG + 1) * U * (np.abs(corr) + b1)) * (1 + 8 * U) + 8 * U64 * (np.abs(corr) + np.abs(sv))
    return b_sn, b_corr


# ------------------------------------------------------------------------------------------------ noise masks
# csrc/noise_masks.hip: float32 Sv, linear terms ``exp10f(v * 0.1f)`` (fast_math.h:65) widened to double at once, every
# sum, mean and median in double (header, :12-13), the result ``(T)(10 * fast_log10(double))``; window membership, the
# feasibility tests and every comparison against a threshold in float32 on the float32 values (``bound<T,..>``,
# ``pool_feasible``, :866-901) -- the oracle is called on the float32 range array, so membership is never an error term.
DD = 2.0**-102                    # one double-double addition (``Dd::add``, :952-966): a few 2^-106 of its result
SUM64 = 2.0**-28                  # gamma of a double sum of up to 2^24 same-sign terms (2^24 * 2^-53 / (1 - ...))


def f64_db_slack(exp):
    """What the double part of a mask kernel and the oracle's own float64 evaluation may differ by, in dB: a double sum
    of same-sign terms (SUM64, any order), a division, the double ``lin_from_db`` / ``fast_log10`` (4e-16 relative,
    fast_math.h:6) and the multiplication by 10 on both sides."""
    with np.errstate(invalid="ignore"):
        return DB * 2 * SUM64 + 16 * U64 * np.abs(np.asarray(exp, np.float64))


def sv_abs_max(sv):
    """Largest finite |Sv| of the field (the argument ``exp10_rel`` is evaluated at)."""
    a = np.abs(np.asarray(sv, np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def lin_max(sv):
    """Largest finite linear value of the field: no window or running sum of n terms exceeds n times it."""
    v = np.asarray(sv, np.float64)
    v = v[np.isfinite(v)]
    return float(10.0 ** (v.max() / 10.0)) if v.size else 0.0


def pooled_mean_bound(sv, exp, carried_terms=0, carried_ops=0):
    """Absolute dB bound of a pooled / smoothed float32 mean with double sums: ``range_bin_smooth_kernel`` (:123,134,140),
    ``box_range_kernel`` / ``box_range_scan_kernel`` (:208,311) + ``box_ping_slide_kernel``, ``pool_value_mean_kernel``
    (:931,936) and the ``row_*`` / ``value_slide*`` / staged / lean routes, which add the same terms in another order.
      each term exp10f(v * 0.1f): relative ``exp10_rel(|v|)`` <= exp10_rel(max |Sv|); the terms are positive, so their
          sum and mean inherit at most the largest relative error of a member (a weighted mean of the members' errors,
          as ``bin_stats`` weighs them), plus E_EXP * 2^-149 per term where exp10f is subnormal (``mean_db_bound``)
      the sum, the division and the logarithm in double: ``f64_db_slack``
      (T)(10 log10 mean): 1/2 ulp of the float32 result.
    The routes that SUBTRACT -- per-row double-double running sums W[hi-1] - W[lo-1] (``row_running_sum_kernel`` +
    ``row_interval_sum_kernel``, :943-951) and the window sums carried down the columns (enter / leave:
    ``box_ping_slide_kernel``, ``value_slide*``) -- hold sums of up to ``carried_terms`` values to DD each over
    ``carried_ops`` additions: an ABSOLUTE error carried_ops * DD * carried_terms * max lin, i.e. relative to the window
    sum (>= its mean, one value at least) carried_ops * DD * carried_terms * max lin / mean.  For the inputs used here
    (a +60 dB sample over a background whose windows average -100 dB or more, rows of up to 8200 values) that is at
    most 8200 * 2e-31 * 8200 * 10^6 / 10^-10 = 1.3e-7 relative (6e-7 dB, a sixth of the final rounding at -70 dB) in the
    weakest window of such a row, and below 1e-15 wherever the field has no such spike.
    ``sv`` = the float32 field (any shape); ``exp`` = the oracle's pooled value in dB."""
    exp = np.asarray(exp, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean_lin = 10.0 ** (exp / 10.0)
        carried = float(carried_ops) * DD * float(carried_terms) * lin_max(sv) / mean_lin if carried_ops else 0.0
        R = (1 + exp10_rel(sv_abs_max(sv)) + E_EXP * TINY / mean_lin) * (1 + carried) - 1
        b1 = db_of_rel(R)
        return b1 * (1 + 8 * U) + half_ulp(np.abs(exp) + b1) + f64_db_slack(exp)


def pooled_median_bound(exp):
    """Absolute dB bound of a float32 median route (``pool_median*``, ``pool_value_median*``, ``attenuated_*``): the keys
    are the float32 values themselves, the two middle ones go through the DOUBLE table (select.h:286-291), their mean
    and logarithm are double -> ``f64_db_slack`` + 1/2 ulp of the float32 result."""
    exp = np.asarray(exp, np.float64)
    s = f64_db_slack(exp)
    return half_ulp(np.abs(exp) + s) + s


def sub_rounding(diff, b):
    """Rounding of one float32 subtraction whose exact result is within ``b`` of ``diff``."""
    with np.errstate(invalid="ignore"):
        return half_ulp(np.abs(np.asarray(diff, np.float64)) + b)


def threshold_decision_bound(x, out_exp, b_out, thr):
    """``x - out > thr`` in float32 (:939 and every pooling route's epilogue): the bound of ``out``, the rounding of the
    subtraction and the rounding of ``thr`` to float32.  ``x`` = the float32 Sv, ``out_exp`` = the oracle's pooled value."""
    with np.errstate(invalid="ignore"):
        d = np.asarray(x, np.float64) - np.asarray(out_exp, np.float64)
    return b_out + sub_rounding(d, b_out) + half_ulp(thr)


def impulse_decision_bound(up_exp, b_up, n, thr):
    """``up[p] - up[p +- n] > thr`` (``impulse_compare_kernel``, :158-163), (..., P, S) arrays: two smoothed values and
    one subtraction per side, the threshold rounded to float32.  The mask is the AND of two comparisons, so it can differ
    from the oracle's only where ONE of them is within ITS bound.  Returns (margin, bound) for ``check_decisions``:
    ``margin`` = the smaller of |difference - thr| / bound over the two sides, ``bound`` = 1 (a missing side or a NaN
    difference counts as +inf on both sides of the comparison: ratio inf)."""
    up = np.asarray(up_exp, np.float64)
    b = np.broadcast_to(np.asarray(b_up, np.float64), up.shape)
    P = up.shape[-2]
    ratio = np.full(up.shape, np.inf)
    k = max(P - n, 0)
    for sgn in (1, -1):
        d = np.full(up.shape, np.nan)
        bb = np.zeros(up.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            if sgn > 0:
                d[..., :k, :] = up[..., :k, :] - up[..., n:, :]
                bb[..., :k, :] = b[..., :k, :] + b[..., n:, :]
            else:
                d[..., n:, :] = up[..., n:, :] - up[..., :k, :]
                bb[..., n:, :] = b[..., n:, :] + b[..., :k, :]
            bb = bb + sub_rounding(d, bb) + half_ulp(thr)
            r = np.abs(d - thr) / bb
        r = np.where(np.isnan(r), np.inf, r)     # (a NaN difference or bound belongs to a NaN value: +inf > thr)
        ratio = np.minimum(ratio, r)
    return ratio, np.ones(up.shape)


def attenuated_decision_bound(ping_db, block_db, thr):
    """``ping_db - block_db < thr`` (:642-644; the walk, :2889,:2914): both medians cast to float32
    (``pooled_median_bound``), one float32 subtraction, the threshold rounded to float32."""
    b = pooled_median_bound(ping_db) + pooled_median_bound(block_db)
    with np.errstate(invalid="ignore"):
        d = np.asarray(ping_db, np.float64) - np.asarray(block_db, np.float64)
    return b + sub_rounding(d, b) + half_ulp(thr)


def assert_few_near(margin, bound, what="", cap=1e-3):
    """The cap on what a decision check may leave out: at most ``cap`` of the decisions may lie within the bound of the
    threshold (a condition on the INPUT, asserted before comparing)."""
    with np.errstate(invalid="ignore"):
        near = np.abs(np.asarray(margin, np.float64)) <= np.broadcast_to(np.asarray(bound, np.float64), np.shape(margin))
    assert near.mean() <= cap, f"{what}: {int(near.sum())} of {near.size} decisions lie within the bound of the threshold"
    return int(near.sum())


# ------------------------------------------------------------------------------------------------ checks
def _log(what, err, ratio, shape, **extra):
    path = os.environ.get("EPA_F32_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"what": what, "max_err": err, "max_ratio": ratio, "shape": list(shape), **extra}) + "\n")


def assert_f32_close(got, exp, bound, what=""):
    """float32 ``got`` against the float64 ``exp``: the same NaN and inf pattern, |got - exp| <= bound at every finite
    element, and the old north-star bar |got - exp| / max(|exp|, 1) <= 1e-3 as well.  Returns (max error,
    max error / bound)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), exp.shape)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{what}: NaN pattern")
    np.testing.assert_array_equal(np.isinf(got), np.isinf(exp), err_msg=f"{what}: inf pattern")
    inf = np.isinf(exp)
    np.testing.assert_array_equal(got[inf], exp[inf], err_msg=f"{what}: inf sign")
    fin = np.isfinite(exp)
    if not fin.any():
        return 0.0, 0.0
    err = np.abs(got[fin] - exp[fin])
    old = err / np.maximum(np.abs(exp[fin]), 1.0)
    assert old.max() <= OLD_RTOL, f"{what}: old bar, max rel err {old.max():.3e}"
    assert np.all(np.isfinite(bound[fin])), f"{what}: an element without a finite bound"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound[fin], 0.0)
    k = int(np.argmax(ratio))
    assert ratio[k] <= 1.0, (f"{what}: |err| {err[k]:.3e} dB > bound {bound[fin][k]:.3e} dB at "
                             f"{np.unravel_index(np.flatnonzero(fin)[k], exp.shape)} (exp {exp[fin][k]!r}, "
                             f"got {got[fin][k]!r})")
    _log(what, float(err.max()), float(ratio.max()), exp.shape)
    return float(err.max()), float(ratio.max())


def check_decisions(got_keep, exp_keep, margin, bound, what="", max_frac=None):
    """A decision (keep / remove, inside / outside) may differ from the oracle's only where the oracle's margin to the
    threshold is within ``bound`` of the quantity compared: |margin| <= bound.  ``max_frac`` keeps an existing
    fraction limit on top.  Returns the number of flips."""
    got_keep, exp_keep = np.asarray(got_keep, bool), np.asarray(exp_keep, bool)
    flip = got_keep != exp_keep
    nflip = int(flip.sum())
    if nflip:
        m = np.abs(np.broadcast_to(np.asarray(margin, np.float64), flip.shape)[flip])
        b = np.broadcast_to(np.asarray(bound, np.float64), flip.shape)[flip]
        bad = ~(m <= b)
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {nflip} decision flips lie outside the bound, e.g. "
                               f"margin {m[bad][0]:.3e} > bound {b[bad][0]:.3e}")
    if max_frac is not None:
        assert nflip <= max_frac * flip.size, (what, nflip, flip.size)
    return nflip


# ------------------------------------------------------------------------------------------------ EK80 broadband
# The pulse-compressed routes (csrc/lds_fft.h, csrc/ek80_fft.hip, csrc/ek80_complex.hip, csrc/splitbeam.hip).  The
# oracle is the plain correlation y[k] = sum_j x[k + j] conj(h[j]) in float64 / longdouble of exactly the float32
# samples and complex64 replica the kernel read.
NFFT = 2048                       # EPA_EK80_NFFT: the tile of the LDS transform
ULD = 2.0**-64                    # unit roundoff of the x87 long double the complex128 transform's oracle sums in
E_SINCOS = 2.0                    # ocml's double sincospi: ulp of its result (the twiddle table, ek80_fft.hip:106)


def _cmul_rel(u):
    """|fl(a b) - a b| <= (2u + u^2) |a b| for the product-then-fma complex product (lds_fft.h:53-55 ``cmul``, :375
    ``pk::cmul`` = v_pk_mul then v_pk_fma): re = fl(a_r b_r - fl(a_i b_i)), im = fl(a_r b_i + fl(a_i b_r)); the inner
    products err by u |a_i b_i|, u |a_i b_r| (together u |a_i| |b| in norm), the fma rounds the result once (u |a b|
    (1 + u))."""
    return 2 * u + u * u


def _twiddle_rel(tau1, u, radix):
    """Largest relative error of v[q] * w^q over q = 1 .. radix-1 for ``twiddle8`` (lds_fft.h:109-120, :414-423) /
    ``twiddle4`` (:121-128, :424-429): w1 carries tau1, the powers come from the product tree w2 = w1 w1, w3 = w2 w1,
    w4 = w2 w2, w5 = w4 w1, w6 = w3 w3, w7 = w4 w3 (depth 1 to 3), each product (1 + tau_a)(1 + tau_b)(1 + cmul) - 1,
    and the application to v[q] is one more ``cmul``.  A tone can put a tile's whole energy into one register q, so the
    normwise constant of the step is the largest of them (q = 7: about 21 u for tau1 = u; q = 3 of the first pass's
    second butterfly: about 18 u)."""
    cm = _cmul_rel(u)

    def mul(a, b):
        return (1 + a) * (1 + b) * (1 + cm) - 1

    w = {1: tau1}
    w[2] = mul(w[1], w[1])
    w[3] = mul(w[2], w[1])
    if radix == 8:
        w[4] = mul(w[2], w[2])
        w[5] = mul(w[4], w[1])
        w[6] = mul(w[3], w[3])
        w[7] = mul(w[4], w[3])
    return max((1 + w[q]) * (1 + cm) - 1 for q in range(1, radix))


def fft_constants(u=U):
    """The normwise constants of ``correlate<F>`` (lds_fft.h:276-335 for double, :444-523 for float), u = U (complex64)
    or U64 (complex128): dict(fwd, prod, inv, total), each a relative error in the 2-norm of the tile.

    Every pass is sqrt(r) times a unitary map followed or preceded by a diagonal map of unit-modulus twiddles, so an
    error e of norm <= eps ||z|| made in one step reaches the output with the same relative norm and the steps compound
    as prod(1 + eps_i) - 1.
      complex add / sub (``cadd``, v_pk_add, also with the exact factors -i, +i through op_sel / neg): one rounding per
          component -> u ||result||.
      ``dft4`` (:71-77, :378-384): two stages of adds -> (1 + u)^2 - 1.
      ``dft8`` (:79-91, :393-413): dft4 on evens and odds, then out = e +- rot(o).  The rotations of o1, o3 by
          e^{-+i pi/4}: float forms q = o -+ i o (one rounding), then fma(q, kh, e) -- kh = fl(1/sqrt 2) (<= u) -- so
          rot(o) carries rho = (1 + u)^2 - 1 before the fma's own rounding; double multiplies (o_r + o_i) kh first
          (three roundings: rho = (1 + u)^3 - 1).  ||o|| <= ||out|| / sqrt 2 and an error dt of rot(o) enters two
          outputs (sqrt 2 ||dt||): stage 3 errs by (1 + u)(1 + rho) - 1 of ||out||.
          -> dft8 = (1 + u)^3 (1 + rho) - 1  (5 u float, 6 u double); the inverse forms are the same operations.
      twiddle table (ek80_fft.hip:104-111): double sincospi (E_SINCOS ulp), rounded to F: tau = u + 2 E_SINCOS 2^-53.
      first pass (``fwd_pass0`` :172-180, :456-462): dft4, then ``twiddle4`` with wa = table entry and
          wb = kh (wa - i wa): one add, one product, kh -> tau_b = (1 + tau)(1 + u)^3 - 1.
      inner passes: dft8 then ``twiddle8`` with a table entry (double: the 68-entry table holds every index they use,
          ``tw_mul4`` :159-162).
      last pass (``inv_pass0`` :181-190, :514-520): the conjugate twiddles (exact sign flip), then idft4; double takes
          wa = ``tw_any`` = one ``cmul`` of two table entries (:154-158).
      spectral product (:310, :490): the spectrum entry (ek80_fft.hip:161-166: double, 1/N folded in exactly, float
          rounds it once: u per component; the double transform that made it is charged in ``fft_tile_bound``), one
          ``cmul``.
    Sum for complex64: forward 2 + 18 + 2 (5 + 21) + 5 = 77 u, product 3 u, inverse the same 77 u: total about 157 u
    (computed exactly below, with the second-order terms).  Derived, not measured."""
    double = u < U
    cm = _cmul_rel(u)
    dft4 = (1 + u) ** 2 - 1
    rho = (1 + u) ** 3 - 1 if double else (1 + u) ** 2 - 1
    dft8 = (1 + u) ** 3 * (1 + rho) - 1
    tau = u + 2 * E_SINCOS * U64
    tau_b = (1 + tau) * (1 + u) ** 3 - 1
    tw4_fwd = max(_twiddle_rel(tau, u, 4), _twiddle_rel(tau_b, u, 4))
    tau_inv = (1 + tau) ** 2 * (1 + cm) - 1 if double else tau
    tau_inv_b = (1 + tau_inv) * (1 + u) ** 3 - 1
    tw4_inv = max(_twiddle_rel(tau_inv, u, 4), _twiddle_rel(tau_inv_b, u, 4))
    inner = (1 + dft8) * (1 + _twiddle_rel(tau, u, 8)) - 1
    fwd = (1 + dft4) * (1 + tw4_fwd) * (1 + inner) ** 2 * (1 + dft8) - 1
    inv = (1 + dft8) * (1 + inner) ** 2 * (1 + tw4_inv) * (1 + dft4) - 1
    prod = (1 + (0.0 if double else u)) * (1 + cm) - 1
    return dict(fwd=fwd, prod=prod, inv=inv, total=(1 + fwd) * (1 + prod) * (1 + inv) - 1)


def fft_tile_bound(x, h, u=U, u_oracle=U64):
    """Normwise bound of one ``correlate<F>`` tile (lds_fft.h:276-335, :444-523):
        || got - y ||_2 <= K ||x||_2 max_k |FFT(h)_k| + (1 + K) sqrt(N) K64 ||x||_2 ||h||_2 (+ the oracle's own sums)
    for y[k] = sum_j x[(k + j) mod N] conj(h[j]), N = 2048; every sample's error is at most that.

    K = ``fft_constants(u)['total']`` (about 157 u for complex64).  Why ||x||_2 max|H|: with X = FFT(x) (norm sqrt N
    ||x||), the spectrum H = conj(FFT(h)) / N and y = IFFT_unnormalised(X H) (norm sqrt N ||X H||), a forward error of
    relative norm eps reaches the product as at most eps ||X|| max|H|, i.e. eps ||x|| max|FFT(h)| in y; the product's
    and the inverse's errors are relative to ||X H|| <= ||X|| max|H| as well.
    The spectrum itself comes from the double transform of ``replica_prepare_kernel`` (ek80_fft.hip:135-166: the
    scalar templates, full twiddle table): || dH ||_2 <= K64 ||H||_2 with K64 = ``fft_constants(U64)['fwd']``; a tone
    can put all of X into the one bin where dH sits, so that part is bounded by max|X| ||dH|| <= ||X||_2 K64 ||H||_2,
    which is sqrt(N) K64 ||x||_2 ||h||_2 in y.  (For complex64 it is 1e-13 of the first term.)
    The oracle's plain sum in precision ``u_oracle``: gamma_{2 taps} (|x| * |h|)[k] <= gamma ||x|| ||h|| per sample.
    ``x`` (..., 2048) complex: the tile(s) as the transform received them; ``h`` complex replica (<= 2048 taps).
    Returns the bound per tile, shape x.shape[:-1]."""
    x = np.asarray(x)
    h = np.asarray(h).astype(np.complex128)
    assert x.shape[-1] == NFFT and h.size <= NFFT
    xn = np.sqrt(np.sum(np.abs(x.astype(np.complex128)) ** 2, axis=-1))
    hn = float(np.sqrt(np.sum(np.abs(h) ** 2)))
    hmax = float(np.abs(np.fft.fft(h, NFFT)).max()) * (1 + 64 * U64) + 64 * U64 * hn
    K = fft_constants(u)["total"]
    K64 = fft_constants(U64)["fwd"]
    g_or = 2 * h.size * u_oracle / (1 - 2 * h.size * u_oracle)
    return K * xn * hmax + np.sqrt(NFFT) * ((1 + K) * K64 + g_or) * xn * hn


def direct_form_bound(x, h, u=U, u_oracle=U64):
    """Per-sample bound of the direct form ``conv8`` (ek80_complex.hip:139-165) on one staged series ``x`` (1-D complex,
    zero-filled) with the replica ``h``: each component is a chain of 2 taps fused multiply-adds in the accumulation
    type (:156-159), so
        |d re[k]| <= gamma_{2 taps} sum_j (|x_r| |h_r| + |x_i| |h_i|)[k + j],   |d im[k]| likewise with (|x_i| |h_r| +
        |x_r| |h_i|)
    (zero-padded taps add exact zeros) and the complex error is their hypot.  Local -- relative to the products under
    the sample's own window, not to the tile's peak.  Returns (S,) for y[k] = sum_j x[k + j] conj(h[j]), k + j < S."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.complex128)
    n = 2 * h.size

    def g(uu):
        return n * uu / (1 - n * uu)

    def cor(a, b):
        return np.convolve(np.concatenate([a, np.zeros(b.size - 1)]), b[::-1], mode="valid")

    xr, xi, hr, hi = np.abs(x.real), np.abs(x.imag), np.abs(h.real), np.abs(h.imag)
    er = cor(xr, hr) + cor(xi, hi)
    ei = cor(xi, hr) + cor(xr, hi)
    return (g(u) + g(u_oracle)) * np.hypot(er, ei)


def sector_sum_bound(abs_re_sum, abs_im_sum, B, u=U):
    """The staged sector sum in F (``sum_plain`` ek80_fft.hip:289-299, ``load_sample`` :192-256, ``stage_tile``
    ek80_complex.hip:113-124): B - 1 additions in any order -> |d| <= gamma_{B-1} hypot(sum_b |re_b|, sum_b |im_b|)."""
    m = max(B - 1, 0)
    return m * u / (1 - m * u) * np.hypot(abs_re_sum, abs_im_sum)


def norm_scale_rel(taps, form, u=U):
    """Relative error of the factor 1 / (||h||^2 n) the amplitude is scaled with, including the product with y.
      "fft" (ek80_fft.hip:133,142-145,404-406,601-603): ||h||^2 and its reciprocal in double (a sum of taps positive
          terms: gamma64_{taps + 8}), the product (double) y invn in double, one rounding to T -> u + (taps + 12) 2^-53.
      "direct" (ek80_complex.hip:196-209, 266, 279-281): ||h||^2 summed in the accumulation type -- per tap a square
          and an fma (2 roundings), one add per 256-tap round of a lane, six shuffle adds, three adds of the wavefront
          sums, all terms positive: (1 + u)^(2 + ceil(taps8 / 256) + 9) - 1; then 1 / norm2, / n valid sectors and the
          product with y: three more roundings (division in HIP is correctly rounded by default)."""
    if form == "fft":
        return u + (taps + 12) * U64
    taps8 = -(-taps // 8) * 8
    return (1 + u) ** (2 + -(-taps8 // 256) + 9 + 3) - 1


def _range_terms_bound(prx, Rt, R, shift, alpha2, const, nspread, U=U):
    """The dB terms around the received power, as ``cw_complex_bound`` derives them (the epilogues of
    ek80_complex.hip:283-293 and ek80_fft.hip:605-620 are the CW kernel's): returns (bound without the power's own
    relative error, sum of |term|).  ``U``: unit roundoff of the output type (float64 output: the table-driven double
    logarithm, 4e-16 relative, fast_math.h:6, is within E_LOG ulp as well, and the tabulated time-varied gain holds the
    per-sample form's roundings, ek80_fft.hip:342-365)."""
    Tp = np.abs(10 * np.log10(prx))
    drt = U * (np.abs(R) + np.abs(shift) + np.abs(Rt))
    rel_rt = drt / Rt
    Ts = np.abs(nspread * np.log10(Rt))
    b_s = abs(nspread) / LN10 * rel_rt / (1 - rel_rt) + (2 * E_LOG + 1) * U * Ts
    Ta = np.abs(alpha2 * Rt)
    b_a = 2 * U * Ta + np.abs(alpha2) * drt
    Tc = np.abs(const)
    tot = Tp + Ts + Ta + Tc
    return (2 * E_LOG + 1) * U * Tp + b_s + b_a + U * Tc + 3 * U * tot, tot


def bb_sample_bound(delta, y_abs, scale, eps_scale, pscale, prx, Rt, R, shift, alpha2, const, nspread, u_t=U):
    """From an amplitude bound ``delta`` of the summed, pulse-compressed sectors y to the float32 Sv / TS and to the
    linear amplitude sqrt(prx), for either form.  Returns (b_db, b_lin).

      m = y * scale, scale = 1 / (||h||^2 n): |dm| <= d' = scale (delta (1 + eps_scale) + |y| eps_scale)
          (``norm_scale_rel``: ek80_fft.hip:601-603 ``mr = (T)(y * invn)`` through double; ek80_complex.hip:279-281)
      prx = fl(pscale) (mr mr + mi mi) (ek80_fft.hip:605, ek80_complex.hip:283): fl(pscale) (u), the sum of squares
          (two roundings), the product (u):  relative error e_p = (1 + (2 |m| d' + d'^2) / |m|^2)(1 + u)^4 - 1, as
          ``cw_complex_bound``
      10 log10f(prx) (``fast_log10_lean<float>`` is log10f: E_LOG), the time-varied gain n log10f(R') + 2 alpha R'
          per ping (float output never takes the table, ek80_fft.hip:410-411), the additions and the final rounding:
          ``_range_terms_bound``
      -> b_db = DB -ln(1 - e_p) + the range terms; infinite where e_p >= 1 (the sample is at the error floor).
      linear: sqrt(prx_got) = sqrt(pscale) |m_got| sqrt(1 + eta), |eta| <= (1 + u)^4 - 1 = e4:
          |sqrt(prx_got) - sqrt(prx_exp)| <= sqrt(pscale) (d' + (|m| + d') e4 / 2 (1 + e4)) + sqrt(4 pscale 2^-149)
          (the last term: a sum of squares in float32's subnormal range is off by up to a few 2^-149 absolutely).
          It needs no dynamic-range exclusion: it is finite at every sample.
    delta, y_abs, prx, Rt, R (C, P, S); scale, pscale, shift, alpha2, const broadcast to it.  ``u_t``: unit roundoff of
    the output type -- 2^-53 for a float32 transform under the float64 epilogue (no subnormal term then; the double
    logarithm's absolute error near 1, 2e-16, and the oracle's own evaluation go into 64 * 2^-53 (1 + sum |term|))."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = y_abs * scale
        d = scale * (delta * (1 + eps_scale) + y_abs * eps_scale)
        e4 = (1 + u_t) ** 4 - 1
        ep = (1 + (2 * m * d + d * d) / (m * m)) * (1 + e4) - 1
        rng, tot = _range_terms_bound(prx, Rt, R, shift, alpha2, const, nspread, u_t)
        b_db = (db_of_rel(ep) + rng) * (1 + 8 * u_t) + (8 if u_t == U else 64) * U64 * (tot + (0 if u_t == U else 1))
        tiny = np.sqrt(4 * pscale * TINY) if u_t == U else 0.0
        b_lin = (np.sqrt(pscale) * (d + (m + d) * e4 / 2 * (1 + e4)) + tiny) * (1 + 8 * U64)
    return b_db, b_lin


def assert_amp_close(got_prx, exp_amp, b_lin, what=""):
    """Every sample in LINEAR received amplitude: |sqrt(prx_got) - exp_amp| <= b_lin wherever ``exp_amp`` is a number
    (a NaN ``prx_got`` there is the kernels' "prx <= 0 -> NaN": amplitude 0).  Returns (max error, max ratio)."""
    got_prx, exp_amp = np.asarray(got_prx, np.float64), np.asarray(exp_amp, np.float64)
    b = np.broadcast_to(np.asarray(b_lin, np.float64), exp_amp.shape)
    fin = np.isfinite(exp_amp)
    assert np.all(np.isfinite(b[fin])), f"{what}: a sample without a finite linear bound"
    with np.errstate(invalid="ignore"):
        amp = np.sqrt(np.where(np.isnan(got_prx), 0.0, got_prx))
    err = np.abs(amp[fin] - exp_amp[fin])
    ratio = err / b[fin]
    k = int(np.argmax(ratio)) if ratio.size else 0
    assert ratio.size == 0 or ratio[k] <= 1.0, (f"{what}: amplitude off by {err[k]:.3e} > bound {b[fin][k]:.3e} at "
                                                f"{np.unravel_index(np.flatnonzero(fin)[k], exp_amp.shape)}")
    if ratio.size:
        _log(what, float(err.max()), float(ratio.max()), exp_amp.shape)
    return (float(err.max()), float(ratio.max())) if ratio.size else (0.0, 0.0)


def assert_norm_close(got, exp, bound, what=""):
    """One transform tile per row: ||got - exp||_2 <= bound and max |got - exp| <= bound.  Returns the largest ratio."""
    d = np.abs(np.asarray(got).astype(np.clongdouble) - np.asarray(exp).astype(np.clongdouble)).astype(np.float64)
    l2 = np.sqrt(np.sum(d * d, axis=-1))
    bound = np.broadcast_to(np.asarray(bound, np.float64), l2.shape)
    assert np.all(np.isfinite(np.asarray(got).view(np.float64 if np.asarray(got).dtype == np.complex128 else np.float32))), \
        f"{what}: non-finite output"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(l2 > 0, l2 / bound, 0.0)
    k = int(np.argmax(ratio))
    assert ratio[k] <= 1.0, f"{what}: tile {k}: ||err||_2 {l2[k]:.3e} > bound {bound[k]:.3e}"
    assert np.all(d.max(axis=-1) <= bound), f"{what}: a sample's error exceeds the tile bound"
    _log(what, float(l2.max()), float(ratio.max()), np.shape(got))
    return float(ratio.max())


E_ATAN2 = 2.0                     # atan2f / atan2: ulp of the result (HIP's documented accuracy)


def phase_bound_deg(a_abs, da, b_abs, db, u_t=U64):
    """Bound, in degrees, of the angle of a conj(b) computed from a, b known to |da|, |db| (csrc/splitbeam.hip:92-97
    ``angle_deg`` in the output type T, unit roundoff ``u_t``):
      the factors: the phase of a moves by at most asin(da / |a|), of b by asin(db / |b|) (infinite once the bound
          reaches the factor: the sample's phase is then not determined);
      re = ar br + ai bi, im = ai br - ar bi: two roundings each (a product and an fma, or three operations of which
          the sum rounds the larger): |d re|, |d im| <= gamma_2 |a| |b| -> asin(sqrt 2 gamma_2);
      atan2 (E_ATAN2 ulp of a result <= pi), the factor 180 / pi rounded to T (u) and the product (u)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ra, rb = da / a_abs, db / b_abs
        pa = np.where(ra < 1, np.arcsin(np.minimum(ra, 1.0)), np.inf)
        pb = np.where(rb < 1, np.arcsin(np.minimum(rb, 1.0)), np.inf)
    g2 = 2 * u_t / (1 - 2 * u_t)
    rad = pa + pb + np.arcsin(np.sqrt(2) * g2) + 2 * E_ATAN2 * u_t * np.pi
    return np.degrees(rad) * (1 + 2 * u_t) + 2 * u_t * 180.0


def splitbeam_angle_bound(b0, b1, e_al, e_at, four, sens_al, off_al, sens_at, off_at, u_t=U64):
    """Bound of the ELECTRICAL angles (theta + offset) sensitivity the split-beam tests compare (splitbeam_ref
    ``electrical``), from the phase bounds b0, b1 (``phase_bound_deg``) of the two products
    (``finish``, csrc/splitbeam.hip:100-109; the combination products of ``splitbeam_ref.combinations``):
      four sectors (type 1): e_al = ang0, e_at = ang1;
      three sectors: e_al = (ang0 + ang1) / sqrt 3 (an add, fl(sqrt 3) and a division: 3 u), e_at = ang1 - ang0 (u);
      theta = e / fl(sens) - fl(off) in T: fl(sens) (u), the division (u), fl(off) (u |off|), the subtraction
          (u |theta|); back in electrical degrees: 2 u |e| + u |off sens| + u |e - off sens|.
    Returns (b_al, b_at)."""
    e_al, e_at = np.abs(e_al), np.abs(e_at)
    if four:
        ba, bt = b0, b1
    else:
        ba = (b0 + b1) / np.sqrt(3.0) + 3 * u_t * e_al
        bt = b0 + b1 + u_t * e_at
    osa, ost = np.abs(off_al * sens_al), np.abs(off_at * sens_at)
    ba = ba + u_t * (3 * e_al + 2 * osa)
    bt = bt + u_t * (3 * e_at + 2 * ost)
    return ba * (1 + 8 * u_t) + 64 * U64 * (e_al + osa), bt * (1 + 8 * u_t) + 64 * U64 * (e_at + ost)
