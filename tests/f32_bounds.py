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
def _log(what, err, ratio, shape):
    path = os.environ.get("EPA_F32_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"what": what, "max_err": err, "max_ratio": ratio, "shape": list(shape)}) + "\n")


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
