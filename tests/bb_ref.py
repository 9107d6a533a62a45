"""NumPy oracle of the EK80 broadband (pulse-compressed) Sv / TS kernels and the inputs their bound tests share.

The oracle is the plain sum y[k] = sum_j x[k + j] conj(h[j]) in float64 (longdouble for the complex128 transform) of
exactly the float32 samples and the complex64 replica a kernel read; ``sv_case`` turns it into the expected Sv / TS,
the received amplitude and -- per form -- the amplitude bound ``delta`` of the summed sectors that
``f32_bounds.bb_sample_bound`` carries on to dB and to linear amplitude.  Results are cached: a case is computed once
and shared by every test (and parametrised row) that needs it; callers must not modify what they get.
"""
import functools

import numpy as np

import f32_bounds as fb

N = fb.NFFT
RA, RB, SHIFT, ALPHA2, A, PSCALE = range(6)   # the columns of a complex coefficient row (echopype_amd._lib.CC_*)


def correlate(x, h, dtype=np.complex128):
    """y[k] = sum_j x[k + j] conj(h[j]) for k < len(x), x taken as 0 beyond its end: a plain sum in ``dtype``."""
    x, h = np.asarray(x).astype(dtype), np.asarray(h).astype(dtype)
    return np.convolve(np.concatenate([x, np.zeros(h.size - 1, dtype)]), np.conj(h)[::-1], mode="valid")


def circ_correlate(x, h, dtype=np.complex128):
    """out[t, k] = sum_j x[t, (k + j) mod N] conj(h[j]) per row of ``x`` (T, N): a plain sum in ``dtype``."""
    x, h = np.asarray(x).astype(dtype), np.asarray(h).astype(dtype)
    hr = np.conj(h)[::-1]
    ext = np.concatenate([x, x[:, :h.size - 1]], axis=1)
    return np.stack([np.convolve(row, hr, mode="valid") for row in ext])


def _cor_real(a, b):
    return np.convolve(np.concatenate([a, np.zeros(b.size - 1)]), b[::-1], mode="valid")


def window_has_product(nz_x, nz_h):
    """Boolean correlation of the non-zero masks: True at k where some j has x[k + j] != 0 and h[j] != 0."""
    return _cor_real(nz_x.astype(np.float64), nz_h.astype(np.float64)) > 0.5


# ---------------------------------------------------------------------------------------------------- inputs
def fft_path_case(taps, S, mixed, B):
    """The inputs of test_sv_complex_fft_path_matches_direct (echoes over 140 dB, NaN tails, a missing ping, partly-NaN
    sectors, a missing beam 0, two replica lengths, per-ping coefficients) as float64 arrays."""
    rng = np.random.default_rng(taps + S)
    C, P = 2, 5
    amp = 10.0 ** rng.uniform(-7, 0, (C, P, S, 1))
    re = amp * rng.standard_normal((C, P, S, B))
    im = amp * rng.standard_normal((C, P, S, B))
    re[:, :, S - 37:], im[:, :, S - 37:] = np.nan, np.nan  # end-of-ping padding
    re[1, 1], im[1, 1] = np.nan, np.nan                    # a whole missing ping
    if mixed:
        re[0, 0, 100:130, B - 1] = np.nan                  # one sector missing -> per-sector fallback
        im[0, 2, S // 2, 0] = np.nan
        re[1, 0, 200:203, 0] = np.nan                      # beam 0 missing: masked echo_range, Sv NaN (B > 1: others valid)
    lens = [taps, max(taps // 2, 1)]
    rep = np.concatenate([(rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.hanning(n + 2)[1:-1]
                          for n in lens]).astype(np.complex64)
    cc = np.zeros((C, P, 8))
    cc[..., 0], cc[..., 1], cc[..., 2], cc[..., 3], cc[..., 4], cc[..., 5] = 2.6e-5, 750.0, 0.2, 0.02, -30.0, 1e3
    # a ping with its own sound speed / absorption: it leaves the per-channel time-varied-gain table (and its
    # neighbours in a tile do not)
    cc[0, 2, 1], cc[1, 2, 3] = 751.5, 0.021
    cc[:, 3, 4], cc[:, 4, 5] = -31.5, 1.1e3                 # per-ping gain / power terms
    return re, im, rep, lens, cc


def flat_case(taps=177, S=4500, B=4, seed=11):
    """A "flat" input: every finite sample within 40 dB of its tile's peak.  Each sector is a common unit-modulus
    sequence, constant over ``taps`` samples (so that a window's sum is ~taps times the sample, never a cancellation),
    times a level within 6 dB and a sector gain; the replica is an untapered one-level chirp-free sequence of ones with
    a slow phase ramp.  Ragged end, NaN tail, a partly-NaN sector run and a missing beam 0 as in ``fft_path_case``."""
    rng = np.random.default_rng(seed)
    C, P = 2, 3
    ph = np.repeat(rng.uniform(0, 2 * np.pi, (C, P, -(-S // taps))), taps, axis=2)[:, :, :S]
    lev = 10.0 ** rng.uniform(-0.3, 0.0, (C, P, S))
    z = (lev * np.exp(1j * ph))[..., None] * (1.0 + 0.1 * np.arange(B))
    re, im = z.real.copy(), z.imag.copy()
    re[:, :, S - 29:], im[:, :, S - 29:] = np.nan, np.nan
    re[0, 1, 300:340, B - 1] = np.nan
    re[1, 0, 900:903, 0] = np.nan
    lens = [taps, max(taps // 2, 1)]
    rep = np.concatenate([np.exp(1j * 0.003 * np.arange(n)) for n in lens]).astype(np.complex64)
    cc = np.zeros((C, P, 8))
    cc[..., 0], cc[..., 1], cc[..., 2], cc[..., 3], cc[..., 4], cc[..., 5] = 2.6e-5, 750.0, 0.2, 0.02, -30.0, 1e3
    cc[0, 1, 1], cc[1, 2, 3] = 751.5, 0.021
    return re, im, rep, lens, cc


# ---------------------------------------------------------------------------------------------------- the oracle
def sv_oracle(re, im, rep, lens, cc, nspread=20.0):
    """The reference's arithmetic (calibrate_ek.py:483-490, 571-638 after ek80_complex.py:285-391) in float64 on the
    float32 values of ``re`` / ``im`` (C, P, S, B) and the complex64 replicas ``rep`` (concatenated, lengths ``lens``).
    A sector contributes to output k where it is valid at k; NaN samples enter the filter as zeros."""
    re = np.asarray(re).astype(np.float32).astype(np.float64)
    im = np.asarray(im).astype(np.float32).astype(np.float64)
    C, P, S, B = re.shape
    ok = ~(np.isnan(re) | np.isnan(im))
    xz = np.where(ok, re + 1j * im, 0.0)
    off = np.cumsum([0] + list(lens))
    reps = [np.asarray(rep[off[c]:off[c + 1]]).astype(np.complex128) for c in range(C)]
    yb = np.empty((C, P, S, B), np.complex128)
    for c in range(C):
        for p in range(P):
            for b in range(B):
                yb[c, p, :, b] = correlate(xz[c, p, :, b], reps[c])
    nvalid = ok.sum(-1)
    y = np.where(ok, yb, 0.0).sum(-1)
    hn2 = np.array([np.sum(np.abs(h) ** 2) for h in reps])[:, None, None]
    s = np.arange(S)[None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.where(nvalid > 0, 1.0 / (hn2 * np.maximum(nvalid, 1)), np.nan)
        m_abs = np.abs(y) * scale
        pscale = cc[..., PSCALE:PSCALE + 1]
        amp = np.sqrt(pscale) * m_abs                      # NaN where no sector is valid, 0 under an empty window
        prx = pscale * m_abs**2
        prx = np.where(prx > 0, prx, np.nan)
        R = (s * cc[..., RA:RA + 1]) * cc[..., RB:RB + 1]
        range_ok = ~np.isnan(re[..., 0])
        Rt = R - cc[..., SHIFT:SHIFT + 1]
        Rt = np.where((Rt > 0) & range_ok, Rt, np.nan)
        exp = 10 * np.log10(prx) + nspread * np.log10(Rt) + cc[..., ALPHA2:ALPHA2 + 1] * Rt + cc[..., A:A + 1]
    return dict(re=re, im=im, ok=ok, xz=xz, reps=reps, yb=yb, y=y, nvalid=nvalid, scale=scale, amp=amp, prx=prx, R=R,
                Rt=Rt, exp=exp, cc=cc, nspread=nspread, shape=(C, P, S, B))


def _tiles_of(x, lo_step, n_tiles):
    """(n_tiles, N) zero-filled windows x[t * lo_step : t * lo_step + N] of a 1-D array."""
    out = np.zeros((n_tiles, N), x.dtype)
    for t in range(n_tiles):
        seg = x[t * lo_step:t * lo_step + N]
        out[t, :seg.size] = seg
    return out


def amplitude_bound(o, form, max_taps, u_f=fb.U):
    """``delta`` (C, P, S): bound of |y_kernel - y| for the summed, pulse-compressed sectors of ``form``.

    "fft" (ek80_fft.hip ``process_tile``): tiles of N staged samples, N - max_taps + 1 outputs each.
        A tile without a partly-NaN sample: the sector sum in F (``fb.sector_sum_bound``) goes through the exact filter
        (|d| * |h|) and the transform adds ``fb.fft_tile_bound`` of the staged tile (its norm taken with the sum's
        own error).  A tile with one (the MIXED pass, :490-565): one transform per sector, then up to B - 1 additions
        in F of the sectors valid at the sample.
    "direct" (ek80_complex.hip ``sv_complex_kernel``): tiles of 2048 outputs staged with taps8 + 8 more samples; the
        same two cases with ``fb.direct_form_bound`` (accumulation in the output type: float32)."""
    C, P, S, B = o["shape"]
    part = (o["nvalid"] > 0) & (o["nvalid"] < B)
    delta = np.zeros((C, P, S))
    g_b = max(B - 1, 0) * u_f / (1 - max(B - 1, 0) * u_f)
    opt = N - max_taps + 1
    for c in range(C):
        h = o["reps"][c]
        habs = np.abs(h)
        taps8 = -(-h.size // 8) * 8
        for p in range(P):
            xz = o["xz"][c, p]
            xs = xz.sum(-1)
            sr, si = np.abs(xz.real).sum(-1), np.abs(xz.imag).sum(-1)
            dsum = fb.sector_sum_bound(sr, si, B, u_f)
            d_through = _cor_real(dsum, habs)
            yb_abs = np.abs(o["yb"][c, p])
            if form == "fft":
                nt = -(-S // opt)
                xs_up = (np.abs(xs.real) + g_b * sr) + 1j * (np.abs(xs.imag) + g_b * si)
                b_sum = fb.fft_tile_bound(_tiles_of(xs_up, opt, nt), h, u_f)
                b_sec = [fb.fft_tile_bound(_tiles_of(xz[:, b], opt, nt), h, u_f) for b in range(B)]
                for t in range(nt):
                    lo, hi = t * opt, min(t * opt + opt, S)
                    if part[c, p, lo:lo + N].any():
                        eb = sum(b_sec[b][t] for b in range(B))
                        delta[c, p, lo:hi] = eb + g_b * (yb_abs[lo:hi].sum(-1) + eb)
                    else:
                        delta[c, p, lo:hi] = d_through[lo:hi] + b_sum[t]
            else:
                xs_up = (np.abs(xs.real) + g_b * sr) + 1j * (np.abs(xs.imag) + g_b * si)
                b_sum = d_through + fb.direct_form_bound(xs_up, h)
                b_mix = None
                for t in range(-(-S // N)):
                    lo, hi = t * N, min(t * N + N, S)
                    if part[c, p, lo:lo + N + taps8 + 8].any():
                        if b_mix is None:
                            eb = sum(fb.direct_form_bound(xz[:, b], h) for b in range(B))
                            b_mix = eb + g_b * (yb_abs.sum(-1) + eb)
                        delta[c, p, lo:hi] = b_mix[lo:hi]
                    else:
                        delta[c, p, lo:hi] = b_sum[lo:hi]
    return delta


def sample_bounds(o, form, max_taps, u_f=fb.U, u_t=fb.U):
    """(delta, b_db, b_lin) of ``form`` for the outputs of the oracle case ``o``: transform / accumulation precision
    ``u_f``, output type ``u_t`` (float32 unless a float32 transform runs under the float64 epilogue)."""
    cc = o["cc"]
    delta = amplitude_bound(o, form, max_taps, u_f)
    eps = np.array([fb.norm_scale_rel(h.size, form, u_t) for h in o["reps"]])[:, None, None]
    b_db, b_lin = fb.bb_sample_bound(delta, np.abs(o["y"]), o["scale"], eps, cc[..., PSCALE:PSCALE + 1], o["prx"],
                                     o["Rt"], o["R"], cc[..., SHIFT:SHIFT + 1], cc[..., ALPHA2:ALPHA2 + 1],
                                     np.broadcast_to(cc[..., A:A + 1], o["exp"].shape), o["nspread"], u_t)
    return delta, b_db, b_lin


@functools.lru_cache(maxsize=None)
def sv_case(kind, *key):
    """The cached oracle and per-form bounds of a named input: ``kind`` = "path" (``fft_path_case(*key)``), "flat"
    (``flat_case(*key)``) or "zeros" (``zeros_case(*key)``) -> dict(inputs, o, fft=(delta, b_db, b_lin), direct=(...))."""
    inputs = {"path": fft_path_case, "flat": flat_case, "zeros": zeros_case}[kind](*key)
    re, im, rep, lens, cc = inputs
    o = sv_oracle(re, im, rep, lens, cc)
    return dict(inputs=inputs, o=o, fft=sample_bounds(o, "fft", lens[0]), direct=sample_bounds(o, "direct", lens[0]))


def judge_sv(got_out, got_prx, case, form, what):
    """One form's float32 ``out`` / ``prx`` (C, P, S) against the oracle of ``case``:
      * NaN wherever the oracle is NaN for a structural reason (no valid sector, an empty window, a missing beam 0,
        R' <= 0) -- prx where the first two hold, the dB value where any does;
      * EVERY sample with a valid sector in linear amplitude (``fb.assert_amp_close``);
      * the dB value wherever ``b_db`` is finite: finite and within it.
    Returns dict(lin=(err, ratio), db=(err, ratio), judged_db=fraction of the finite samples with a finite dB bound)."""
    amp, b_lin = case["o"]["amp"], case[form][2]
    got_prx = np.asarray(got_prx, np.float64)
    empty = np.isnan(amp) | (amp == 0)
    assert np.isnan(got_prx[empty]).all(), f"{what}: prx is a number where no product enters the sample"
    lin = fb.assert_amp_close(got_prx, amp, b_lin, f"{what}: linear amplitude")
    db = judge_db(got_out, case, form, what)
    return dict(lin=lin, db=db[:2], judged_db=db[2])


def judge_db(got_out, case, form, what):
    """The dB values alone: NaN where the oracle is, a number within ``b_db`` wherever that bound is finite.  Returns
    (max error, max ratio, fraction of the oracle's finite samples with a finite bound)."""
    exp, b_db = case["o"]["exp"], case[form][1]
    got_out = np.asarray(got_out, np.float64)
    assert np.isnan(got_out[np.isnan(exp)]).all(), f"{what}: a dB value where the oracle has none"
    fin = np.isfinite(exp)
    judged = fin & np.isfinite(b_db)
    assert np.isfinite(got_out[judged]).all(), f"{what}: NaN at a sample whose dB bound is finite"
    err = np.abs(got_out[judged] - exp[judged])
    ratio = err / b_db[judged]
    k = int(np.argmax(ratio)) if ratio.size else 0
    assert ratio.size == 0 or ratio[k] <= 1.0, (f"{what}: |err| {err[k]:.3e} dB > bound {b_db[judged][k]:.3e} dB at "
                                                f"{np.unravel_index(np.flatnonzero(judged)[k], exp.shape)}")
    if ratio.size:
        fb._log(f"{what}: dB", float(err.max()), float(ratio.max()), exp.shape)
    frac = float(judged.sum()) / max(int(fin.sum()), 1)
    return (float(err.max()), float(ratio.max()), frac) if ratio.size else (0.0, 0.0, frac)


def case_of(re, im, rep, lens, cc, forms=("fft", "direct"), nspread=20.0):
    """The oracle and bounds of inputs given as arrays (uncached): as ``sv_case``."""
    o = sv_oracle(re, im, rep, lens, cc, nspread)
    return dict(inputs=(re, im, rep, lens, cc), o=o, **{f: sample_bounds(o, f, max(lens)) for f in forms})


# ---------------------------------------------------------------------------------------------------- CPU emulation
# What the CPU tests of the judge run in place of a kernel: the same operation ORDER in NumPy float32 (an fma as the
# float64 product-sum rounded once), the transform by scipy's complex64 pocketfft -- an ordinary complex64 transform,
# not the kernel's.
f32 = np.float32


def _sum32(xz):
    """Sector sum in float32, in sector order (``sum_plain`` / ``stage_tile``)."""
    r, i = xz.real.astype(f32), xz.imag.astype(f32)
    sr, si = r[..., 0].copy(), i[..., 0].copy()
    for b in range(1, xz.shape[-1]):
        sr, si = sr + r[..., b], si + i[..., b]
    return sr, si


def _direct32(xr, xi, h):
    """``conv8`` in float32: per tap four fused multiply-adds."""
    S = xr.size
    xr = np.concatenate([xr, np.zeros(h.size, f32)]).astype(np.float64)
    xi = np.concatenate([xi, np.zeros(h.size, f32)]).astype(np.float64)
    ar, ai = np.zeros(S, f32), np.zeros(S, f32)
    for j in range(h.size):
        tr, ti = float(h[j].real), float(h[j].imag)
        ar = (xr[j:j + S] * tr + ar).astype(f32)
        ar = (xi[j:j + S] * ti + ar).astype(f32)
        ai = (xi[j:j + S] * tr + ai).astype(f32)
        ai = (-xr[j:j + S] * ti + ai).astype(f32)
    return ar.astype(np.float64) + 1j * ai.astype(np.float64)


def fft32_tiles(tiles, h):
    """Circular correlation of (T, N) tiles with ``h`` through scipy's complex64 transform (spectrum: the double
    transform of the replica, 1/N folded in, rounded once to complex64 -- as ``replica_prepare_kernel``)."""
    import scipy.fft as sf

    spec = (np.conj(np.fft.fft(np.asarray(h).astype(np.complex128), N)) / N).astype(np.complex64)
    X = sf.fft(np.asarray(tiles).astype(np.complex64), axis=-1)
    assert X.dtype == np.complex64
    return (sf.ifft(X * spec, axis=-1) * f32(N)).astype(np.complex64)


def _fft32(xr, xi, h, opt, tile_fn=fft32_tiles):
    S = xr.size
    nt = -(-S // opt)
    x = xr.astype(np.complex64) + 1j * xi.astype(np.complex64)
    yt = tile_fn(_tiles_of(x, opt, nt), h)
    nz = _tiles_of((x != 0), opt, nt)
    y = np.zeros(S, np.complex128)
    for t in range(nt):
        lo, hi = t * opt, min(t * opt + opt, S)
        seg = yt[t, :hi - lo].astype(np.complex128)
        keep = window_has_product(nz[t], np.asarray(h) != 0)[:hi - lo]   # the exact zeros of the direct form
        y[lo:hi] = np.where(keep, seg, 0.0)
    return y


def emulate_y(o, form, max_taps, tile_fn=fft32_tiles):
    """The summed pulse-compressed sectors (C, P, S) as a float32 ``form`` computes them (values held in complex128)."""
    C, P, S, B = o["shape"]
    part = (o["nvalid"] > 0) & (o["nvalid"] < B)
    y = np.zeros((C, P, S), np.complex128)
    opt = N - max_taps + 1
    for c in range(C):
        h = o["reps"][c].astype(np.complex64)
        run = (lambda r, i: _fft32(r, i, h, opt, tile_fn)) if form == "fft" else (lambda r, i: _direct32(r, i, h))
        for p in range(P):
            xz = o["xz"][c, p]
            sr, si = _sum32(xz)
            ys = run(sr, si)
            if part[c, p].any():   # (the whole ping sector by sector: a superset of the kernels' mixed tiles, whose
                # non-mixed tiles see samples with all or no sectors and sum them first -- taken from ``ys`` below)
                ym = np.zeros(S, np.complex64)
                for b in range(B):
                    yb = run(xz[:, b].real.astype(f32), xz[:, b].imag.astype(f32)).astype(np.complex64)
                    ym = np.where(o["ok"][c, p, :, b], (ym.real + yb.real) + 1j * (ym.imag + yb.imag), ym).astype(np.complex64)
                step, span = (opt, N) if form == "fft" else (N, N + -(-h.size // 8) * 8 + 8)
                for t in range(-(-S // step)):
                    lo, hi = t * step, min(t * step + step, S)
                    if part[c, p, lo:lo + span].any():
                        ys[lo:hi] = ym[lo:hi]
            y[c, p] = ys
    return y


def epilogue32(o, y, form):
    """Sector mean -> prx -> Sv in float32 (ek80_fft.hip:590-637 / ek80_complex.hip:271-298) -> (out, prx)."""
    cc = o["cc"]
    C, P, S, B = o["shape"]
    hn2 = np.array([np.sum(np.abs(h) ** 2) for h in o["reps"]])[:, None, None]
    nv = np.maximum(o["nvalid"], 1)
    with np.errstate(all="ignore"):
        if form == "fft":
            invn = (1.0 / hn2) / nv
            mr, mi = (y.real * invn).astype(f32), (y.imag * invn).astype(f32)
        else:
            invn = (f32(1) / hn2.astype(f32)) / nv.astype(f32)
            mr, mi = y.real.astype(f32) * invn, y.imag.astype(f32) * invn
        prx = cc[..., PSCALE:PSCALE + 1].astype(f32) * (mr * mr + mi * mi)
        prx = np.where((prx > 0) & (o["nvalid"] > 0), prx, f32(np.nan))
        rt = o["R"].astype(f32) - cc[..., SHIFT:SHIFT + 1].astype(f32)
        rt = np.where((rt > 0) & ~np.isnan(o["re"][..., 0]), rt, f32(np.nan))
        tvg = f32(o["nspread"]) * np.log10(rt) + cc[..., ALPHA2:ALPHA2 + 1].astype(f32) * rt
        out = (f32(10) * np.log10(prx) + tvg) + cc[..., A:A + 1].astype(f32)
    assert out.dtype == f32 and prx.dtype == f32
    return out, prx


# ---------------------------------------------------------------------------------------------------- transform inputs
def transform_cases():
    """[(name, tiles (T, N) complex128, replica complex64)] for the transform self-test: inputs white noise does not
    reach.  Lane j of the kernel owns the samples j + 256 i (register i); after the first (radix-4) pass bin k lives in
    register k mod 4, then (k // 4) mod 8, (k // 32) mod 8 and (k // 256) mod 8 of the three radix-8 passes, so a tone
    of bin k exercises exactly one twiddle power per pass."""
    rng = np.random.default_rng(2048)

    def crand(n):
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)

    def padded(n, lead, trail):   # n taps in all, exact zeros at both ends
        h = crand(n)
        h[:lead] = 0
        if trail:
            h[n - trail:] = 0
        return h.astype(np.complex64)

    cases = []
    h177 = crand(177).astype(np.complex64)
    # a unit impulse at every register of first / last lanes of each wavefront and one inside
    pos = [j + 256 * i for j in (0, 37, 63, 64, 127, 128, 191, 192, 255) for i in range(8)]
    imp = np.zeros((len(pos), N), np.complex128)
    imp[np.arange(len(pos)), pos] = 1.0
    cases.append(("impulses", imp, h177))
    cases.append(("impulses, one-tap replica", imp[::5] * (0.3 - 1.1j), np.array([0.6 - 0.8j], np.complex64)))
    # single tones: every register of every pass, DC, Nyquist, the last bin
    bins = sorted(set(list(range(4)) + [4 * q for q in range(8)] + [32 * q for q in range(8)] +
                      [256 * q for q in range(8)] + [1 + 4 + 32 + 256, N // 2, N - 1]))
    n = np.arange(N)
    tones = np.exp(2j * np.pi * np.outer(bins, n) / N)
    cases.append(("tones", tones, h177))
    cases.append(("tones, one-tap replica", tones, np.array([-0.28 + 0.96j], np.complex64)))
    # purely real / purely imaginary data and replicas: a swapped half shows as a wrong quadrant
    xr, hr = rng.standard_normal((2, N)), rng.standard_normal(64)
    cases.append(("real data, real replica", xr + 0j, hr.astype(np.complex64)))
    cases.append(("imaginary data, imaginary replica", 1j * xr, (1j * hr).astype(np.complex64)))
    cases.append(("real data, imaginary replica", xr + 0j, (1j * hr).astype(np.complex64)))
    cases.append(("imaginary data, real replica", 1j * xr, hr.astype(np.complex64)))
    # white and 140 dB log-uniform tiles against replicas of 1, 16, 177, 1024 taps with exact-zero ends
    white = crand((2, N))
    wide = crand((2, N)) * 10.0 ** rng.uniform(-7, 0, (2, N))
    both = np.concatenate([white, wide])
    for taps, lead, trail in ((1, 0, 0), (16, 3, 2), (177, 5, 9), (1024, 17, 1)):
        cases.append((f"white and 140 dB tiles, {taps} taps ({lead} + {trail} zero)", both, padded(taps, lead, trail)))
    return cases


def transform_expected(tiles, h, u):
    """(x as the transform reads it, oracle, bound per tile): complex64 (u = fb.U) against the float64 plain sum,
    complex128 against the longdouble one."""
    if u == fb.U:
        x = np.asarray(tiles).astype(np.complex64)
        exp = circ_correlate(x, h, np.complex128)
        return x, exp, fb.fft_tile_bound(x, h, fb.U, fb.U64)
    x = np.asarray(tiles).astype(np.complex128)
    exp = circ_correlate(x, h, np.clongdouble)
    return x, exp, fb.fft_tile_bound(x, h, fb.U64, fb.ULD)


# ---------------------------------------------------------------------------------------------------- exact zeros
def zeros_case(taps=177, seed=3):
    """Exact-zero runs inside strong flat data (the background and replicas of ``flat_case``: a footprint's edge sample
    is one product of modulus ~1 x 1, far above the transform's bound).  Ping p has two runs, each longer than the
    replica so that some windows are empty: the first STARTS, the second ENDS on, one before or one after a multiple of
    64, of 256 or of the tile's output count N - taps + 1 (the seams) -- all nine combinations over the pings -- with
    two single non-zero samples inside the second; channel 1's replica starts and ends with exact-zero taps
    (``tap_lo`` / ``tap_hi``); two pings have a partly-NaN sector (the per-sector route)."""
    opt = N - taps + 1
    combos = [(al, of) for al in (64, 256, opt) for of in (-1, 0, 1)]
    C, P, B = 2, len(combos), 4
    runs = []
    for p, (al, of) in enumerate(combos):
        a = al * -(-100 // al) + of
        b = a + taps + 37 + p
        al2, of2 = combos[(p + 4) % P]
        b2 = al2 * -(-(b + 2 * taps + 300) // al2) + of2
        runs.append((a, b, b2 - taps - 150 - 3 * p, b2))
    S = max(max(r[3] for r in runs) + taps + 200, 2 * opt + 100)
    re, im, rep, lens, cc = flat_case(taps, S, B, seed)
    re, im, cc = np.resize(re[:, :1], (C, P, S, B)), np.resize(im[:, :1], (C, P, S, B)), np.resize(cc[:, :1], (C, P, 8))
    for p, (a, b, a2, b2) in enumerate(runs):
        re[:, p, a:b], im[:, p, a:b] = 0.0, 0.0
        re[:, p, a2:b2], im[:, p, a2:b2] = 0.0, 0.0
        re[:, p, a2 + 60], im[:, p, a2 + 61] = 0.75, -0.5      # single non-zero samples inside the long run
    re[0, 3, runs[3][1] + 5:runs[3][1] + 8, 1] = np.nan        # a partly-NaN sector: the per-sector route
    re[1, 6, runs[6][2] - 3, 2] = np.nan
    h1 = np.asarray(rep[lens[0]:]).copy()                      # channel 1: exact-zero first and last taps
    if h1.size > 8:
        h1[:3], h1[-2:] = 0, 0
    rep = np.concatenate([rep[:lens[0]], h1]).astype(np.complex64)
    return re, im, rep, lens, cc


def zero_pattern(o):
    """(C, P, S) bool: the sample's window holds a non-zero product of a sector valid at it (boolean correlation of the
    non-zero masks; tiles the kernels sum first see the sum's mask, which is the same wherever all sectors are zero
    together -- as in ``zeros_case``)."""
    C, P, S, B = o["shape"]
    has = np.zeros((C, P, S), bool)
    for c in range(C):
        nzh = o["reps"][c] != 0
        for p in range(P):
            for b in range(B):
                has[c, p] |= window_has_product(o["xz"][c, p, :, b] != 0, nzh) & o["ok"][c, p, :, b]
    return has


def footprint(case):
    """(has, sure) of a case: ``has`` the samples whose window holds a non-zero product of a valid sector, ``sure`` those
    of them whose oracle amplitude exceeds the FFT form's amplitude bound (no rounding can make them vanish)."""
    o = case["o"]
    has = zero_pattern(o) & (o["nvalid"] > 0)
    return has, has & (np.abs(o["y"]) > case["fft"][0])


def check_footprint(case, prx, form):
    """The NaN pattern of ``prx``: the direct form's is exactly ~has; the FFT form is NaN wherever the window holds no
    product and a number at every ``sure`` sample -- a decision may differ only where the oracle's amplitude is within
    the amplitude bound."""
    has, sure = footprint(case)
    nan = np.isnan(np.asarray(prx))
    if form == "direct":
        np.testing.assert_array_equal(nan, ~has, err_msg="direct form: NaN pattern")
        return
    assert nan[~has].all(), f"FFT form: {int((~nan[~has]).sum())} numbers outside the footprint"
    assert not nan[sure].any(), f"FFT form: NaN inside the footprint at {np.argwhere(sure & nan)[:5].tolist()}"


# ---------------------------------------------------------------------------------------------------- perturbations
def pass0_perturbed(x, h, n0, q, how):
    """The exact circular correlation of one tile with ONE element of the first (radix-4) pass's output disturbed:
    z_q[n] = (sum_r x[n + 512 r] e^{-2 pi i r q / 4}) w^(n q), X[4 k + q] = FFT_512(z_q)[k].  ``how`` = "twiddle":
    element (q, n0) takes the twiddle of table index n0 + 1 (w^((n0 + 1) q)); "swap": its real and imaginary halves
    are exchanged.  Returns (disturbed - exact), to be added to a result."""
    x = np.asarray(x).astype(np.complex128)
    n = np.arange(N // 4)
    z = np.stack([sum(x[n + 512 * r] * np.exp(-2j * np.pi * r * qq / 4) for r in range(4)) *
                  np.exp(-2j * np.pi * n * qq / N) for qq in range(4)])
    X = np.empty(N, np.complex128)
    for qq in range(4):
        X[qq::4] = np.fft.fft(z[qq])
    assert np.allclose(X, np.fft.fft(x), rtol=0, atol=1e-9 * np.abs(X).max())
    zp = z.copy()
    zp[q, n0] = z[q, n0] * np.exp(-2j * np.pi * q / N) if how == "twiddle" else z[q, n0].imag + 1j * z[q, n0].real
    Xp = X.copy()
    Xp[q::4] = np.fft.fft(zp[q])
    H = np.conj(np.fft.fft(np.asarray(h).astype(np.complex128), N))
    return np.fft.ifft((Xp - X) * H)
