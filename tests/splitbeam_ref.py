"""NumPy restatement of the reference's split-beam angles (consolidate/split_beam_angle.py) and the tolerance rule the
split-beam tests compare complex-sample angles with.  Used by test_splitbeam_host.py (against the reference-executed
goldens) and test_gpu_splitbeam.py (against the kernels)."""
import numpy as np

GOLDEN = "ref_splitbeam_goldens.npz"
SUPPORTED = (1, 17, 49, 65, 81)
QSCALE, QNAN = 4096.0, -32768  # scripts/gen_splitbeam_goldens.py encode_plane


def load_goldens(path):
    """The fixture as a dict; the complex sample planes (``*_re`` / ``*_im``, stored as int16 codes of the 2^-12 grid,
    QNAN = NaN) decoded to the float32 planes the reference was run on -- exactly."""
    g = dict(np.load(path))
    for k, v in g.items():
        if (k.endswith("_re") or k.endswith("_im")) and v.dtype == np.int16:
            g[k] = np.where(v == QNAN, np.float32(np.nan), v.astype(np.float32) / np.float32(QSCALE))
    return g


def power_angles(along, athw, sa, st, oa, ot):
    """split_beam_angle.py:142-148: (180/128) * angle / sensitivity - offset, in NumPy's promotion order (a Python
    float times a float32 plane stays float32).  Parameters broadcast over (channel[, ping_time])."""
    def bc(v):
        v = np.asarray(v, float)
        return v[:, None, None] if v.ndim == 1 else v[:, :, None]

    conv = 180.0 / 128.0
    a = along.astype(np.float64) if along.dtype.kind == "i" else along
    t = athw.astype(np.float64) if athw.dtype.kind == "i" else athw
    return (conv * a / bc(sa) - bc(oa)).astype(np.float64), (conv * t / bc(st) - bc(ot)).astype(np.float64)


def compress(x, tx):
    """compress_pulse of one (ping, sector) series (ek80_complex.py:316-369): NaN -> 0, y[k] = sum_j x[k+j] conj(tx[j])."""
    z = np.where(np.isnan(x), 0, x)
    return np.convolve(z, np.conj(tx)[::-1], mode="full")[tx.size - 1:]


def combinations(x, beam_type):
    """The sector combinations of a beam type (x: (..., B) complex), in the order the angles pair them:
    type 1 -> (fore, aft, star, port), others -> (fore, star, port)."""
    if beam_type == 1:
        return [(x[..., 2] + x[..., 3]) / 2, (x[..., 0] + x[..., 1]) / 2, (x[..., 0] + x[..., 3]) / 2,
                (x[..., 1] + x[..., 2]) / 2]
    if beam_type == 17:
        return [x[..., 2], x[..., 0], x[..., 1]]
    return [(x[..., 2] + x[..., 3]) / 2, (x[..., 0] + x[..., 3]) / 2, (x[..., 1] + x[..., 3]) / 2]


def complex_angles(re, im, beam_types, sa, st, oa, ot, replicas=None, replica_id=None):
    """Angles of complex samples in float64 arithmetic -> (theta, phi, electrical (e_al, e_at), weak) with ``weak``
    True where a factor of a product is below 1e-3 of its ping's RMS combination magnitude, or -- three-sector types --
    where a product lies within 1e-3 degrees of the negative real axis.  ``replicas``: list of
    complex replicas; ``replica_id`` (C, P) picks one per ping (default: replica c for channel c)."""
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    C, P, S, B = x.shape
    out = [np.full((C, P, S), np.nan) for _ in range(5)]
    weak = np.zeros((C, P, S), bool)

    def bc(v, c):
        v = np.asarray(v, float)
        return v[c] if v.ndim == 1 else v[c][:, None]

    for c in range(C):
        bt = int(beam_types[c])
        if bt not in SUPPORTED:
            continue
        xc = x[c]
        nan = np.isnan(xc).any(axis=-1) if bt != 17 else np.isnan(xc[..., :3]).any(axis=-1)
        if replicas is not None:
            y = np.empty_like(xc)
            for p in range(P):
                tx = replicas[c if replica_id is None else int(replica_id[c, p])]
                for b in range(B):
                    y[p, :, b] = compress(xc[p, :, b], tx)
            xc = y
        else:
            xc = np.where(np.isnan(xc), 0, xc)
        cmb = combinations(xc, bt)
        rms = [np.sqrt(np.mean(np.abs(k) ** 2, axis=-1, keepdims=True)) for k in cmb]
        small = np.zeros((P, S), bool)
        for k, r in zip(cmb, rms):
            small |= np.abs(k) <= 1e-3 * r
        if bt == 1:
            e_al = np.angle(cmb[0] * np.conj(cmb[1]), deg=True)
            e_at = np.angle(cmb[2] * np.conj(cmb[3]), deg=True)
        else:
            f1 = np.angle(cmb[0] * np.conj(cmb[1]), deg=True)
            f2 = np.angle(cmb[0] * np.conj(cmb[2]), deg=True)
            e_al, e_at = (f1 + f2) / np.sqrt(3), f2 - f1
            # a product on the negative real axis: its phase is +-180 by the sign of a zero (or of a last-bit rounding),
            # and the three-sector sum moves by 360 / sqrt 3 with it -- no wrap undoes that, it is not compared
            small |= (np.abs(np.abs(f1) - 180.0) < 1e-3) | (np.abs(np.abs(f2) - 180.0) < 1e-3)
        e_al[nan], e_at[nan] = np.nan, np.nan
        out[0][c], out[1][c] = e_al / bc(sa, c) - bc(oa, c), e_at / bc(st, c) - bc(ot, c)
        out[2][c], out[3][c] = e_al, e_at
        weak[c] = small
    return out[0], out[1], (out[2], out[3]), weak


def wrap(d):
    """Angle differences wrapped to (-180, 180]."""
    return -((-d + 180.0) % 360.0 - 180.0)


def electrical(angle, sens, off):
    """(angle + offset) * sensitivity, parameters broadcast over (channel[, ping_time])."""
    def bc(v):
        v = np.asarray(v, float)
        return v[:, None, None] if v.ndim == 1 else v[:, :, None]

    return (angle + bc(off)) * bc(sens)


def assert_complex_close(got, want, sens, off, weak, tol=1e-3, beam_types=None):
    """The comparison of complex-sample angles.

    The reference forms the angle from complex64 products (float32 atan2), the kernels from float32 / float64 ones:
    they cannot agree bit for bit.  The ELECTRICAL angle (theta + offset) * sensitivity is compared, because that is
    the phase of the product and its rounding error does not grow with 1 / sensitivity; the difference is wrapped to
    (-180, 180] because rounding can move a product that lies on the negative real axis from +180 to -180.  The phase
    of a * conj(b) computed from rounded a and b is off by about eps * (1/|a| + 1/|b|) * |rounding scale| radians: with
    the combination magnitudes at least 1e-3 of their ping's RMS (``weak`` False) and float32 rounding (eps = 6e-8
    relative to the ping's largest values, which are within ~10x of the RMS), that is below 1e-3 degrees.  Where a
    factor is smaller than that the phase is ill-conditioned (and an FFT's rounding noise can decide it), so only the
    NaN pattern is required to agree there.  The same holds for a three-sector type where a product lies on the
    negative real axis: theta = (fac1 + fac2) / sqrt 3 jumps by 360 / sqrt 3 between the two signs of a zero, which no
    wrap of the difference undoes (``weak`` marks those samples too)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want) & ~weak
    d = wrap(electrical(got, sens, off) - electrical(want, sens, off))
    assert ok.sum() > 0.5 * (~np.isnan(want)).sum(), "too few well-conditioned samples to compare"
    err = np.abs(d[ok]).max() if ok.any() else 0.0
    assert err <= tol, f"electrical angle differs by {err:.3g} deg (tolerance {tol})"


def _kernel_combos(beam_type):
    """The sector pairs the kernels filter (csrc/splitbeam.hip ``combo_sectors``: plain sums, no factor 1/2 -- a phase
    does not see it), in ``combinations``' order: list of (u, v) with v = None for a single sector."""
    if beam_type == 1:
        return [(2, 3), (0, 1), (0, 3), (1, 2)]
    if beam_type == 17:
        return [(2, None), (0, None), (1, None)]
    return [(2, 3), (0, 3), (1, 3)]


def complex_angle_bounds(re, im, beam_types, sa, st, oa, ot, replicas, replica_id=None, form="fft", max_taps=None,
                         u_f=2.0**-24, u_t=2.0**-53):
    """The float64 oracle angles of the pulse-compressed route on the float32 samples and the complex64-ROUNDED
    replicas the kernels read, with the derived per-sample bound of the electrical angles (tests/f32_bounds.py):
    per combination the amplitude bound of its filtered series -- the float add of its two sectors (u_f |c|) through
    the exact filter, plus ``fft_tile_bound`` of its 2048-sample tile (form "fft", transform precision u_f) or
    ``direct_form_bound`` (form "direct", accumulation in the output type, u_t), and the rounding of a wider
    transform's output to the output type -- then ``phase_bound_deg`` of the two products and ``splitbeam_angle_bound``.  -> (theta, phi, b_al, b_at, weak); ``weak`` is ``complex_angles``'."""
    import f32_bounds as fb

    reps = [np.asarray(r).astype(np.complex64).astype(np.complex128) for r in replicas]
    theta, phi, (e_al, e_at), weak = complex_angles(re, im, beam_types, sa, st, oa, ot, reps, replica_id)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    C, P, S, B = x.shape
    b_al, b_at = np.full((C, P, S), np.inf), np.full((C, P, S), np.inf)
    if max_taps is None:
        max_taps = max(r.size for r in reps)
    opt = fb.NFFT - max_taps + 1

    def bc(v, c):
        v = np.asarray(v, float)
        return v[c] if v.ndim == 1 else v[c][:, None]

    for c in range(C):
        bt = int(beam_types[c])
        if bt not in SUPPORTED:
            continue
        pairs = _kernel_combos(bt)
        yabs = np.zeros((len(pairs), P, S))
        dlt = np.zeros((len(pairs), P, S))
        for p in range(P):
            h = reps[c if replica_id is None else int(replica_id[c, p])]
            habs = np.abs(h)
            for k, (u, v) in enumerate(pairs):
                xz = np.where(np.isnan(x[c, p]), 0, x[c, p])
                ck = xz[:, u] + (xz[:, v] if v is not None else 0)
                d_add = (u_f if v is not None else 0.0) * np.abs(ck)
                yabs[k, p] = np.abs(np.convolve(np.concatenate([ck, np.zeros(h.size - 1)]), np.conj(h)[::-1], "valid"))
                d = np.convolve(np.concatenate([d_add, np.zeros(h.size - 1)]), habs[::-1], "valid")
                if form == "fft":
                    nt = -(-S // opt)
                    tiles = np.zeros((nt, fb.NFFT), np.complex128)
                    for t in range(nt):
                        seg = ck[t * opt:t * opt + fb.NFFT]
                        tiles[t, :seg.size] = seg * (1 + u_f)
                    tb = fb.fft_tile_bound(tiles, h, u_f)
                    d = d + np.repeat(tb, opt)[:S]
                else:
                    d = d + fb.direct_form_bound(ck * (1 + u_f), h, u_t)
                if u_t > u_f:   # the transform's output is rounded to the output type before the product (:574)
                    d = d + u_t * (yabs[k, p] + d)
                dlt[k, p] = d
        four = bt == 1
        b0 = fb.phase_bound_deg(yabs[0], dlt[0], yabs[1], dlt[1], u_t)
        b1 = fb.phase_bound_deg(yabs[2], dlt[2], yabs[3], dlt[3], u_t) if four else \
            fb.phase_bound_deg(yabs[0], dlt[0], yabs[2], dlt[2], u_t)
        b_al[c], b_at[c] = fb.splitbeam_angle_bound(b0, b1, e_al[c], e_at[c], four, bc(sa, c), bc(oa, c), bc(st, c),
                                                    bc(ot, c), u_t)
    return theta, phi, b_al, b_at, weak


def assert_complex_bound(got, want, sens, off, weak, bound, cap, what=""):
    """The electrical angle against the oracle's with the derived per-sample ``bound``, ``cap`` (the old flat
    tolerance) on top of it: |difference| <= min(bound, cap) at every sample ``assert_complex_close`` compares.
    Returns (largest ratio, share of the compared samples at which the DERIVED bound is the smaller of the two, i.e.
    governs); the share is logged with the ratio.  For a complex64 transform the derived bound is the tile's normwise
    bound taken per sample and governs only the strongest few per cent of the samples (the cap judges the rest); for a
    complex128 transform and for the direct form it governs everywhere."""
    import f32_bounds as fb

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want) & ~weak
    assert ok.sum() > 0.5 * (~np.isnan(want)).sum(), "too few well-conditioned samples to compare"
    d = np.abs(wrap(electrical(got, sens, off) - electrical(want, sens, off)))[ok]
    tol = np.minimum(bound[ok], cap)
    ratio = d / tol
    k = int(np.argmax(ratio))
    assert ratio[k] <= 1.0, f"{what}: electrical angle differs by {d[k]:.3g} deg (bound {bound[ok][k]:.3g}, cap {cap})"
    gov = bound[ok] <= cap
    fb._log(f"{what}: electrical angle", float(d.max()), float(ratio.max()), want.shape, governed=float(gov.mean()),
            max_ratio_where_governed=float(ratio[gov].max()) if gov.any() else 0.0,
            bound_median_deg=float(np.median(bound[ok])))
    return float(ratio.max()), float(gov.mean())
