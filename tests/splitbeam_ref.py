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
