"""The rules of calibrate.compute_Sv_spectrum (echopype_amd/calibrate/sv_spectrum.py states them) restated in NumPy
float64 as plain loops over ping, cell and frequency: the judge of csrc/sv_spectrum.hip.  Nothing here shares code with
the package, and nothing follows the kernel's order of summation: every sector is compressed on its own, sample by
sample, and every Fourier sum is one ``sum`` over explicitly formed terms.

``sv_spectrum`` also returns the conditioning kappa = sum |terms| / |sum| of the Fourier sums Y (per cell and frequency)
and A (per replica and frequency): the rounding of a sum of n terms is about n * 2**-53 * kappa relative."""
import numpy as np

FPARAMS = ("frequency", "sound_absorption", "gain_correction", "impedance_transducer", "equivalent_beam_angle")
PPARAMS = ("transmit_power", "sound_speed", "impedance_transceiver", "sample_interval")


def n_cells(S, Nw, hop):
    return (S - Nw) // hop + 1


def window(Nw, kind="hann"):
    """Rule 4: the normalised window, sum w~^2 = Nw."""
    if kind == "hann":
        w = np.array([0.5 * (1.0 - np.cos(2.0 * np.pi * k / (Nw - 1))) for k in range(Nw)])
    else:
        assert kind == "rectangular"
        w = np.ones(Nw)
    return w / np.sqrt(np.sum(w ** 2) / Nw)


def compress_row(re, im, tx):
    """Rules 1 and 2 for one ping: re, im (S, B); tx complex (L,).  -> (pc complex (S,), valid bool (S,))."""
    S, B = re.shape
    L = tx.size
    E = float(np.sum(np.abs(tx.astype(np.complex128)) ** 2))
    ok = ~np.isnan(re) & ~np.isnan(im)
    z = np.where(ok, re.astype(np.float64) + 1j * im.astype(np.float64), 0.0)
    ctx = np.conj(tx.astype(np.complex128))
    pc = np.zeros(S, dtype=np.complex128)
    for n in range(S):
        if not ok[n].any():
            continue
        m = min(L, S - n)
        acc = 0.0
        for b in np.flatnonzero(ok[n]):
            acc = acc + np.sum(z[n:n + m, b] * ctx[:m]) / E
        pc[n] = acc / ok[n].sum()
    return pc, ok.any(axis=1)


def replica_spectrum(tx, dt, Nw, f):
    """Rule 6: A(f) complex (F,) and its conditioning."""
    t = tx.astype(np.complex128)
    L = t.size
    E = float(np.sum(np.abs(t) ** 2))
    hh = min((Nw - 1) // 2, L - 1)
    f = np.asarray(f, dtype=np.float64)
    A = np.zeros(f.shape, dtype=np.complex128)
    mag = np.zeros(f.shape)
    for j in range(-hh, hh + 1):
        if j >= 0:
            a = np.sum(t[j:] * np.conj(t[:L - j])) / E
        else:
            a = np.sum(t[:L + j] * np.conj(t[-j:])) / E
        term = a * np.exp(-2j * np.pi * f * j * dt)
        A += term
        mag += np.abs(term)
    with np.errstate(divide="ignore", invalid="ignore"):
        return A, mag / np.abs(A)


def sv_spectrum(re, im, replicas, replica_id, rep_dt, fparams, pparams, Nw, hop, kind="hann", compressed=None):
    """re, im (C, P, S, B); replicas: list of complex arrays; replica_id (C, P) int or None (replica c); rep_dt (R,);
    fparams (R, 5, F) in the order FPARAMS; pparams (4, C, P) in the order PPARAMS.  ``compressed``: optionally a dict
    that keeps ``compress_row`` per (c, p, replica) between calls on the same cubes.
    -> dict(Sv_spectrum (C, P, M, F), echo_range (C, P, M), kappa_Y (C, P, M, F), kappa_A (R, F)), float64."""
    C, P, S, B = re.shape
    R, _, F = fparams.shape
    M = n_cells(S, Nw, hop)
    sv = np.full((C, P, M, F), np.nan)
    rng = np.full((C, P, M), np.nan)
    kY = np.full((C, P, M, F), np.nan)
    kA = np.full((R, F), np.nan)
    A_of = {}
    for r in range(min(R, len(replicas))):
        A_of[r], kA[r] = replica_spectrum(np.asarray(replicas[r]), rep_dt[r], Nw, fparams[r, 0])
    wt = window(Nw, kind)
    k = np.arange(Nw)
    for c in range(C):
        for p in range(P):
            p_t, c_w, z_er, dt = (float(pparams[i, c, p]) for i in range(4))
            r_of = lambda n: n * dt * c_w / 2  # noqa: E731
            for m in range(M):
                rng[c, p, m] = (r_of(m * hop) + r_of(m * hop + Nw - 1)) / 2
            rid = c if replica_id is None else int(replica_id[c, p])
            if not (0 <= rid < R):
                continue
            key = (c, p, rid)
            if compressed is not None and key in compressed:
                pc, valid = compressed[key]
            else:
                pc, valid = compress_row(re[c, p], im[c, p], np.asarray(replicas[rid]))
                if compressed is not None:
                    compressed[key] = (pc, valid)
            ps = np.arange(S) * dt * c_w / 2 * pc
            f, alpha, G, z_et, psi = fparams[rid]
            for m in range(M):
                n0 = m * hop
                r_m = rng[c, p, m]
                if not valid[n0:n0 + Nw].all() or not r_m > 0:
                    continue
                terms = (wt * ps[n0:n0 + Nw])[None, :] * np.exp(-2j * np.pi * f[:, None] * k[None, :] * dt)
                Y = terms.sum(axis=1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    kY[c, p, m] = np.abs(terms).sum(axis=1) / np.abs(Y)
                    prx = B * np.abs(Y / A_of[rid]) ** 2 / 8 * (np.abs(z_er + z_et) / z_er) ** 2 / z_et
                    prx = np.where((prx > 0) & np.isfinite(prx), prx, np.nan)
                    lam = c_w / f
                    sv[c, p, m] = 10 * np.log10(prx) + 2 * alpha * r_m \
                        - 10 * np.log10(p_t * lam ** 2 * c_w / (32 * np.pi ** 2)) - 2 * G - 10 * np.log10(Nw * dt) - psi
    return dict(Sv_spectrum=sv, echo_range=rng, kappa_Y=kY, kappa_A=kA)
