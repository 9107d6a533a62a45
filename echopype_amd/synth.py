"""Seeded synthetic echograms of the BASELINE.json shapes (SURVEY.md 8d recipe).

Two flavours of the same recipe:
  * ``ek60_numpy`` / ``ek80_numpy`` / ``azfp_numpy`` -- host arrays for the parity tests (the
    oracle and the HIP path consume the same arrays);
  * ``ek60_device`` -- generated directly in HBM with torch for the full-size bench volumes
    (16-130 GB never cross PCIe).
Raw EK60 power: float32(int16 ~ U[-12000, -2000]) * float32(10*log10(2)/256)
(convert/parse_base.py:24,302); 10 % of pings carry a NaN tail over the last 5 % of the range.
"""
import numpy as np

INDEX2POWER = np.float32(10.0 * np.log10(2.0) / 256.0)

EK60_FREQ = np.array([18e3, 38e3, 120e3, 200e3])
EK60_PT = np.array([2000.0, 2000.0, 250.0, 150.0])
EK60_G = np.array([22.9, 26.5, 27.0, 27.0])
EK60_PSI = np.array([-17.0, -20.6, -20.4, -20.2])
PULSE_LENGTHS = np.array([256e-6, 512e-6, 1024e-6, 2048e-6, 4096e-6])
T0 = np.datetime64("2026-05-01T00:00:00", "ns")


def fg_absorption(f_hz, T=10.0, S=35.0, P=10.0, pH=8.0):
    """Francois & Garrison absorption [dB/m] for the synthetic Environment group (host prep)."""
    from .utils.uwa import calc_absorption

    return calc_absorption(frequency=f_hz, temperature=T, salinity=S, pressure=P, pH=pH,
                           formula_source="FG")


def _channels(C):
    if C == 2:
        return np.array([1, 2])  # 38 / 120 kHz (cfg1)
    if C <= 4:
        return np.arange(C)
    return np.arange(C) % 4


def ek60_params(C, P, vary_tau=False, seed=0, ping0=0, ss_every=1):
    """Per-channel / per-ping parameters of the synthetic EK60 file (host, O(C*P)).  ``ping0``: global index of
    the first ping when the arrays are a ping shard / tile of a longer file (ping times and the sound-speed drift
    follow the global index).  ``ss_every``: the sound speed an EK60 records with every ping is the operator's
    setting -- it follows the slow drift in steps of this many pings (1: a new value every ping, the hardest case
    for the kernels that cache per-range-column terms)."""
    ch = _channels(C)
    p = np.arange(P) + ping0
    si = np.full((C, P), 2.56e-4)
    tau = np.full((C, P), 1.024e-3)
    if vary_tau:  # exercise the pulse-length table lookup (+ a NaN ping)
        rng = np.random.default_rng(seed + 99)
        tau = PULSE_LENGTHS[rng.integers(0, 5, size=(C, P))]
        tau[:, 0] = 1.024e-3
    ss = np.tile(1500.0 + 0.5 * np.sin(2 * np.pi * (p // ss_every * ss_every) / 1e5), (C, 1))
    g = EK60_G[ch]
    return dict(
        channel=[f"GPT {int(EK60_FREQ[i] / 1e3)} kHz 00907205{i:04d} 1 ES{int(EK60_FREQ[i] / 1e3)}" for i in ch],
        frequency_nominal=EK60_FREQ[ch].copy(),
        sample_interval=si,
        transmit_duration_nominal=tau,
        transmit_power=np.tile(EK60_PT[ch][:, None], (1, P)),
        sound_speed_indicative=ss,
        absorption_indicative=np.tile(fg_absorption(EK60_FREQ[ch])[:, None], (1, P)),
        equivalent_beam_angle=EK60_PSI[ch].copy(),
        pulse_length=np.tile(PULSE_LENGTHS, (C, 1)),
        gain_correction=np.stack([g - 1.0, g - 0.5, g, g + 0.2, g + 0.3], axis=1),
        sa_correction=np.tile(np.array([-0.7, -0.6, -0.5, -0.3, -0.3]), (C, 1)),
        ping_time=T0 + (p * 1_000_000_000).astype("timedelta64[ns]"),
    )


def ek60_numpy(C=2, P=200, S=1000, seed=20260501, vary_tau=False, ss_every=1):
    """Host arrays: backscatter_r f32 (C,P,S) + params."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(-12000, -2000, size=(C, P, S), dtype=np.int16).astype(np.float32) * INDEX2POWER
    nan_pings = rng.random(P) < 0.10
    tail = max(1, int(round(0.05 * S)))
    raw[:, nan_pings, S - tail:] = np.nan
    d = ek60_params(C, P, vary_tau=vary_tau, seed=seed, ss_every=ss_every)
    d["backscatter_r"] = raw
    return d


def ek60_device(C, P, S, seed=20260501, device=None, chunk_pings=20000, ping0=0, ss_every=2000):
    """Same recipe generated in HBM: returns dict of torch CUDA tensors (raw f32 + f64 params).  The recorded sound
    speed changes every ``ss_every`` pings (see :func:`ek60_params`)."""
    import torch

    dev = device or torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    raw = torch.empty((C, P, S), dtype=torch.float32, device=dev)
    tail = max(1, int(round(0.05 * S)))
    for c in range(C):
        for p0 in range(0, P, chunk_pings):
            p1 = min(P, p0 + chunk_pings)
            blk = torch.randint(-12000, -2000, (p1 - p0, S), generator=g, device=dev, dtype=torch.int16)
            raw[c, p0:p1] = blk.to(torch.float32) * float(INDEX2POWER)
            del blk
    nan_pings = torch.rand(P, generator=g, device=dev) < 0.10
    idx = torch.nonzero(nan_pings).flatten()
    raw[:, idx, S - tail:] = float("nan")
    h = ek60_params(C, P, ping0=ping0, ss_every=ss_every)
    out = {"backscatter_r": raw}
    for k in ("sample_interval", "transmit_duration_nominal", "transmit_power", "sound_speed_indicative",
              "absorption_indicative", "equivalent_beam_angle", "frequency_nominal", "pulse_length",
              "gain_correction", "sa_correction"):
        out[k] = torch.from_numpy(np.ascontiguousarray(h[k], dtype=np.float64)).to(dev)
    out["ping_time_ns"] = torch.from_numpy(h["ping_time"].astype(np.int64)).to(dev)
    out["ping_time"] = h["ping_time"]
    out["channel"] = h["channel"]
    return out


def ek60_device_i16(C, P, S, seed=20260501, device=None, chunk_pings=20000, ss_every=2000):
    """The same recipe as :func:`ek60_device` before the converter's float conversion: int16 power
    samples (C,P,S) + the recorded length of every ping (C,P) int32."""
    import torch

    dev = device or torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    raw = torch.empty((C, P, S), dtype=torch.int16, device=dev)
    for c in range(C):
        for p0 in range(0, P, chunk_pings):
            p1 = min(P, p0 + chunk_pings)
            raw[c, p0:p1] = torch.randint(-12000, -2000, (p1 - p0, S), generator=g, device=dev, dtype=torch.int16)
    short = torch.rand(P, generator=g, device=dev) < 0.10
    n_valid = torch.full((C, P), S, dtype=torch.int32, device=dev)
    n_valid[:, short] = S - max(1, int(round(0.05 * S)))
    h = ek60_params(C, P, ss_every=ss_every)
    out = {"raw_i16": raw, "n_valid": n_valid}
    for k in ("sample_interval", "transmit_duration_nominal", "transmit_power", "sound_speed_indicative",
              "absorption_indicative", "equivalent_beam_angle", "frequency_nominal", "pulse_length",
              "gain_correction", "sa_correction"):
        out[k] = torch.from_numpy(np.ascontiguousarray(h[k], dtype=np.float64)).to(dev)
    out["ping_time_ns"] = torch.from_numpy(h["ping_time"].astype(np.int64)).to(dev)
    out["ping_time"] = h["ping_time"]
    return out


# ---------------------------------------------------------------------------------------- EK80
def ek80_filters(seed=20260501):
    """Deterministic stand-ins for the Vendor_specific WBT/PC filter coefficients (complex64)."""
    k47, k91 = np.arange(47), np.arange(91)
    wbt = (np.hanning(47) * np.exp(2j * np.pi * 0.045 * k47) / 10).astype(np.complex64)
    pc = (np.hanning(91) * np.exp(2j * np.pi * 0.13 * k91) / 20).astype(np.complex64)
    return dict(wbt_fil=wbt, wbt_decifac=6, pc_fil=pc, pc_decifac=2)


EK80_BB = dict(
    frequency_nominal=np.array([70e3, 120e3]),
    f_start=np.array([45e3, 90e3]),
    f_stop=np.array([90e3, 170e3]),
    tau=np.array([1.024e-3, 0.512e-3]),
    transmit_power=np.array([750.0, 250.0]),
    z_er=np.array([5400.0, 5400.0]),
    z_et=np.array([75.0, 75.0]),
    psi=np.array([-20.7, -20.7]),
    gain=np.array([27.0, 26.8]),
    sa=np.array([-0.1, -0.05]),
    angle_offset_alongship=np.array([0.05, -0.03]),
    angle_offset_athwartship=np.array([-0.02, 0.04]),
    beamwidth_alongship=np.array([6.8, 6.6]),
    beamwidth_athwartship=np.array([6.9, 6.5]),
)


def ek80_numpy(C=2, P=16, S=1024, B=4, seed=20260504, waveform="BB", replicas=None,
               mixed_nan=False):
    """Host arrays for EK80 complex data: backscatter_r/_i f64 (C,P,S,B) + params.

    Complex noise N(0,1)+iN(0,1) * 1e-3 plus replica-shaped echoes at 3 random ranges per ping,
    NaN tail on ~10 % of pings, optional per-sector (mixed) NaNs to exercise the per-sector path.
    """
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((C, P, S, B)) + 1j * rng.standard_normal((C, P, S, B))) * 1e-3
    if replicas is not None:
        for c in range(C):
            r = replicas[c]
            for p in range(P):
                for start in rng.integers(0, max(1, S - 8), size=3):
                    n = min(r.size, S - start)
                    amp = 0.2 + 0.6 * rng.random()
                    x[c, p, start:start + n, :] += amp * r[:n, None] * np.exp(1j * rng.random(B))[None, :]
    re = np.ascontiguousarray(x.real, dtype=np.float64)
    im = np.ascontiguousarray(x.imag, dtype=np.float64)
    nan_pings = rng.random(P) < 0.10
    nan_pings[min(1, P - 1)] = True
    tail = max(1, int(round(0.05 * S)))
    re[:, nan_pings, S - tail:, :] = np.nan
    im[:, nan_pings, S - tail:, :] = np.nan
    if mixed_nan:
        re[0, 0, S // 3: S // 3 + 5, 1] = np.nan
        im[0, 0, S // 3: S // 3 + 5, 1] = np.nan
        im[C - 1, P - 1, 10, B - 1] = np.nan   # imag-only NaN (convert sets imag 0 -> NaN)
        re[C - 1, P - 1, 17, :] = np.nan       # whole sample NaN in the middle of a ping
        im[C - 1, P - 1, 17, :] = np.nan
        # beam 0 missing, the other sectors valid: echo_range is masked there (range.py:143-148), hence Sv NaN
        re[0, min(1, P - 1), S // 2: S // 2 + 3, 0] = np.nan
    p = np.arange(P)
    d = dict(EK80_BB)
    d = {k: (v[:C].copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    d.update(
        backscatter_r=re, backscatter_i=im,
        channel=[f"WBT 4000{i}-15 ES{int(d['frequency_nominal'][i] / 1e3)}-7C" for i in range(C)],
        sample_interval=np.full((C, P), 8e-6),
        sound_speed=np.tile(1500.0 + 0.5 * np.sin(2 * np.pi * p / 1e5), (C, 1)),
        slope=np.full(C, 0.05), fs=np.full(C, 1.5e6),
        ping_time=T0 + (p * 1_000_000_000).astype("timedelta64[ns]"),
        waveform=waveform,
    )
    return d



# ---------------------------------------------------------------------------------------- split-beam angles
# (consolidate.add_splitbeam_angle; new generators with their own seeds: the ones above are untouched)
def splitbeam_sector_phases(e_along, e_athw, beam_type):
    """Complex sector values (..., 4) whose combinations (consolidate/split_beam_angle.py:34-118) give the electrical
    angles ``e_along`` / ``e_athw`` (degrees, arrays of one shape) exactly in exact arithmetic:
      beam_type 1:  b_k = exp(i (s_k a + t_k b) / 2) with s = (-1, -1, 1, 1) (aft / fore), t = (1, -1, -1, 1)
                    (star / port): fore conj(aft) = 4 cos^2(b/2) e^{ia}, star conj(port) = 4 cos^2(a/2) e^{ib};
      17:           star = e^{-i fac1}, port = e^{-i fac2}, fore = 1 with fac1 = (sqrt3 a - b)/2, fac2 = (sqrt3 a + b)/2;
      49/65/81:     the same three combinations, each written as (sector + centre) around a centre element q.
    Unit magnitudes; the caller scales them."""
    a, b = np.deg2rad(np.asarray(e_along, float)), np.deg2rad(np.asarray(e_athw, float))
    out = np.zeros(a.shape + (4,), dtype=np.complex128)
    if beam_type == 1:
        for k, (sk, tk) in enumerate(((-1, 1), (-1, -1), (1, -1), (1, 1))):
            out[..., k] = np.exp(0.5j * (sk * a + tk * b))
        return out
    fac1, fac2 = (np.sqrt(3) * a - b) / 2, (np.sqrt(3) * a + b) / 2
    star, port, fore = np.exp(-1j * fac1), np.exp(-1j * fac2), np.ones_like(a, dtype=np.complex128)
    if beam_type == 17:
        out[..., 0], out[..., 1], out[..., 2] = star, port, fore
        return out
    q = 0.3 * np.exp(0.7j) * np.ones_like(a)  # the centre element
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = star - q, port - q, fore - q, q
    return out


def ek80_splitbeam_numpy(C=2, P=8, S=600, B=4, beam_type=1, seed=20261015, waveform="BB", sens=(23.0, 21.5),
                         offset=(0.05, -0.03)):
    """An EK80 complex data set whose samples are a split-beam target of KNOWN angles: ``ek80_numpy``'s dictionary
    (its own stream, unchanged) with the samples replaced by sector values of splitbeam_sector_phases -- a physical
    alongship / athwartship angle per (channel, ping, sample) drawn in +-(150 / sens) degrees, magnitudes in
    [0.5, 1.5) -- plus ``beam_type`` and the angle parameters.  Returns (d, theta, phi) with the angles the samples
    encode, float64 (C, P, S).  ``beam_type``: one int for every channel, or a sequence of C."""
    d = ek80_numpy(C=C, P=P, S=S, B=B, seed=seed, waveform=waveform)
    rng = np.random.default_rng(seed + 7)
    bts = np.broadcast_to(np.asarray(beam_type), (C,)).astype(np.int64)
    sens_al = np.broadcast_to(np.asarray(sens[0], float), (C,)).copy()
    sens_at = np.broadcast_to(np.asarray(sens[1], float), (C,)).copy()
    off_al = np.broadcast_to(np.asarray(offset[0], float), (C,)).copy()
    off_at = np.broadcast_to(np.asarray(offset[1], float), (C,)).copy()
    theta = np.empty((C, P, S))
    phi = np.empty((C, P, S))
    x = np.empty((C, P, S, B), dtype=np.complex128)
    for c in range(C):
        lim = 150.0 / max(sens_al[c], sens_at[c])
        theta[c] = rng.uniform(-lim, lim, (P, S))
        phi[c] = rng.uniform(-lim, lim, (P, S))
        e_al, e_at = (theta[c] + off_al[c]) * sens_al[c], (phi[c] + off_at[c]) * sens_at[c]
        if bts[c] != 1:  # three-sector types: theta / phi come from fac1 +- fac2, keep both inside (-180, 180)
            e_al = e_al * 0.5
            e_at = e_at * 0.5
            theta[c], phi[c] = e_al / sens_al[c] - off_al[c], e_at / sens_at[c] - off_at[c]
        sec = splitbeam_sector_phases(e_al, e_at, int(bts[c]) if bts[c] in (1, 17, 49, 65, 81) else 1)
        amp = 0.5 + rng.random((P, S, 1))
        x[c] = (amp * sec)[..., :B]
    d["backscatter_r"] = np.ascontiguousarray(x.real)
    d["backscatter_i"] = np.ascontiguousarray(x.imag)
    d["beam_type"] = bts
    d["angle_sensitivity_alongship"], d["angle_sensitivity_athwartship"] = sens_al, sens_at
    d["angle_offset_alongship"], d["angle_offset_athwartship"] = off_al, off_at
    return d, theta, phi


def splitbeam_nan_pad(d, pings, tail, single_sector=None):
    """NaN-padded short pings (the last ``tail`` samples of ``pings``, every sector, as the converter pads them) and,
    optionally, ``single_sector`` = (c, p, s, b): one sector NaN at one sample (re and im).  In place; returns d."""
    for k in ("backscatter_r", "backscatter_i"):
        d[k][:, list(pings), d[k].shape[2] - tail:, :] = np.nan
        if single_sector is not None:
            c, p, s_, b = single_sector
            d[k][c, p, s_, b] = np.nan
    return d


def ek60_splitbeam_numpy(C=2, P=40, S=400, seed=20261016, nan_pad=False, sens=(21.9, 23.1), offset=(0.02, -0.07)):
    """``ek60_numpy`` (its own stream, unchanged) plus split-beam angle planes: int8 electrical-angle steps as parsed
    (convert/utils/ek_raw_parsers.py:1705-1743), or -- ``nan_pad`` -- float32 planes whose short pings end in NaN (what
    a NaN-padded file holds, convert/parse_base.py:688); ``beam_type`` 1 and the angle parameters per channel."""
    d = ek60_numpy(C, P, S, seed=seed)
    rng = np.random.default_rng(seed + 11)
    for k in ("angle_alongship", "angle_athwartship"):
        a = rng.integers(-128, 128, (C, P, S)).astype(np.int8)
        if nan_pad:
            a = a.astype(np.float32)
            short = rng.random(P) < 0.2
            short[0] = True
            a[:, short, S - S // 7:] = np.nan
        d[k] = a
    d["beam_type"] = np.ones(C, dtype=np.int64)
    d["angle_sensitivity_alongship"] = np.broadcast_to(np.asarray(sens[0], float), (C,)).copy()
    d["angle_sensitivity_athwartship"] = np.broadcast_to(np.asarray(sens[1], float), (C,)).copy()
    d["angle_offset_alongship"] = np.broadcast_to(np.asarray(offset[0], float), (C,)).copy()
    d["angle_offset_athwartship"] = np.broadcast_to(np.asarray(offset[1], float), (C,)).copy()
    return d

# ---------------------------------------------------------------------------------------- AZFP
def azfp_numpy(C=4, P=60, S=500, seed=20260507):
    rng = np.random.default_rng(seed)
    counts = rng.integers(2000, 60000, size=(C, P, S)).astype(np.float32)
    f = np.array([38e3, 125e3, 200e3, 455e3])[:C]
    p = np.arange(P)
    return dict(
        backscatter_r=counts, frequency_nominal=f,
        channel=[f"55030-{int(x / 1e3)}-1" for x in f],
        transmit_duration_nominal=np.tile(np.array([5e-4, 3e-4, 3e-4, 1.5e-4])[:C, None], (1, P)),
        number_of_samples_per_average_bin=np.array([20.0, 10.0, 10.0, 5.0])[:C],
        digitization_rate=np.full(C, 64000.0), lock_out_index=np.array([0.0, 2.0, 2.0, 4.0])[:C],
        EL=np.array([142.8, 144.0, 141.5, 140.3])[:C], DS=np.array([0.02293, 0.02243, 0.02273, 0.02293])[:C],
        TVR=np.array([169.9, 170.3, 172.6, 175.5])[:C], VTX0=np.array([105.2, 117.8, 110.1, 63.8])[:C],
        Sv_offset=np.array([1.1, 1.4, 1.4, 1.3])[:C],
        equivalent_beam_angle=10 ** (np.array([-11.8, -18.3, -18.5, -18.6])[:C] / 10),
        temperature=np.full(P, 8.5), salinity=29.6, pressure=60.0,
        ping_time=T0 + (p * 3_000_000_000).astype("timedelta64[ns]"),
    )


# ------------------------------------------------------------------------------------- seafloor scenes (mask.detect_seafloor)
def seafloor_scene(P=120, S=160, seed=20261017, dtype=np.float64, dz=0.5, band_top=110, slope=-0.1, thickness=6,
                   band_angle=(8.0, -6.0), noise_angle=2.0, nan_pad=True):
    """One channel's (ping_time, range_sample) planes of a seabed scene -> dict sv, theta, phi, depth (P, S):
    - a sloped bottom band (Sv about -25 dB) whose angles are coherent (``band_angle`` + small noise);
    - a fish school above it (bright Sv, zero-mean noisy angles);
    - a chain of single pixels linked only diagonally, from the band's top up to a bright patch far above it (kept only
      under 8-connectivity: the angle mask reaches neither the patch nor the chain's upper part);
    - a bright patch that touches nothing;
    - NaN padding at the end of every seventh ping (Sv and angles; depth stays uniform).
    Background Sv about -90 dB, angles zero-mean with ``noise_angle`` spread.  ``band_top`` / ``slope``: first band
    sample of ping 0 and its drift in samples per ping."""
    rng = np.random.default_rng(seed)
    sv = -90.0 + 3.0 * rng.standard_normal((P, S))
    theta = noise_angle * rng.standard_normal((P, S))
    phi = noise_angle * rng.standard_normal((P, S))
    top = np.clip(np.round(band_top + slope * np.arange(P)).astype(int), 0, S - thickness)
    for p in range(P):
        b = slice(top[p], top[p] + thickness)
        sv[p, b] = -25.0 + rng.standard_normal(thickness)
        theta[p, b] = band_angle[0] + 0.05 * rng.standard_normal(thickness)
        phi[p, b] = band_angle[1] + 0.05 * rng.standard_normal(thickness)
    # fish school: pings P/8 .. 3P/8, samples S/8 .. S/4
    sv[P // 8:3 * P // 8, S // 8:S // 4] = -45.0 + 2.0 * rng.standard_normal((3 * P // 8 - P // 8, S // 4 - S // 8))
    # diagonal chain up and forward from the band top at ping pc, then a 3 x 3 patch at its end
    pc = P // 2
    n_chain = min(40, top[pc] - 8, P - pc - 6)
    for j in range(1, n_chain + 1):
        sv[pc + j, top[pc] - j] = -30.0
        # keep the chain diagonal-only: its 4-neighbours off the band are background
        for (a, b) in ((pc + j - 1, top[pc] - j), (pc + j, top[pc] - j + 1)):
            if b < top[a]:
                sv[a, b] = -90.0
    pe, re = pc + n_chain, top[pc] - n_chain
    sv[pe + 1:pe + 4, re - 3:re] = -30.0  # the patch: diagonal to the chain's last pixel (pe, re)
    sv[pe + 1:pe + 4, re] = -90.0
    sv[pe, re - 3:re] = -90.0
    # a patch that touches nothing, high above the band
    q = 3 * P // 4
    sv[q:q + 4, S // 16:S // 16 + 4] = -28.0
    depth = np.tile(np.arange(S) * dz, (P, 1))
    if nan_pad:
        for p in range(3, P, 7):
            sv[p, S - S // 9:] = np.nan
            theta[p, S - S // 9:] = np.nan
            phi[p, S - S // 9:] = np.nan
    return {"sv": sv.astype(dtype), "theta": theta.astype(dtype), "phi": phi.astype(dtype), "depth": depth.astype(dtype),
            "top": top}


def ek60_seafloor_numpy(C=2, P=96, S=400, seed=20261018, band_top=300, slope=-0.5, thickness=8):
    """``ek60_splitbeam_numpy`` (its own streams, unchanged) with a seabed written into the raw samples of every
    channel: a sloped band of strong power whose int8 electrical-angle steps are coherent (+40 / -30 steps), over
    the generator's noise (random steps elsewhere).  For the whole chain from_ek60_arrays -> compute_Sv -> add_depth
    -> add_splitbeam_angle -> detect_seafloor."""
    d = ek60_splitbeam_numpy(C, P, S, seed=seed)
    # the operator's sound speed held for the whole file: the depth grid is the same in every ping (the detectors
    # refuse a grid that varies)
    d["sound_speed_indicative"] = np.repeat(d["sound_speed_indicative"][:, :1], P, axis=1)
    rng = np.random.default_rng(seed + 5)
    top = np.clip(np.round(band_top + slope * np.arange(P)).astype(int), 0, S - thickness)
    power = np.array(d["backscatter_r"], copy=True)
    al = np.array(d["angle_alongship"], copy=True)
    at = np.array(d["angle_athwartship"], copy=True)
    hi = float(np.nanmax(power)) + 30.0
    for p in range(P):
        b = slice(top[p], top[p] + thickness)
        power[:, p, b] = (hi + rng.standard_normal((C, thickness))).astype(power.dtype)
        al[:, p, b] = 40
        at[:, p, b] = -30
    d["backscatter_r"], d["angle_alongship"], d["angle_athwartship"] = power, al, at
    d["seafloor_top"] = top
    return d


def shoal_scene(P=90, S=120, seed=20261016, dtype=np.float64, schools=6, nan_frac=0.03, speckle=0.02):
    """One channel's (ping_time, range_sample) Sv plane of a school scene:
    - ``schools`` smooth blobs (Gaussian bumps of random centre and radii) reaching about -50 dB, with soft edges, so a
      -70 dB threshold cuts ragged outlines with small satellites and holes;
    - background about -85 dB with a spread of 4 dB, and ``speckle`` of the pixels raised to about -62 dB (single-pixel
      candidates and short gaps inside the blobs' fringes);
    - ``nan_frac`` of the pixels NaN."""
    rng = np.random.default_rng(seed)
    pp, ss = np.meshgrid(np.arange(P, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    sv = -85.0 + 4.0 * rng.standard_normal((P, S))
    for _ in range(schools):
        cp, cs = rng.uniform(0, P), rng.uniform(0, S)
        rp, rs = rng.uniform(0.03, 0.12) * P + 1.5, rng.uniform(0.03, 0.12) * S + 1.5
        bump = np.exp(-0.5 * (((pp - cp) / rp) ** 2 + ((ss - cs) / rs) ** 2))
        sv = np.maximum(sv, -95.0 + 45.0 * bump + 3.0 * rng.standard_normal((P, S)))
    spk = rng.random((P, S)) < speckle
    sv[spk] = -62.0 + 2.0 * rng.standard_normal(int(spk.sum()))
    sv[rng.random((P, S)) < nan_frac] = np.nan
    return sv.astype(dtype)


def transient_scene(P=200, S=300, seed=20261019, dtype=np.float64, dz=2.5, elevated=6, elevation=(6.0, 15.0),
                    nan_frac=0.02, sigma=2.0, bottom_frac=(0.85, 0.97)):
    """One channel's water column with transient noise, as a dict of NumPy arrays:
    - ``Sv`` (P, S): a noisy background (-78 dB at the surface falling 6 dB to the last sample, spread ``sigma`` dB),
      ``elevated`` pings raised by ``elevation[0] .. elevation[1]`` dB from a start row of their own (``tops``) down to
      the end of the column, ``nan_frac`` of the samples NaN, and a seafloor echo of about -25 dB under ``bottom``;
    - ``depth`` (S,): ``dz * arange(S)``, of ``dtype``;
    - ``bottom`` (P,) float64: a line sloping from ``bottom_frac[0]`` to ``bottom_frac[1]`` of the last depth;
    - ``pings`` / ``tops`` / ``gains``: the elevated pings, their start rows and elevations."""
    rng = np.random.default_rng(seed)
    depth = dz * np.arange(S, dtype=np.float64)
    sv = -78.0 - 6.0 * (np.arange(S) / max(S - 1, 1))[None, :] + sigma * rng.standard_normal((P, S))
    k = min(int(elevated), P)
    pings = np.sort(rng.choice(P, size=k, replace=False))
    tops = rng.integers(S // 8, max(S // 8 + 1, (3 * S) // 5), size=k)
    gains = rng.uniform(elevation[0], elevation[1], size=k)
    for j, t, e in zip(pings, tops, gains):
        sv[j, t:] += e
    bottom = np.linspace(bottom_frac[0], bottom_frac[1], P) * (depth[-1] if S else 0.0)
    under = depth[None, :] >= bottom[:, None]
    sv[under] = -25.0 + 1.5 * rng.standard_normal(int(under.sum()))
    sv[rng.random((P, S)) < nan_frac] = np.nan
    return {"Sv": sv.astype(dtype), "depth": depth.astype(dtype), "bottom": bottom, "pings": pings, "tops": tops,
            "gains": gains}


def single_target_scene(P=37, S=257, seed=20261020, dtype=np.float64, seam=1024, density=0.6, floor=-75.0, dr=0.2,
                        scale=1):
    """One channel's (ping_time, range_sample) planes for the single-target detector, as a dict of NumPy arrays:
    ``TS``, ``angle_alongship``, ``angle_athwartship`` (P, S) of ``dtype`` and ``echo_range`` (S,) = ``dr * arange(S)``.
    - a noise floor around ``floor`` dB (spread 3 dB: well below a -50 dB threshold) with angles scattered over +-5
      degrees; a row of fewer than 16 samples is instead one echo throughout: samples within 5 dB of each other
      below a level between -52 and -35 dB, one beam position, twice the angle jitter below, 5 % of the samples NaN;
    - the row is cut into slots of 16 samples, and a slot carries an echo with probability ``density``: mostly echoes
      parabolic in dB, of a half-width (at 6 dB) between 0.6 and 4.5 samples about a centre between two samples, peak
      between -55 and -30 dB, at a random position in the beam (out to 4.5 degrees off axis) and with an angle jitter
      of 0.05, 0.3 or 0.9 degrees from sample to sample; and, planted because random echoes almost never make them:
      overlapping pairs (a weaker peak inside the envelope of a stronger one), plateaus of two equal samples, and
      echoes with a NaN inside the envelope (in TS, or in one of the angles);
    - every fourth ping starts with an echo whose peak is sample 0, the next with one whose envelope starts there; the
      two after that end the row likewise;
    - every third ping carries an echo across each multiple of ``seam`` (the tile length of the kernel), its peak
      alternately on the sample before the seam and on it.
    ``scale`` = k > 1 stretches everything along the row by k (longer pulses: a detector then wants ``spp`` near 4 k):
    slots of 16 k samples, half-widths k times as large, the planted shapes interpolated to k times their length.  The
    pair becomes a wide parabola with a spike 3 dB above its peak k samples beside it; the echo across a seam reaches
    about 2.4 k samples over it, alternately from the sample before the seam and back from the sample on it."""
    rng = np.random.default_rng(seed)
    k = max(int(scale), 1)

    def stretch(shape):
        shape = np.asarray(shape, dtype=np.float64)
        m = len(shape)
        return shape if k == 1 else np.interp(np.arange((m - 1) * k + 1) / k, np.arange(m), shape)

    ts = floor + 3.0 * rng.standard_normal((P, S))
    al = rng.uniform(-5.0, 5.0, (P, S))
    at = rng.uniform(-5.0, 5.0, (P, S))

    def position():
        u = rng.random()
        rad = rng.uniform(0.0, 2.0) if u < 0.6 else (rng.uniform(2.0, 3.2) if u < 0.85 else rng.uniform(3.2, 4.5))
        phi = rng.uniform(0.0, 2.0 * np.pi)
        return rad * np.cos(phi), rad * np.sin(phi), (0.05, 0.3, 0.9)[int(rng.choice(3, p=(0.65, 0.2, 0.15)))]

    def put(p, s0, shape, nan_angle=None):
        """The dB values ``shape`` (NaN allowed) from sample ``s0`` on, clipped to the row, with one beam position."""
        a0, b0, jit = position()
        for j, v in enumerate(shape):
            s = s0 + j
            if 0 <= s < S:
                ts[p, s] = v
                al[p, s] = a0 + jit * rng.standard_normal()
                at[p, s] = b0 + jit * rng.standard_normal()
                if nan_angle is not None and j == len(shape) // 2:
                    (al if nan_angle == 0 else at)[p, s] = np.nan

    def parabola(v, h, frac, half=6):
        k = np.arange(-half, half + 1)
        shape = v - 6.0 * ((k - frac) / h) ** 2
        return shape[shape > v - 25.0]

    if S < 16:
        for p in range(P):
            a0, b0, jit = position()
            ts[p] = rng.uniform(-52.0, -35.0) - rng.uniform(0.0, 5.0, S)
            al[p] = a0 + 2.0 * jit * rng.standard_normal(S)
            at[p] = b0 + 2.0 * jit * rng.standard_normal(S)
        ts[rng.random((P, S)) < 0.05] = np.nan
    else:
        for p in range(P):
            for slot in range(S // (16 * k)):
                if rng.random() >= density:
                    continue
                s0 = slot * 16 * k + 3 * k
                v = rng.uniform(-55.0, -30.0)
                kind = rng.random()
                if kind < 0.55:
                    sh = parabola(v, k * float(rng.choice((0.6, 1.2, 1.8, 2.4, 3.2, 4.5))), rng.uniform(-0.5, 0.5), 6 * k)
                    put(p, s0 + 5 * k - len(sh) // 2, sh)
                elif kind < 0.7:  # the weaker peak v lies in the envelope of v + 3
                    if k == 1:
                        put(p, s0, [v - 9, v - 3, v, v - 2.5, v - 2, v + 3, v - 1, v - 9])
                    else:
                        sh = parabola(v, 1.6 * k, rng.uniform(-0.4, 0.4), 6 * k)
                        sh[len(sh) // 2 + k] = v + 3
                        put(p, s0 + 5 * k - len(sh) // 2, sh)
                elif kind < 0.8:
                    put(p, s0, stretch([v - 8, v - 2, v, v, v - 2, v - 8]))
                elif kind < 0.88:
                    sh = stretch([v - 8, v - 2, v, v - 1, v - 2, v - 8]).copy()
                    sh[3 * k] = np.nan
                    put(p, s0, sh)
                else:
                    put(p, s0, stretch([v - 8, v - 2, v - 1, v, v - 1.5, v - 8]), nan_angle=int(rng.integers(2)))
            v = rng.uniform(-45.0, -32.0)
            end = p % 4
            if end == 0:
                put(p, 0, stretch([v, v - 2, v - 4, v - 9, v - 30]))
            elif end == 1:
                put(p, 0, stretch([v - 2, v, v - 1, v - 3, v - 9, v - 30]))
            elif end == 2:
                put(p, S - 4 * k - 1, stretch([v - 30, v - 9, v - 4, v - 2, v]))
            else:
                put(p, S - 5 * k - 1, stretch([v - 30, v - 9, v - 3, v - 1, v, v - 2]))
            if p % 3 == 0:
                for m in range(seam, S - 4 * k, seam):
                    v = rng.uniform(-45.0, -32.0)
                    sh = stretch([v - 30, v - 9, v - 3, v, v - 2, v - 4, v - 9, v - 30])
                    if k == 1:
                        put(p, m - 4 + (p // 3) % 2, sh)
                    elif (p // 3) % 2 == 0:
                        put(p, m - 1 - 3 * k, sh)      # the peak on the sample before the seam, the long side after it
                    else:
                        put(p, m - 4 * k, sh[::-1])    # the peak on the seam, the long side before it
    return {"TS": ts.astype(dtype), "angle_alongship": al.astype(dtype), "angle_athwartship": at.astype(dtype),
            "echo_range": (dr * np.arange(S)).astype(dtype)}


# ---------------------------------------------------------------------------------------- target strength spectra
# (targets.target_spectra; new generators with their own seeds: the ones above are untouched)
def ek80_bandpass_filters(f_start=None, f_stop=None):
    """Band-pass stand-ins for the Vendor_specific WBT / PC filter coefficients, one dict per channel (a list, which
    ``echodata.from_ek80_arrays`` takes).  ``ek80_filters()`` does not pass the transmit band: the replica spectrum A(f)
    of targets.target_spectra is 40 to 100 dB down in band on it.  Here, for the band ``f_start .. f_stop`` of a
    channel (default: ``EK80_BB``), centre fc and width bw:
      stage 1: firwin(47, 0.65 bw, fs=1.5e6) times exp(2 pi i fc k / 1.5e6), decimated by 6;
      stage 2: firwin(91, 0.6 bw, fs=250e3) times exp(2 pi i fc k / 250e3), decimated by 2."""
    from scipy import signal

    f0 = np.asarray(EK80_BB["f_start"] if f_start is None else f_start, dtype=np.float64)
    f1 = np.asarray(EK80_BB["f_stop"] if f_stop is None else f_stop, dtype=np.float64)
    out = []
    for a, b in zip(f0, f1):
        fc, bw = (a + b) / 2, b - a
        wbt = signal.firwin(47, 0.65 * bw, fs=1.5e6) * np.exp(2j * np.pi * fc * np.arange(47) / 1.5e6)
        pc = signal.firwin(91, 0.6 * bw, fs=250e3) * np.exp(2j * np.pi * fc * np.arange(91) / 250e3)
        out.append(dict(wbt_fil=wbt.astype(np.complex64), wbt_decifac=6, pc_fil=pc.astype(np.complex64), pc_decifac=2))
    return out


def target_spectra_scene(C=2, P=3, S=400, B=4, seed=20261021, dtype=np.float64, noise=1e-4, tail=40, echoes=None):
    """An EK80 FM data set with point echoes of KNOWN strength for targets.target_spectra: ``ek80_numpy``'s dictionary
    (its own stream, unchanged) with ``filters`` = ``ek80_bandpass_filters()``, ``beam_type`` 1 and the samples replaced
    by
    - a noise floor: complex normal of standard deviation ``noise`` per part (0: none);
    - echoes ``K tx`` -- ``tx`` the channel's transmit replica rounded to complex64, the values compute_TS uploads --
      planted from sample ``s`` on with the sector phases of ``splitbeam_sector_phases`` for the electrical angles
      ``(e_al, e_at)`` in degrees; ``echoes``: a list of (c, p, s, K, e_al, e_at), default: six per channel -- whole
      echoes 200 samples or more apart, among them one at sample 0, one that ends just in front of the NaN tail and one
      that ends with the row (7 samples earlier on the second channel), and one at the last sample, cut off by the end
      of the row;
    - NaN tails: the last ``tail`` samples of ping 1 of every channel, all sectors;
    - one mixed-sector patch: sector 1 NaN at samples S/2 + 3 .. S/2 + 7 of (channel 0, ping 0), inside the echo at
      S/2, and the imaginary part alone of the last sector at sample 200 of the last (channel, ping).
    The sector mean of an echo is ``K cos(e_al / 2) cos(e_at / 2) tx`` (beam type 1).  Returns (d, replicas, echoes):
    the dictionary (samples of ``dtype``), the complex64 replicas per channel and the list of echoes."""
    from .calibrate.ek80_complex import filter_decimate_chirp, tapered_chirp

    d = ek80_numpy(C=C, P=P, S=S, B=B, seed=seed, waveform="BB")
    filters = ek80_bandpass_filters(d["f_start"], d["f_stop"])
    replicas = []
    for c in range(C):
        y, _ = tapered_chirp(d["fs"][c], d["tau"][c], d["slope"][c], d["f_start"][c], d["f_stop"][c])
        tx, _ = filter_decimate_chirp(filters[c], y, d["fs"][c])
        replicas.append(np.asarray(tx).astype(np.complex64))
    rng = np.random.default_rng(seed + 11)
    x = (rng.standard_normal((C, P, S, B)) + 1j * rng.standard_normal((C, P, S, B))) * noise
    if echoes is None:
        echoes = []
        for c in range(C):
            L = replicas[c].size
            # whole echoes, 200 samples or more apart, the last of a ping ending with the row (or in front of the NaN
            # tail), and one cut off by the end of the row
            echoes += [(c, 0, 0, 0.31, 0.0, 0.0), (c, 0, S // 2, 0.08, 40.0, -25.0),
                       (c, 1 % P, max(S - tail - L - 1, 0), 0.22, 15.0, 35.0),
                       (c, P - 1, 30, 0.12, 0.0, 0.0), (c, P - 1, max(S - L - (7 if c else 0), 0), 0.27, 30.0, 30.0),
                       (c, P - 1, S - 1, 0.5, -20.0, -45.0)]
    for c, p, s, K, e_al, e_at in echoes:
        tx = replicas[c].astype(np.complex128)
        n = min(tx.size, S - s)
        sec = splitbeam_sector_phases(np.float64(e_al), np.float64(e_at), 1)[:B]
        x[c, p, s:s + n, :] += K * tx[:n, None] * sec[None, :]
    re = np.ascontiguousarray(x.real).astype(dtype)
    im = np.ascontiguousarray(x.imag).astype(dtype)
    if P > 1 and tail > 0:
        re[:, 1, S - tail:, :] = np.nan
        im[:, 1, S - tail:, :] = np.nan
    if B > 1 and S > 200:
        re[0, 0, S // 2 + 3:S // 2 + 8, 1] = np.nan
        im[0, 0, S // 2 + 3:S // 2 + 8, 1] = np.nan
        im[C - 1, P - 1, 200, B - 1] = np.nan
    d["backscatter_r"], d["backscatter_i"] = re, im
    d["beam_type"] = np.ones(C, dtype=np.int64)
    d["filters"] = filters
    return d, replicas, list(echoes)
