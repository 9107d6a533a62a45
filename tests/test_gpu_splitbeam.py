"""Split-beam angles on the GPU (csrc/splitbeam.hip through ops.splitbeam_* and consolidate.add_splitbeam_angle):
every form and beam type against the reference-executed goldens, a known-answer target, the reference's NaN patterns,
float32 output, a multi-filter_time file in one launch, device-resident outputs, direct == FFT."""
import os

import numpy as np
import pytest

from splitbeam_ref import (GOLDEN, load_goldens, assert_complex_bound, assert_complex_close, complex_angle_bounds,
                           complex_angles)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PC_TAGS = ["pc_fft", "pc_fft17", "pc_short", "pc_long", "pc_multi"]
CX_TAGS = ["cx_bt1", "cx_bt17", "cx_bt49", "cx_bt65", "cx_bt81", "cx_mixed"]


@pytest.fixture(scope="module")
def g():
    return load_goldens(os.path.join(HERE, "golden", GOLDEN))


def _t(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _prm(g, tag):
    return [g[f"{tag}_{k}"] for k in ("sens_al", "sens_at", "off_al", "off_at")]


def _dev_prm(g, tag):
    import torch

    return [_t(v, torch.float64) for v in _prm(g, tag)]


def _replicas(g, tag):
    reps, k = [], 0
    while f"{tag}_replica{k}_0" in g:
        c = 0
        while f"{tag}_replica{k}_{c}" in g:
            reps.append(g[f"{tag}_replica{k}_{c}"])
            c += 1
        k += 1
    return reps


def _dev_replicas(reps):
    import torch

    off = np.concatenate([[0], np.cumsum([r.size for r in reps])]).astype(np.int32)
    flat = np.concatenate(reps).astype(np.complex64).view(np.float32)
    return _t(flat), _t(off), int(max(r.size for r in reps))


def _pc_inputs(g, tag):
    import torch

    reps = _replicas(g, tag)
    rep, off, taps = _dev_replicas(reps)
    C = g[f"{tag}_re"].shape[0]
    rid_h = g[f"{tag}_replica_id"]
    rid = None if len(reps) == C and np.array_equal(rid_h, np.arange(C)[:, None] + 0 * rid_h) else _t(rid_h, torch.int32)
    return reps, rid_h, dict(replica=rep, replica_off=off, max_taps=taps, replica_id=rid)


def _check(g, tag, th, ph, weak):
    sa, st, oa, ot = _prm(g, tag)
    assert_complex_close(th.cpu().numpy(), g[f"{tag}_theta"], sa, oa, weak)
    assert_complex_close(ph.cpu().numpy(), g[f"{tag}_phi"], st, ot, weak)


def _bt(g, tag):
    """The kernel's beam-type table: a type the reference skips (mixed types) is -1."""
    bt = g[f"{tag}_beam_type"]
    return np.where(np.isin(bt, (1, 17, 49, 65, 81)), bt, -1)


def _weak(g, tag, reps=None, rid=None):
    return complex_angles(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"], *_prm(g, tag), reps, rid)[3]


# ---- power / angle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["pow_i8", "pow_f32"])
@pytest.mark.parametrize("in_dtype", ["as_stored", "float64"])
def test_power_against_goldens(g, tag, in_dtype):
    import torch

    from echopype_amd import ops

    a, b = g[f"{tag}_angle_alongship"], g[f"{tag}_angle_athwartship"]
    if in_dtype == "float64":
        a, b = a.astype(np.float64), b.astype(np.float64)
    th, ph = ops.splitbeam_power(_t(a), _t(b), _dev_prm(g, tag))
    assert th.dtype == torch.float64
    for got, want in ((th.cpu().numpy(), g[f"{tag}_theta"]), (ph.cpu().numpy(), g[f"{tag}_phi"])):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        f = ~np.isnan(want)
        assert np.max(np.abs(got[f] - want[f])) <= 1e-12


def test_power_float32_output_and_unaligned_length(g):
    """S = 37 / 41 take the scalar form; a multiple of 4 the vector form: both against the f64 result."""
    import torch

    from echopype_amd import ops

    rng = np.random.default_rng(3)
    for S in (41, 64):
        a = rng.integers(-128, 128, (2, 3, S)).astype(np.int8)
        b = rng.integers(-128, 128, (2, 3, S)).astype(np.int8)
        prm = [_t(np.array([22.0, 23.5])), _t(np.array([21.0, 24.0])), _t(np.array([0.1, -0.2])), _t(np.array(0.05))]
        th, ph = ops.splitbeam_power(_t(a), _t(b), prm)
        th32, ph32 = ops.splitbeam_power(_t(a), _t(b), prm, dtype=torch.float32)
        assert th32.dtype == torch.float32
        np.testing.assert_array_equal(th32.cpu().numpy(), th.cpu().numpy().astype(np.float32))
        np.testing.assert_array_equal(ph32.cpu().numpy(), ph.cpu().numpy().astype(np.float32))
        want = 180 / 128 * a.astype(float) / np.array([22.0, 23.5])[:, None, None] - np.array([0.1, -0.2])[:, None, None]
        assert np.max(np.abs(th.cpu().numpy() - want)) <= 1e-12


# ---- complex, no replica -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CX_TAGS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_complex_against_goldens(g, tag, dtype):
    import torch

    from echopype_amd import ops

    th, ph = ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag), _dev_prm(g, tag),
                                   dtype=getattr(torch, dtype))
    assert th.dtype == getattr(torch, dtype)
    _check(g, tag, th, ph, _weak(g, tag))


def test_complex_float64_planes_and_generic_sector_load(g):
    """f64 planes (the NB = 4 vector loads of f64) and a misaligned plane (the per-sector loads) agree."""
    import torch

    from echopype_amd import ops

    tag = "cx_bt1"
    re, im = g[f"{tag}_re"].astype(np.float64), g[f"{tag}_im"].astype(np.float64)
    th, ph = ops.splitbeam_complex(_t(re), _t(im), _bt(g, tag), _dev_prm(g, tag))
    _check(g, tag, th, ph, _weak(g, tag))
    buf_r = torch.empty(re.size + 1, dtype=torch.float32, device="cuda")
    buf_i = torch.empty(re.size + 1, dtype=torch.float32, device="cuda")
    r1 = buf_r[1:].view(re.shape)
    i1 = buf_i[1:].view(re.shape)
    r1.copy_(_t(g[f"{tag}_re"]))
    i1.copy_(_t(g[f"{tag}_im"]))
    th2, ph2 = ops.splitbeam_complex(r1, i1, _bt(g, tag), _dev_prm(g, tag))
    th3, ph3 = ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag), _dev_prm(g, tag))
    np.testing.assert_array_equal(th2.cpu().numpy(), th3.cpu().numpy())
    np.testing.assert_array_equal(ph2.cpu().numpy(), ph3.cpu().numpy())


# ---- complex with pulse compression -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", PC_TAGS)
@pytest.mark.parametrize("method", ["auto", "direct", "fft"])
def test_pulse_compressed_against_goldens(g, tag, method):
    import torch

    from echopype_amd import _lib, ops

    reps, rid_h, kw = _pc_inputs(g, tag)
    if method == "fft" and kw["max_taps"] > _lib.EK80_NFFT // 2:
        with pytest.raises(ValueError, match="FFT form takes replicas"):
            ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag), _dev_prm(g, tag),
                                  method=method, **kw)
        return
    with _lib.launch_trace() as tr:
        th, ph = ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag),
                                       _dev_prm(g, tag), method=method, **kw)
    want = "sba_pc_fft_kernel" if ops.splitbeam_uses_fft(kw["replica"], kw["max_taps"], method) else "sba_pc_direct_kernel"
    assert want in tr.kernels and tr.kernels.count(want) == 1  # a multi-filter_time file too: ONE launch
    assert th.dtype == torch.float64
    _check(g, tag, th, ph, _weak(g, tag, reps, rid_h))


def test_auto_picks_the_sv_rule(g):
    from echopype_amd import ops

    for tag, fft in (("pc_fft", True), ("pc_short", False), ("pc_long", False)):
        _, _, kw = _pc_inputs(g, tag)
        assert ops.splitbeam_uses_fft(kw["replica"], kw["max_taps"]) is fft
        assert ops.sv_complex_uses_fft(kw["replica"], kw["max_taps"]) is fft


@pytest.mark.parametrize("fft_dtype", ["float64", "float32"])
def test_direct_equals_fft(g, fft_dtype):
    """The same replica through both forms: f64 transform to ~1e-9 deg, complex64 butterflies to the f32 tolerance."""
    import torch

    from echopype_amd import ops

    tag = "pc_fft"
    reps, rid_h, kw = _pc_inputs(g, tag)
    re, im = _t(g[f"{tag}_re"]), _t(g[f"{tag}_im"])
    d_th, d_ph = ops.splitbeam_complex(re, im, _bt(g, tag), _dev_prm(g, tag), method="direct", **kw)
    f_th, f_ph = ops.splitbeam_complex(re, im, _bt(g, tag), _dev_prm(g, tag), method="fft",
                                       fft_dtype=getattr(torch, fft_dtype), **kw)
    weak = _weak(g, tag, reps, rid_h)
    sa, st, oa, ot = _prm(g, tag)
    # complex64 butterflies err by ~3e-7 of the TILE's strongest echo (ek80_fft.hip), not of the sample: near the
    # 1e-3-of-RMS factors that is ~1e-2 deg
    tol = 1e-7 if fft_dtype == "float64" else 0.05
    assert_complex_close(f_th.cpu().numpy(), d_th.cpu().numpy(), sa, oa, weak, tol=tol)
    assert_complex_close(f_ph.cpu().numpy(), d_ph.cpu().numpy(), st, ot, weak, tol=tol)
    if fft_dtype == "float32":
        # each form on its own against the float64 oracle angles (on the complex64 replica the kernels read), with the
        # bound derived per sample (tests/f32_bounds.py); 0.05 deg stays as a cap on top of it.  The samples left out
        # as ``weak`` are the ones splitbeam_ref leaves out.  For the complex64 transform the derived bound -- the
        # tile's normwise bound taken per sample -- is below the cap at 3 % of this golden's samples only: the cap is
        # what judges the rest (tests/test_f32_bounds.py::test_bb_splitbeam_bound_governs_where_stated; the share is
        # logged).  For the float64 direct form the derived bound governs everywhere.
        _judge_pc(g, tag, reps, rid_h, kw, f_th, f_ph, "fft", 2.0**-24, 2.0**-53, 0.05, "sba fft complex64")
        _judge_pc(g, tag, reps, rid_h, kw, d_th, d_ph, "direct", 2.0**-53, 2.0**-53, 0.05, "sba direct float64")


def _judge_pc(g, tag, reps, rid_h, kw, th, ph, form, u_f, u_t, cap, what):
    """Pulse-compressed angles against ``complex_angle_bounds`` (u_f: the transform's / the combination's precision,
    u_t: the output type's), capped at ``cap``."""
    sa, st, oa, ot = _prm(g, tag)
    rid = None if kw["replica_id"] is None else rid_h
    w_th, w_ph, b_al, b_at, weak = complex_angle_bounds(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"], sa, st,
                                                        oa, ot, reps, rid, form=form, max_taps=kw["max_taps"],
                                                        u_f=u_f, u_t=u_t)
    np.testing.assert_array_equal(weak, _weak(g, tag, reps, rid_h))
    th, ph = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (th, ph)]
    assert_complex_bound(th, w_th, sa, oa, weak, b_al, cap, what + " theta")
    assert_complex_bound(ph, w_ph, st, ot, weak, b_at, cap, what + " phi")


def test_float32_output_pulse_compressed(g):
    import torch

    from echopype_amd import ops

    for tag in ("pc_fft", "pc_short"):
        reps, rid_h, kw = _pc_inputs(g, tag)
        th, ph = ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag),
                                       _dev_prm(g, tag), dtype=torch.float32, **kw)
        assert th.dtype == torch.float32
        _check(g, tag, th, ph, _weak(g, tag, reps, rid_h))
        # the derived bound of the float32 output (complex128 transform / float32 direct form) beside the goldens' 1e-3
        fft = ops.splitbeam_uses_fft(kw["replica"], kw["max_taps"])
        _judge_pc(g, tag, reps, rid_h, kw, th, ph, "fft" if fft else "direct", 2.0**-53 if fft else 2.0**-24, 2.0**-24,
                  0.05, f"sba float32 output {tag}")


# ---- known answer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bt,B", [(1, 4), (17, 3), (17, 4), (49, 4), (65, 4), (81, 4)])
def test_known_target(bt, B):
    """Sector phases built so that theta / phi are known in closed form (synth.ek80_splitbeam_numpy): from f64 planes
    in fp64 the angles hold to 1e-9 deg -- a sector taken in the wrong order or a combination mixed up is off by
    degrees."""
    from echopype_amd import ops, synth

    d, theta, phi = synth.ek80_splitbeam_numpy(C=2, P=5, S=700, B=B, beam_type=bt)
    prm = [_t(d[k]) for k in ops.SPLITBEAM_PARAMS]
    th, ph = ops.splitbeam_complex(_t(d["backscatter_r"]), _t(d["backscatter_i"]), d["beam_type"], prm)
    assert np.max(np.abs(th.cpu().numpy() - theta)) < 1e-9
    assert np.max(np.abs(ph.cpu().numpy() - phi)) < 1e-9


def test_known_target_through_a_unit_replica():
    """A one-tap replica of 1 (direct) and a 20-tap replica e_0 (FFT): pulse compression leaves the samples as they
    are, so the known angles come out of both forms too."""
    from echopype_amd import ops, synth

    d, theta, phi = synth.ek80_splitbeam_numpy(C=2, P=3, S=2500, B=4, beam_type=[1, 49])
    prm = [_t(d[k]) for k in ops.SPLITBEAM_PARAMS]
    for n, method in ((1, "direct"), (20, "fft")):
        r = np.zeros(n, np.complex64)
        r[0] = 1.0
        rep, off, taps = _dev_replicas([r, r])
        th, ph = ops.splitbeam_complex(_t(d["backscatter_r"]), _t(d["backscatter_i"]), d["beam_type"], prm,
                                       replica=rep, replica_off=off, max_taps=taps, method=method)
        assert np.max(np.abs(th.cpu().numpy() - theta)) < 1e-9
        assert np.max(np.abs(ph.cpu().numpy() - phi)) < 1e-9


# ---- the public API --------------------------------------------------------------------------------------------------
def _api_ek80(g, tag, waveform="BB"):
    """An EK80 EchoData holding a golden case's samples and an Sv-like dataset with its angle parameters."""
    from echopype_amd import echodata, synth
    from echopype_amd.xr_lite import Dataset

    re, im = g[f"{tag}_re"], g[f"{tag}_im"]
    C, P, S, B = re.shape
    d = synth.ek80_numpy(C=min(C, 2), P=P, S=S, B=B, waveform=waveform)
    if C > 2:  # (the synthetic parameter tables have two channels: repeat them)
        for k, v in list(d.items()):
            if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 2 and k != "ping_time":
                d[k] = np.resize(v, (C,) + v.shape[1:])
        d["channel"] = [f"WBT 4000{i}-15 ES{i}" for i in range(C)]
    d["backscatter_r"], d["backscatter_i"] = re, im
    d["beam_type"] = g[f"{tag}_beam_type"]
    ed = echodata.from_ek80_arrays(d, synth.ek80_filters())
    ds = Dataset(coords={"channel": list(d["channel"]), "ping_time": d["ping_time"], "range_sample": np.arange(S)},
                 attrs={"processing_function": "calibrate.compute_Sv"})
    sa, st, oa, ot = _prm(g, tag)
    cp = ("channel", "ping_time")
    for k, v in zip(("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
                     "angle_offset_athwartship"), (sa, st, oa, ot)):
        ds[k] = (("channel",) if v.ndim == 1 else cp, v)
    ds["receiver_sampling_frequency"] = (("channel",), d["fs"])
    return ed, ds, d


@pytest.mark.parametrize("tag", ["cx_bt1", "cx_bt17", "cx_mixed"])
def test_api_complex_without_pulse_compression(g, tag):
    import echopype_amd as ep
    from echopype_amd.xr_lite import DeviceArray

    ed, ds, _ = _api_ek80(g, tag)
    out = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", to_disk=False)
    assert out is ds
    th, ph = out["angle_alongship"], out["angle_athwartship"]
    assert tuple(th.dims) == ("channel", "ping_time", "range_sample") and th.attrs["long_name"].startswith("split-beam")
    assert th.attrs["history"][:4].isdigit() and isinstance(th.data, DeviceArray)
    assert th.data.tensor.dtype.is_floating_point and th.dtype == np.float64
    sa, st, oa, ot = _prm(g, tag)
    weak = _weak(g, tag)
    assert_complex_close(th.values, g[f"{tag}_theta"], sa, oa, weak)
    assert_complex_close(ph.values, g[f"{tag}_phi"], st, ot, weak)


def test_api_pulse_compression_uses_the_calibrators_replica(g):
    """BB with pulse compression through the public API: the replica is what calibrate's get_transmit_signal builds
    from Vendor_specific; the result equals ops with that replica, and the restatement with it."""
    import torch

    import echopype_amd as ep
    from echopype_amd import ops
    from echopype_amd.calibrate.ek80_complex import get_filter_coeff, get_transmit_signal

    tag = "cx_bt1"
    ed, ds, d = _api_ek80(g, tag)
    out = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", pulse_compression=True, to_disk=False)
    beam = ed["Sonar/Beam_group1"]
    tx, _ = get_transmit_signal(beam, get_filter_coeff(ed["Vendor_specific"]), "BB", ds["receiver_sampling_frequency"])
    reps = [np.asarray(tx[ch]) for ch in beam["channel"].values]
    rep, off, taps = _dev_replicas(reps)
    th, ph = ops.splitbeam_complex(_t(g[f"{tag}_re"]), _t(g[f"{tag}_im"]), _bt(g, tag), _dev_prm(g, tag),
                                   replica=rep, replica_off=off, max_taps=taps)
    np.testing.assert_array_equal(out["angle_alongship"].values, th.cpu().numpy())
    np.testing.assert_array_equal(out["angle_athwartship"].values, ph.cpu().numpy())
    # against the restatement with the f64 replica: the kernels take the replica as complex64 (as the Sv kernels do),
    # an error of ~6e-8 of the tile's signal, not of the sample -- a looser bound than the goldens' 1e-3 deg
    want_th, want_ph, _, weak = complex_angles(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"], *_prm(g, tag),
                                               reps)
    sa, st, oa, ot = _prm(g, tag)
    assert_complex_close(th.cpu().numpy(), want_th, sa, oa, weak, tol=0.05)
    assert_complex_close(ph.cpu().numpy(), want_ph, st, ot, weak, tol=0.05)
    # ... and against the restatement with the complex64 replica the kernels read: the derived bound (complex128
    # transform, float64 output), 0.05 deg as a cap
    fft = ops.splitbeam_uses_fft(rep, taps)
    w_th, w_ph, b_al, b_at, weak64 = complex_angle_bounds(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"],
                                                          *_prm(g, tag), reps, form="fft" if fft else "direct",
                                                          max_taps=taps, u_f=2.0**-53, u_t=2.0**-53)
    assert_complex_bound(th.cpu().numpy(), w_th, sa, oa, weak64, b_al, 0.05, "sba API theta")
    assert_complex_bound(ph.cpu().numpy(), w_ph, st, ot, weak64, b_at, 0.05, "sba API phi")
    # float32 output through the API
    ed, ds, d = _api_ek80(g, tag)
    out32 = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", pulse_compression=True, to_disk=False,
                                               dtype="float32")
    assert out32["angle_alongship"].data.tensor.dtype == torch.float32
    # ... judged like the float64 one: complex128 transform (the route's default) or float32 direct form, float32 output
    w_th, w_ph, b_al, b_at, weak32 = complex_angle_bounds(g[f"{tag}_re"], g[f"{tag}_im"], g[f"{tag}_beam_type"],
                                                          *_prm(g, tag), reps, form="fft" if fft else "direct",
                                                          max_taps=taps, u_f=2.0**-53 if fft else 2.0**-24, u_t=2.0**-24)
    assert_complex_bound(out32["angle_alongship"].values, w_th, sa, oa, weak32, b_al, 0.05, "sba API float32 theta")
    assert_complex_bound(out32["angle_athwartship"].values, w_ph, st, ot, weak32, b_at, 0.05, "sba API float32 phi")


def test_api_power_samples_ek60_and_nan_padding():
    """EK60 power/angle through the API: int8 planes (uploaded by the call) and NaN-padded float32 planes."""
    import echopype_amd as ep
    from echopype_amd import echodata, synth
    from echopype_amd.xr_lite import Dataset
    from splitbeam_ref import power_angles

    for nan_pad in (False, True):
        d = synth.ek60_splitbeam_numpy(C=2, P=20, S=300, nan_pad=nan_pad)
        ed = echodata.from_ek60_arrays(d)
        ds = Dataset(coords={"channel": list(d["channel"]), "ping_time": d["ping_time"], "range_sample": np.arange(300)},
                     attrs={"processing_function": "calibrate.compute_Sv"})
        prm = []
        for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
                  "angle_offset_athwartship"):
            ds[k] = (("channel",), d[k])
            prm.append(d[k])
        out = ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)
        want_th, want_ph = power_angles(d["angle_alongship"], d["angle_athwartship"], *prm)
        for got, want in ((out["angle_alongship"].values, want_th), (out["angle_athwartship"].values, want_ph)):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            assert np.isnan(got).any() == nan_pad
            f = ~np.isnan(want)
            assert np.max(np.abs(got[f] - want[f])) <= 1e-12


def test_api_reads_resident_samples_and_leaves_results_resident(g, monkeypatch):
    """After to_device() the samples are read where they are (no upload of the planes) and the outputs stay in HBM:
    nothing synchronises with the host until .values."""
    import torch

    import echopype_amd as ep
    from echopype_amd import ops

    tag = "cx_bt49"
    ed, ds, _ = _api_ek80(g, tag)
    ed.to_device()
    big = []
    real_upload = ops.to_device

    def spy(a, *k, **kw):
        if np.asarray(a).nbytes > 100_000:
            big.append(np.asarray(a).shape)
        return real_upload(a, *k, **kw)

    monkeypatch.setattr(ops, "to_device", spy)
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: synced.append(1))
    out = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", to_disk=False)
    assert not big and not synced
    assert out["angle_alongship"].data.tensor.is_cuda
    monkeypatch.undo()
    sa, st, oa, ot = _prm(g, tag)
    weak = _weak(g, tag)
    assert_complex_close(out["angle_alongship"].values, g[f"{tag}_theta"], sa, oa, weak)


def test_api_channel_subset_of_source_sv(g):
    """source_Sv holding one channel of two: ds_beam.sel(channel=source_Sv.channel)."""
    import echopype_amd as ep
    from echopype_amd.xr_lite import Dataset

    tag = "cx_bt1"
    ed, ds_full, d = _api_ek80(g, tag)
    ds = Dataset(coords={"channel": [d["channel"][1]], "ping_time": d["ping_time"],
                         "range_sample": ds_full["range_sample"].values},
                 attrs={"processing_function": "calibrate.compute_Sv"})
    for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
              "angle_offset_athwartship"):
        ds[k] = (("channel",), ds_full[k].values[1:])
    out = ep.consolidate.add_splitbeam_angle(ds, ed, "BB", "complex", to_disk=False)
    sa, st, oa, ot = _prm(g, tag)
    weak = _weak(g, tag)[1:]
    assert_complex_close(out["angle_alongship"].values, g[f"{tag}_theta"][1:], sa[1:], oa[1:], weak)


def test_argument_errors_come_from_the_library(g):
    from echopype_amd import ops

    tag = "cx_bt17"  # B = 3
    re, im = _t(g[f"{tag}_re"]), _t(g[f"{tag}_im"])
    with pytest.raises(ValueError, match="needs 4 sectors"):
        ops.splitbeam_complex(re, im, [1, 1], _dev_prm(g, tag))
    with pytest.raises(ValueError, match="beam_type 5"):
        ops.splitbeam_complex(re, im, [17, 5], _dev_prm(g, tag))
    with pytest.raises(ValueError, match="3 or 4 sectors"):
        ops.splitbeam_complex(re[..., :2].contiguous(), im[..., :2].contiguous(), [17, 17], _dev_prm(g, tag))
