"""What a call returns is a function of its inputs alone: every ``ops`` wrapper that allocates an output or scratch,
and some thirty public API calls, run three times -- plainly, with every fresh device allocation pre-filled with 0xA5, and
with 0x5A (tests/poison.py) -- must give the same bits, leave every guard band intact, and have allocated through the
patch.  A result element the library never wrote, or a scratch word it read before writing it, differs between the two
patterns.

The table ``CASES`` below is the file: one row per case, a closure over one wrapper or one API call, built from small
seeded inputs.  ``kind``:

- ``base``: ordinary input at the smallest shapes at which the launch plan has an edge (rows of 1, 3, 4, 5, 63, 64, 65,
  255, 256, 257 samples; tile edges of the single-target, track and window-filter kernels; both element types);
- ``degenerate``: all samples NaN, a bin without a member, a channel without targets, masks that remove everything.
  Such a row also holds its result to the wrapper's reference (oracle/, tests/*_ref.py, or the reference's rule restated in
  NumPy beside it) on the row's own inputs -- an empty or all-NaN reduction gives NaN there -- or names in ``no_oracle``
  why there is none;
- ``zero``: a zero-length dimension.  ``zero="returns"``: arrays of the documented shape, identical under both patterns;
  ``zero="raises"``: ValueError before any launch (``_lib.launch_trace()`` stays empty).  Which one holds is recorded
  in the row, so a change of behaviour shows.

No case runs its closure more than three times; no case compares with a tolerance (``FALLBACK`` is empty): where
floating-point atomics could reorder additions the shapes give at most two partials per cell (the binned means: two
sample columns per range bin, ``FINE``; NASC: one ping per distance bin as well; region sums: regions of two pixels),
and orders the API leaves free are canonicalised (the component ids of ``shoal_label``, the roots of
``seafloor_components``, the reversal list of ``time_reversals``).

Scratch interiors are poisoned as well.  ``AUDIT`` names, for every buffer of ``epa_scratch_bytes``, where the library
initialises it before its first read; tests/test_poison_table_host.py holds it to the table in csrc/runtime.hip."""
import numpy as np
import pytest

from poison import BYTES, Poisoned
from test_gpu_scratch_guard import _bits, complex_rows, power_rows, randn, replicas

pytestmark = pytest.mark.gpu

# buffer -> where the library initialises it before its first read
AUDIT = {
    "sv_power_stats.workspace": "sv_power.hip:415 piece_keys_init_kernel (keys :262-264) on the one-piece route; the strided "
                                "rows write one partial per workgroup, folded at sv_power.hip:445; the scalar route hands it "
                                "to epa_nanminmax (below)",
    "depth_rows.workspace": "reduce_util.hip:296 piece_slots_init_kernel (:196-201) on the one-piece route; depth_rows_kernel "
                            "(reduce_util.hip:364) writes its workgroup's partial, epa_minmax_final reads `grid` of them (:369)",
    "nanminmax.workspace": "reduce_util.hip:36-38: each of the `grid` workgroups writes its partial; minmax_final_kernel reads "
                           "`grid` partials (:409)",
    "range_step_mean.workspace": "reduce_util.hip:97-98: step_rows_kernel writes (sum, count) of every (channel, ping) row",
    "sv_complex_cw_stats.workspace": "ek80_complex.hip:537 cw_stats_init_kernel",
    "sv_complex_fft.workspace": "ek80_fft.hip:850 replica_prepare_kernel (spectra, log table, statistics slots), :870 "
                                "hipMemsetAsync of the deferred-tile counter and map, :877 tvg_table_kernel",
    "sv_complex_fft_indexed.workspace": "the same entry (ek80_fft.hip:832)",
    "selftest_correlate.workspace": "the same layout: replica_prepare_kernel of epa_selftest_correlate",
    "splitbeam_complex_fft.workspace": "splitbeam.hip:679 sba_replica_spectrum_kernel writes every replica's spectrum",
    "sv_mvbs_fused_depth.depth_stats_out": "block_reduce.hip:693 init_range_outputs (the key word and the three statistics)",
    "apply_masks.workspace": "noise_masks.hip:3139-3140: each of the `grid` workgroups writes its pair; minmax_pairs_kernel "
                             "reads `grid` pairs (none when n == 0)",
    "pool_sv.sum_ws": "noise_masks.hip:3277 / :3283 box_range(_scan)_kernel writes the columns [first_sample, S) of every row, "
                      "the ones box_ping_slide_kernel reads",
    "pool_sv.cnt_ws": "the same two kernels",
    "pool_sv_value.ws_mean": "noise_masks.hip:3336-3338 ref / differ / ilo / ihi (every entry: :1881, :1918-1919); the run "
                             "tables :3370-3373 hipMemsetAsync and run_flag / run_scan_tiles / run_finish kernels (every row: "
                             ":2062, :2093, :2167-2168); the lean kernel's todo bytes :3453; the running sums and `dirty` by "
                             "row_running_sum_kernel (:1097-1107) for the rows the staged kernels read",
    "pool_sv_value.ws_median": "noise_masks.hip:3475-3477 ref_row / rows_same / value_intervals kernels write every entry",
    "nasc.workspace": "nasc.hip:223 hipMemsetAsync",
    "seafloor.state": "ops.py seafloor_state: zero=True",
    "seafloor_angle_mask.work": "seafloor.hip:415 sf_box_rows_kernel writes both planes before sf_box_cols_kernel reads them",
    "seafloor_median.hist": "seafloor.hip:434 hipMemsetAsync before every radix pass",
    "shoal.state": "ops.py shoal_state: zero=True",
    "shoal_echoview_link.queue": "shoal.hip:365-366: sh_link_kernel writes entry `slot` before counting it in state[kBig]; "
                                 "sh_link_big_kernel reads the first min(state[kBig], capacity) entries (:382-386)",
    "transient_fielding.todo": "transient.hip:96: entry i is written when `count` passes i; the walk reads i < count (:106-113)",
    "transient_fielding.count": "transient.hip:280 hipMemsetAsync",
    "transient_matecho.s_hi": "transient.hip:170 tr_matecho_rows_kernel writes every row",
    "transient_matecho.flag": "transient.hip:237 tr_matecho_flag_kernel writes every row",
    "time_rebuild.tile_workspace": "qc.hip:150 time_tile_sums_kernel writes every tile's sum before the carry kernel (:155)",
    "regrid_mask.out": "mask_grid.hip:382 regrid_clear_kernel",
    "target_spectra.table": "target_spectrum.hip:265-268 replica_table_kernel",
    "sv_spectrum.table": "sv_spectrum.hip:369-372 replica_table_kernel",
}

FALLBACK = {}  # case name -> why it compares with a tolerance instead of bits (none does)


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


# ---- inputs ------------------------------------------------------------------------------------------------------------
ROWS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
# the samples of ``power_rows`` lie 0.2 m apart: on range bins of 0.3 m a cell of a binned mean takes the sums of two
# columns at the most, and two floating-point atomics on a zeroed cell give the same bits in either order
FINE = 0.3
NAN = float("nan")


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def nans(torch, shape, dtype):
    return torch.full(shape, NAN, dtype=dtype).cuda()


def samples(torch, shape, dtype, seed, fill="rand", **kw):
    """Seeded values with a few NaN (``fill="rand"``) or nothing but NaN (``fill="nan"``)."""
    return nans(torch, shape, dtype) if fill == "nan" else randn(torch, shape, dtype, seed, **kw)


def sv_like(torch, shape, dtype, seed, fill="rand"):
    return samples(torch, shape, dtype, seed, fill, scale=8.0, shift=-70.0)


def ramp(torch, shape, dtype, step=0.5, first=0.0):
    """A range array: ``first + step * sample`` in every row."""
    S = shape[-1]
    return (first + step * torch.arange(S, dtype=torch.float64)).expand(shape).contiguous().to(dtype).cuda()


def ping_ns(P, step=10**9):
    return np.arange(P, dtype=np.int64) * step + 1_700_000_000 * 10**9


def tdt(torch, name):
    return getattr(torch, name)


def host(t):
    return t.detach().cpu().numpy()


def checked(run, check):
    """``run`` with its result held to ``check`` (the wrapper's reference on the row's inputs) every time it runs."""
    def both():
        res = run()
        check(res)
        return res

    both.has_oracle = True
    return both


def same(got, want, what, rtol=0.0):
    """NaN and infinity patterns equal, finite values equal (or within ``rtol`` of max(|want|, 1))."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    f = np.isfinite(want.astype(np.float64))
    np.testing.assert_array_equal(got[~f & ~np.isnan(want)], want[~f & ~np.isnan(want)], err_msg=f"{what}: infinities")
    err = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64)) / np.maximum(np.abs(want[f].astype(np.float64)), 1.0)
    assert err.size == 0 or err.max() <= rtol, f"{what}: {err.max():.3e} > {rtol}"


def nan_in_nan_out(run, pick, why):
    """``run`` held to the reference's rule ``why``: without a valid sample every picked float output is NaN, every picked
    mask (uint8 / bool) is empty."""
    def check(res):
        for k, t in enumerate(pick(res)):
            h = host(t)
            assert (np.isnan(h).all() if h.dtype.kind == "f" else not h.any()), f"{why}: output {k} of all-NaN input"

    return checked(run, check)


def binned_mean_ref(sv, rng, P, per, n_tbins, range_bin, n_rbins):
    """oracle.commongrid.groupby_mean on ping numbers as times: the bins of ``bins_of`` are [k * per, (k + 1) * per)."""
    from oracle import commongrid as ogrid

    t_edges = np.arange(n_tbins + 1, dtype=np.float64) * per
    return ogrid.groupby_mean(np.asarray(sv, dtype=np.float64), np.asarray(rng, dtype=np.float64),
                              np.arange(P, dtype=np.float64), t_edges, np.arange(n_rbins + 1) * float(range_bin))


def ek60(torch, ops, C, P, S, nan_ping=False):
    from echopype_amd import synth

    d = synth.ek60_numpy(C, max(P, 1), S, vary_tau=True)
    if nan_ping and P:
        d["transmit_duration_nominal"][0, P // 2] = np.nan
    if P == 0:  # no ping: the per-ping tables cut to nothing
        tau0 = d["transmit_duration_nominal"][:, :1].copy()
        d = {k: (v[:, :0] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[:2] == (C, 1) else v) for k, v in d.items()}
        d["transmit_duration_nominal"] = np.concatenate([tau0, tau0], axis=1)[:, :0]
        d["tau0"] = tau0[:, 0]
    return d


def coef_ek60(torch, ops, d, cal_type="Sv"):
    f64 = torch.float64
    g = lambda k: dev(torch, d[k], f64)  # noqa: E731
    return ops.power_coef_ek(g("sample_interval"), g("transmit_duration_nominal"), g("transmit_power"),
                             g("sound_speed_indicative"), g("absorption_indicative"), g("gain_correction"), g("sa_correction"),
                             g("equivalent_beam_angle"), g("frequency_nominal"),
                             dev(torch, d["tau0"] if "tau0" in d else d["transmit_duration_nominal"][:, 0].copy(), f64),
                             sonar="EK60", cal_type=cal_type,
                             pulse_length=g("pulse_length"), gain_is_table=True, sa_is_table=True)


# ---- the ops wrappers: builders of closures -------------------------------------------------------------------------------
def b_power_coef(torch, ops, C=2, P=5, nan_ping=False):
    d = ek60(torch, ops, C, P, 4, nan_ping)
    return lambda: coef_ek60(torch, ops, d)


def b_pulse_table(torch, ops, C=2, P=5, nan=False):
    d = ek60(torch, ops, C, P, 4)
    tau = np.full((C, P), np.nan) if nan else d["transmit_duration_nominal"]
    a = [dev(torch, x, torch.float64) for x in (tau, d["pulse_length"], d["gain_correction"])]
    return lambda: ops.pulse_table_lookup(*a)


def b_sv_power(torch, ops, shape, dtype="float64", fill="rand", stats=True):
    raw = samples(torch, shape, torch.float32, 1, fill, scale=10.0, shift=-70.0)
    coef = power_rows(torch, *shape[:2])
    run = lambda: ops.sv_power(raw, coef, dtype=tdt(torch, dtype), want_range=True, want_range_stats=stats)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r[:2], "oracle.calibrate.cal_power_ek: a NaN sample gives NaN Sv and, masked, NaN range")


def b_sv_power_stats_only(torch, ops, shape, dtype):
    raw = samples(torch, shape, torch.float32, 1, scale=10.0, shift=-70.0)
    coef = power_rows(torch, *shape[:2])
    return lambda: ops.sv_power(raw, coef, dtype=tdt(torch, dtype), want_range=False, want_range_stats=True)


def b_range_power(torch, ops, shape, dtype="float64", fill="rand"):
    raw = samples(torch, shape, torch.float32, 2, fill)
    coef = power_rows(torch, *shape[:2])
    run = lambda: ops.range_power(raw, coef, dtype=tdt(torch, dtype))  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r], "oracle.calibrate: echo_range is NaN where the sample is")


def b_time_bin_offsets(torch, ops, P=9, n_bins=4, dt=2 * 10**9, closed="left"):
    t = dev(torch, ping_ns(P))
    t0 = int(ping_ns(1)[0])
    def check(out):  # the CSR offsets of np.searchsorted on the uniform edges (oracle.commongrid.bin_index's membership)
        edges = t0 + dt * np.arange(n_bins + 1)
        want = np.searchsorted(ping_ns(P), edges, side="left" if closed == "left" else "right")
        np.testing.assert_array_equal(host(out), want.astype(np.int32))

    return checked(lambda: ops.time_bin_offsets(t, t0, dt, n_bins, closed), check)


def bins_of(torch, P, per, n_tbins):
    """CSR offsets of ``n_tbins`` time bins of ``per`` pings each (the pings left over lie in no bin; bins past the last
    ping are empty)."""
    return dev(torch, np.minimum(np.arange(n_tbins + 1) * per, P).astype(np.int32))


def b_sv_mvbs_fused(torch, ops, shape=(2, 8, 65), dtype="float64", fill="rand", per=2, n_tbins=5, **kw):
    C, P, S = shape
    raw = samples(torch, shape, torch.float32, 3, fill, scale=10.0, shift=-70.0)
    coef = power_rows(torch, C, P)
    bs = bins_of(torch, P, per, n_tbins)
    kw = dict(dict(want_range=True, want_partials=True, want_range_stats=True), **kw)
    run = lambda: ops.sv_mvbs_fused(raw, coef, bs, n_tbins, FINE, 48, dtype=tdt(torch, dtype), **kw)  # noqa: E731
    if fill != "nan":
        return run
    return checked(run, lambda r: same(host(r["MVBS"]), binned_mean_ref(host(r["Sv"]), host(r["echo_range"]), P, per, n_tbins,
                                                                        FINE, 48), "MVBS"))


def b_sv_mvbs_fused_depth(torch, ops, shape=(2, 8, 64), dtype="float64", fill="rand", n_tbins=3):
    C, P, S = shape
    raw = samples(torch, shape, torch.float32, 14, fill, scale=10.0, shift=-70.0)
    coef = power_rows(torch, C, P)
    scale = torch.ones((C, P), dtype=torch.float64).cuda()
    offset = torch.full((C, P), 5.0, dtype=torch.float64).cuda()
    bs = bins_of(torch, P, 4, n_tbins)
    run = lambda: ops.sv_mvbs_fused_depth(raw, coef, scale, offset, bs, n_tbins, FINE, 60, dtype=tdt(torch, dtype),  # noqa: E731
                                          want_depth=True, want_partials=True)
    if fill != "nan":
        return run
    return checked(run, lambda r: same(host(r["MVBS"]), binned_mean_ref(host(r["Sv"]), host(r["depth"]), P, 4, n_tbins, FINE,
                                                                        60), "MVBS"))


def b_sv_mvbs_fused_i16(torch, ops, shape=(2, 8, 64), dtype="float64", empty_pings=False):
    C, P, S = shape
    g = np.random.default_rng(5)
    raw = dev(torch, g.integers(-12000, -2000, size=shape, dtype=np.int16))
    nv = np.full((C, P), S, dtype=np.int32)
    if C * P:
        nv[0, P // 2] = S // 2
    if empty_pings:
        nv[:] = 0
    nv = dev(torch, nv)
    coef = power_rows(torch, C, P)
    bs = bins_of(torch, P, 2, 5)
    run = lambda: ops.sv_mvbs_fused_i16(raw, nv, coef, bs, 5, FINE, 48, dtype=tdt(torch, dtype), want_partials=True,  # noqa: E731
                                        want_range_max=True)
    if not empty_pings:
        return run

    def check(r):  # no sample is recorded: Sv is NaN throughout, and groupby_mean of nothing is NaN
        assert np.isnan(host(r["Sv"])).all() and not host(r["cnt"]).any()
        same(host(r["MVBS"]), binned_mean_ref(host(r["Sv"]), np.zeros(shape), P, 2, 5, FINE, 48), "MVBS")

    return checked(run, check)


def b_mvbs(torch, ops, shape=(2, 8, 65), dtype="float64", fill="rand", by="range"):
    C, P, S = shape
    sv = sv_like(torch, shape, tdt(torch, dtype), 6, fill)
    bs = bins_of(torch, P, 2, 5)
    if by == "range":  # samples 0.3 m apart on bins of 0.5 m: two columns per range bin at the most
        rng = ramp(torch, shape, tdt(torch, dtype), 0.3)
        run = lambda: ops.mvbs(sv, bs, 5, 0.5, 40, want_partials=True, range=rng)  # noqa: E731
        if fill != "nan":
            return run
        return checked(run, lambda r: same(host(r["MVBS"]), binned_mean_ref(host(sv), host(rng), P, 2, 5, 0.5, 40), "MVBS"))
    coef = power_rows(torch, C, P)
    return lambda: ops.mvbs(sv, bs, 5, FINE, 48, want_partials=True, coef=coef)


def b_selftests(torch, ops, n=257, dtype="float64"):
    u = randn(torch, (n,), tdt(torch, dtype), 7, scale=30.0)
    x = u.abs() + 1e-3
    return lambda: (ops.selftest_lin_from_db(u), ops.selftest_log10(x), ops.selftest_log10(x, inline=True))


def b_selftest_correlate(torch, ops, dtype="complex64", fill="rand", tiles=1):
    g = torch.Generator().manual_seed(9)
    x = torch.randn((1, 2048), generator=g, dtype=getattr(torch, dtype)).cuda()
    rep = torch.randn(64, generator=g, dtype=torch.complex64).cuda()
    if fill == "nan":
        x = torch.full_like(x, complex(NAN, NAN))
        # a correlation of NaN tiles is NaN throughout (every output sums all 2048 samples of its tile)
        return checked(lambda: ops.selftest_correlate(x, rep), lambda out: np.isnan(host(out)).all() or pytest.fail("not NaN"))
    if tiles == 0:
        x = x[:0]
    return lambda: ops.selftest_correlate(x, rep)


def b_mvbs_finalize(torch, ops, shape=(2, 3, 65), dtype="float64", empty=False):
    ssum = randn(torch, shape, tdt(torch, dtype), 8, n_nan=0).abs()
    cnt = torch.zeros(shape, dtype=torch.int32).cuda() if empty else (torch.arange(int(np.prod(shape))) % 3).view(shape).int().cuda()
    def check(out):  # 10 log10(sum / count), the fill value where nothing was counted (commongrid/utils.py:92)
        with np.errstate(all="ignore"):
            n = host(cnt)
            want = np.where(n > 0, 10 * np.log10(host(ssum).astype(np.float64) / np.where(n > 0, n, 1)), np.nan)
        same(host(out), want.astype(host(out).dtype), "mvbs_finalize", 1e-9 if dtype == "float64" else 1e-5)

    return checked(lambda: ops.mvbs_finalize(ssum, cnt), check)


def b_affine_rows(torch, ops, shape=(2, 5, 65), dtype="float64", fill="rand"):
    x = samples(torch, shape, tdt(torch, dtype), 9, fill)
    sc, off = randn(torch, shape[:2], torch.float64, 10, n_nan=0), randn(torch, shape[:2], torch.float64, 11, n_nan=0)
    def check(out):
        hx = host(x)
        want = (host(off)[..., None] + host(sc)[..., None] * hx.astype(np.float64)).astype(hx.dtype)
        same(host(out), want, "affine_rows", 1e-15 if dtype == "float64" else 1e-6)

    return checked(lambda: ops.affine_rows(x, sc, off), check)


def b_depth_rows(torch, ops, shape=(2, 5, 260), dtype="float64", fill="rand", src="range"):
    C, P, S = shape
    sc, off = randn(torch, (C, P), torch.float64, 4, n_nan=0), randn(torch, (C, P), torch.float64, 5, n_nan=0)
    if src == "range":
        rng = samples(torch, shape, tdt(torch, dtype), 2, fill, scale=30.0, shift=100.0)

        def check(res):
            out, stats = res
            hx, ho = host(rng), host(out)
            want = (host(off)[..., None] + host(sc)[..., None] * hx.astype(np.float64)).astype(hx.dtype)
            same(ho, want, "depth", 1e-15 if dtype == "float64" else 1e-6)
            with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
                __import__("warnings").simplefilter("ignore")
                exp = [np.nanmin(ho), np.nanmax(ho), float(np.isnan(ho).sum())] if (ho == ho).any() else [NAN, NAN, float(ho.size)]
            same(host(stats), np.array(exp, dtype=np.float64), "depth statistics")

        return checked(lambda: ops.depth_rows(sc, off, range=rng), check)
    raw = samples(torch, shape, torch.float32, 3, fill)
    coef = power_rows(torch, C, P)
    run = lambda: ops.depth_rows(sc, off, coef=coef, mask_raw=raw, shape=shape, dtype=tdt(torch, dtype))  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r[:1], "consolidate.add_depth on an echo_range that is NaN where the sample is")


def b_nanminmax(torch, ops, n, dtype="float32", fill="rand", want=None):
    x = samples(torch, (n,), tdt(torch, dtype), 6, fill)

    def run():
        got = ops.nanminmax(x, with_nan_count=True)
        h = x.cpu().numpy()
        exp = (NAN, NAN) if not (h == h).any() else (float(np.nanmin(h)), float(np.nanmax(h)))
        assert _bits(list(got[:2])) == _bits(list(exp)) and got[2] == int(np.isnan(h).sum()), (got, exp)
        return got

    run.has_oracle = True  # (np.nanmin / np.nanmax, the reductions the wrapper stands for)
    return run


def b_mvbs_index(torch, ops, shape=(2, 7, 65), dtype="float64", fill="rand"):
    sv = sv_like(torch, shape, tdt(torch, dtype), 12, fill)
    rng = ramp(torch, shape, tdt(torch, dtype))
    def check(res):
        from oracle import commongrid as ogrid

        want, want_r = ogrid.compute_MVBS_index_binning(host(sv).astype(np.float64), host(rng).astype(np.float64), 7, 3)
        tol = 1e-10 if dtype == "float64" else 1e-5
        same(host(res[0]), want.astype(host(res[0]).dtype), "index binning", tol)
        same(host(res[1]), want_r.astype(host(res[1]).dtype), "echo_range block min", tol)

    return checked(lambda: ops.mvbs_index(sv, 3, 7, range=rng), check)


def noise_inputs(torch, shape, dtype, fill):
    C, P, S = shape
    sv = sv_like(torch, shape, tdt(torch, dtype), 13, fill)
    rng = ramp(torch, shape, tdt(torch, dtype), 0.5, 1.0)
    a2 = torch.full((C, P), 0.02, dtype=torch.float64).cuda()
    return sv, rng, a2


def b_noise(torch, ops, shape=(2, 7, 65), dtype="float64", fill="rand"):
    sv, rng, a2 = noise_inputs(torch, shape, dtype, fill)

    def run():
        nb, es, ec = ops.noise_estimate(sv, a2, 2, 2, range=rng, want_edges=True)
        return nb, es, ec, ops.noise_apply(sv, a2, nb, 2, 3.0, range=rng, want_minmax=True)

    if fill != "nan":
        return run

    def check(res):  # oracle.clean.remove_background_noise: no valid sample, no noise estimate, nothing corrected
        from oracle import clean as oclean

        exp_n, exp_c = oclean.remove_background_noise(host(sv).astype(np.float64), host(rng).astype(np.float64),
                                                      np.full(shape[0], 0.01), 2, 2, SNR_threshold="3.0dB")
        sn, sc, mm = res[3]
        same(host(sn), exp_n.astype(host(sn).dtype), "Sv_noise")
        same(host(sc), exp_c.astype(host(sc).dtype), "Sv_corrected")
        assert all(v != v for v in mm), mm

    return checked(run, check)


def b_noise_apply_rows(torch, ops, shape=(2, 7, 64), dtype="float64"):
    C, P, S = shape
    raw = randn(torch, shape, torch.float32, 15, scale=10.0, shift=-70.0)
    coef = power_rows(torch, C, P)
    a2 = torch.full((C, P), 0.02, dtype=torch.float64).cuda()

    def run():
        sv, _ = ops.sv_power(raw, coef, dtype=tdt(torch, dtype), want_range=False)
        nb = ops.noise_estimate(sv, a2, 2, 2, coef=coef)
        return ops.noise_apply(sv, a2, nb, 2, 3.0, coef=coef, mask_raw=raw, want_minmax=True)

    return run


def b_noise_finalize(torch, ops, rows=7, Sb=41, empty=False):
    g = np.random.default_rng(8)
    ssum = g.random((rows, Sb)) * 1e-7
    cnt = np.zeros((rows, Sb)) if empty else g.integers(0, 5, (rows, Sb)).astype(np.float64)
    s, c = dev(torch, ssum), dev(torch, cnt)
    def check(out):  # clean/api.py:402-422: mean -> dB -> min over the blocks -> the maximum where it is not below
        with np.errstate(all="ignore"):
            db = np.where(cnt > 0, 10 * np.log10(ssum / np.where(cnt > 0, cnt, 1.0)), np.nan)
            want = np.array([np.nanmin(r) if (r == r).any() else np.nan for r in db])
            want = np.where(want < -75.0, want, -75.0)
        same(host(out), want, "noise_finalize", 1e-13)

    return checked(lambda: ops.noise_finalize(s, c, -75.0), check)


def b_complex_coef(torch, ops, C=2, P=3, bb=True, nan=False):
    from echopype_amd import _lib

    val = dict(sample_interval=1e-4, tau_nominal=1e-3, transmit_power=1000.0, sound_speed=1500.0, absorption=0.01, gain=25.0,
               freq_center=70000.0, psi=-20.0, sa_correction=0.1, z_er=5400.0, z_et=75.0, angle_offset_alongship=0.1,
               angle_offset_athwartship=-0.1, beamwidth_alongship=7.0, beamwidth_athwartship=7.1)
    params = {k: torch.full((C,), NAN if nan else val[k], dtype=torch.float64).cuda() for k in _lib.CCP}
    tau = torch.full((C,), 9e-4, dtype=torch.float64).cuda()
    return lambda: ops.complex_coef_ek80(params, tau, C, P, B=4, bb=bb)


def complex_inputs(torch, shape, dtype, fill, seed=7):
    return (samples(torch, shape, tdt(torch, dtype), seed, fill), samples(torch, shape, tdt(torch, dtype), seed + 1, fill))


def b_range_complex(torch, ops, shape=(2, 3, 65, 4), dtype="float64", fill="rand"):
    re, _ = complex_inputs(torch, shape, "float32", fill)
    cc = complex_rows(torch, *shape[:2])
    run = lambda: ops.range_complex(re, cc, dtype=tdt(torch, dtype))  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r], "oracle.calibrate: echo_range is NaN where the first sector's sample is")


def b_sv_complex(torch, ops, shape=(2, 3, 2100, 4), dtype="float64", fill="rand", method="fft", indexed=False, cw=False):
    C, P, S, B = shape
    re, im = complex_inputs(torch, shape, "float32", fill)
    cc = complex_rows(torch, C, P)
    if cw:
        run = lambda: ops.sv_complex(re, im, cc, dtype=tdt(torch, dtype), want_prx=True, want_range_stats=True)  # noqa: E731
        if fill != "nan":
            return run
        return nan_in_nan_out(run, lambda r: [r["out"], r["prx"]], "oracle.calibrate.cal_complex_ek80: NaN sectors give NaN")
    taps = 64
    kw = dict(max_taps=taps, method=method, dtype=tdt(torch, dtype), want_prx=True)
    if indexed:
        rep, off = replicas(torch, 3, taps)
        kw["replica_id"] = dev(torch, (np.arange(C * P).reshape(C, P) % 3).astype(np.int32))
    else:
        rep, off = replicas(torch, C, taps)
    if method == "fft":
        kw["want_range_stats"] = True
    run = lambda: ops.sv_complex(re, im, cc, replica=rep, replica_off=off, **kw)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r["out"], r["prx"]], "oracle.calibrate.cal_complex_ek80: NaN sectors give NaN")


def b_splitbeam_power(torch, ops, shape=(2, 5, 65), planes="int8", dtype="float64"):
    g = np.random.default_rng(16)
    if planes == "int8":
        al, at = (dev(torch, g.integers(-128, 128, size=shape, dtype=np.int8)) for _ in range(2))
    else:
        al, at = (samples(torch, shape, torch.float32, 17 + i, planes) for i in range(2))
    prm = [torch.tensor(v, dtype=torch.float64).cuda() for v in (23.0, 23.0, 0.1, -0.2)]
    run = lambda: ops.splitbeam_power(al, at, prm, dtype=tdt(torch, dtype))  # noqa: E731
    if planes != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r, "splitbeam_ref.power_angles: NaN padding stays NaN")


def b_splitbeam_complex(torch, ops, shape=(2, 3, 2100, 4), method="fft", fill="rand", beam=(1, 1), dtype="float64"):
    C, P, S, B = shape
    re, im = complex_inputs(torch, shape, "float32", fill, 12)
    prm = [torch.tensor(v, dtype=torch.float64).cuda() for v in (23.0, 23.0, 0.1, -0.2)]
    if method == "cw":
        run = lambda: ops.splitbeam_complex(re, im, list(beam), prm, dtype=tdt(torch, dtype))  # noqa: E731
        if fill != "nan" and -1 not in beam:
            return run
        skipped = [c for c, b in enumerate(beam) if b == -1 or fill == "nan"]
        return nan_in_nan_out(run, lambda r: [t[skipped] for t in r], "splitbeam_ref.complex_angles: NaN rows for a skipped channel")
    rep, off = replicas(torch, C, 64)
    run = lambda: ops.splitbeam_complex(re, im, list(beam), prm, replica=rep, replica_off=off, max_taps=64, method=method,  # noqa: E731
                                        dtype=tdt(torch, dtype))
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r, "splitbeam_ref.complex_angles: NaN sectors give NaN angles")


def b_seafloor(torch, ops, P=6, S=40, dtype="float64", fill="rand", masked=True):
    r0, R = 5, 30
    th, ph = (samples(torch, (P, S), tdt(torch, dtype), 19 + i, fill, scale=3.0) for i in range(2))
    sv = sv_like(torch, (P, S), tdt(torch, dtype), 21, fill)
    depth0 = (0.5 * torch.arange(S, dtype=torch.float64)).cuda()
    tt = 4.0 if masked else 1e9  # (angle thresholds nothing reaches: an empty angle mask)

    def run():
        state = ops.seafloor_state(sv.device)
        mask = ops.seafloor_angle_mask(th, ph, r0, R, 3, 3, tt, tt, state)
        ops.seafloor_median(sv, r0, R, mask, state)
        parent = ops.seafloor_components(sv, r0, R, -72.0, mask, state)
        bottom = ops.seafloor_bottom(parent, mask, P, r0, depth0, 0.3, tdt(torch, dtype))
        none = ops.seafloor_bottom(None, None, P, r0, depth0, 0.3, tdt(torch, dtype))
        basic = ops.seafloor_basic(sv, 2, -75.0, -60.0, depth0, 0.5)
        # (which root names a component depends on the order of the unions: what is defined is which pixels have one)
        return mask, state[:8], parent >= 0, bottom, none, basic

    def check(res):  # (the basic line against tests/seafloor_ref.py; the Blackwell steps are held to it through the API row)
        import seafloor_ref as R

        same(host(res[5]), R.basic(host(sv), host(depth0), -75.0, -60.0, 2, 0.5), "bottom_basic")
        same(host(res[4]), np.full(P, host(depth0)[0] - 0.3).astype(host(res[4]).dtype), "nothing kept")

    return checked(run, check)


def b_shoal(torch, ops, P=8, S=16, dtype="float32", fill="rand", thr=0.0, connectivity=8):
    sv = samples(torch, (P, S), tdt(torch, dtype), 22, fill)
    idim = torch.arange(S + 1, dtype=torch.float64).cuda()
    jdim = torch.arange(P + 1, dtype=torch.float64).cuda()

    def run():
        state = ops.shoal_state(sv.device)
        filled = ops.shoal_threshold_fill(sv, thr, 1, 1)  # (Weill's gap filling; Echoview's candidates are the bare threshold)
        plane = ops.shoal_threshold_fill(sv, thr)
        parent, table = ops.shoal_label(plane, connectivity, state, with_groups=True)
        # (the component ids, and with them the values of parent and the table, come in no particular order: what is
        #  defined is which pixels carry a component)
        fg = parent < -1
        ops.shoal_echoview_link(plane, parent, table, idim, jdim, (1, 1), (2, 2), (2, 2), state)
        return filled, fg, plane, state[0]

    if connectivity != 8:
        return run

    def check(res):
        import shoal_ref as R

        h = host(sv)
        np.testing.assert_array_equal(host(res[0]), R.weill(h, thr, 1, 1, 0, 0))
        np.testing.assert_array_equal(host(res[2]), R.echoview(h, host(idim), host(jdim), thr, (1, 1), (2, 2), (2, 2)))

    return checked(run, check)


def b_transient(torch, ops, shape=(2, 6, 40), dtype="float64", fill="rand"):
    C, P, S = shape
    sv = sv_like(torch, shape, tdt(torch, dtype), 23, fill)
    chan = np.array([[5, 20, 2, 3], [4, 25, 1, 2]])[:C]
    rows = np.tile(np.arange(S) * 0.5, (C, 1))
    chan_i, chan_d = np.array([[2, 30], [3, 28]])[:C], np.array([[0.5, 19.5], [0.5, 19.5]])[:C]
    run = lambda: (ops.transient_fielding(sv, chan, 2, 3.0, 1.0, -40.0),  # noqa: E731
                   ops.transient_matecho(sv, rows, chan_i, chan_d, None, 2, 50.0, 3.0, 1, 1.0))
    if fill != "nan":
        return run
    # tests/transient_ref.py: an all-NaN layer is uncomputable, nothing is masked (True = valid everywhere)
    return checked(run, lambda r: [np.testing.assert_array_equal(host(m), np.ones(shape, dtype=bool)) for m in r])


def b_freq_diff(torch, ops, shape=(2, 5, 65), dtype="float64", fill="rand"):
    sv = sv_like(torch, shape, tdt(torch, dtype), 25, fill)
    def check(out):
        import freq_diff_ref as R

        np.testing.assert_array_equal(host(out), R.freq_diff(host(sv), 0, 1, ">=", 1.0))

    return checked(lambda: ops.freq_diff_mask(sv, 0, 1, ">=", 1.0), check)


def b_regrid_mask(torch, ops, shape=(1, 4, 8), all_false=False, n_tbins=1):
    g = torch.Generator().manual_seed(24)
    mask = (torch.rand(shape, generator=g) > (2.0 if all_false else 0.3)).to(torch.uint8).cuda()
    rng = torch.arange(shape[2], dtype=torch.float64).cuda()
    bs = bins_of(torch, shape[1], 4, n_tbins)
    def check(res):  # tests/regrid_mask_ref.py's rule: a cell is 1 where samples fall into it and all of them are 1
        m, r = host(mask).astype(bool), host(rng)
        start = host(bs)
        want = np.zeros((shape[0], n_tbins, 5), dtype=np.uint8)
        for k in range(n_tbins):
            for j in range(5):
                cols = (r >= 2.0 * j) & (r < 2.0 * (j + 1))
                cell = m[:, start[k]:start[k + 1]][:, :, cols]
                want[:, k, j] = cell.reshape(shape[0], -1).all(axis=1) & (cell[0].size > 0)
        np.testing.assert_array_equal(host(res[0]), want)
        assert int(res[1].item()) == 0

    return checked(lambda: ops.regrid_mask(mask, rng, bs, n_tbins, 2.0, 5), check)


def b_line_mask(torch, ops, shape=(2, 5, 65), dtype="float64", fill="rand", lazy=False):
    C, P, S = shape
    up = dev(torch, np.full((C, 1), 3.0))
    lo = dev(torch, np.linspace(10.0, 20.0, C * P).reshape(C, P))
    if fill == "nan_line":
        lo = nans(torch, (C, P), torch.float64)
    if lazy:
        raw = samples(torch, shape, torch.float32, 26)
        coef = power_rows(torch, C, P)
        return lambda: ops.line_mask(shape, coef=coef, nan_raw=raw, dtype=tdt(torch, dtype), upper=up, lower=lo)
    rng = ramp(torch, shape, tdt(torch, dtype)) if fill != "nan" else nans(torch, shape, tdt(torch, dtype))

    def check(out):
        from line_mask_ref import line_mask_ref

        np.testing.assert_array_equal(host(out), line_mask_ref(host(rng), upper=host(up), lower=host(lo)))

    return checked(lambda: ops.line_mask(shape, range=rng, upper=up, lower=lo), check)


def b_regrid_rows(torch, ops, shape=(2, 3, 65), dtype="float64", fill="rand", n_rbins=9):
    sv = sv_like(torch, shape, tdt(torch, dtype), 27, fill)
    rng = ramp(torch, shape[2:], tdt(torch, dtype), 0.5, 0.1)
    run = lambda: ops.regrid_rows(sv, rng, 4.0, n_rbins)  # noqa: E731
    if fill != "nan" and shape[1] and n_rbins:
        return run

    def check(res):
        from regrid_ref import regrid_ref
        from test_gpu_regrid import _judge

        want_sv, want_cov, bad = regrid_ref(host(sv), host(rng), np.arange(n_rbins + 1) * 4.0)
        _judge(host(res[0]), want_sv, "regrid Sv")
        _judge(host(res[1]), want_cov, "regrid coverage")
        assert int(res[2].item()) == bad

    return checked(run, check)


def b_window_filter(torch, ops, shape=(2, 18, 73), dtype="float64", fill="rand", method="median"):
    x = sv_like(torch, shape, tdt(torch, dtype), 28, fill)
    run = lambda: ops.window_filter(x, method, 3, 5, min_valid=2)  # noqa: E731
    if fill != "nan":
        return run

    def check(out):
        from window_filter_ref import window_filter_ref

        same(host(out), window_filter_ref(host(x), method, 3, 5, min_valid=2).astype(host(x).dtype), "window_filter")

    return checked(run, check)


def b_echo_metrics(torch, ops, R=5, S=65, dtype="float64", fill="rand"):
    sv = sv_like(torch, (R, S), tdt(torch, dtype), 29, fill)
    rng = ramp(torch, (S,), tdt(torch, dtype), 0.5, 1.0)
    run = lambda: ops.echo_metrics(sv, rng)  # noqa: E731
    if fill != "nan":
        return run

    def check(out):
        import metrics_ref

        want, _ = metrics_ref.rows(host(sv), host(rng))
        for k, v in out.items():
            same(host(v), np.asarray(want[k]).astype(host(v).dtype), k)

    return checked(run, check)


def b_align(torch, ops, N=7, P=65, method="linear", nat=False):
    t = dev(torch, ping_ns(N, 10 * 10**9))
    y = randn(torch, (2, N), torch.float64, 30, n_nan=0)
    pt = ping_ns(P) - 5 * 10**9
    if nat:
        pt[:] = np.iinfo(np.int64).min
    pt = dev(torch, pt)
    run = lambda: ops.align_to_ping_time(t, y, pt, method)  # noqa: E731
    if not nat:
        return run
    # tests/location_ref.py: a NaT ping has no position
    return checked(run, lambda out: np.testing.assert_array_equal(np.isnan(host(out)), np.ones((2, P), dtype=bool)))


def b_time_rebuild(torch, ops, N):
    t = torch.arange(N, dtype=torch.int64) * 1000
    t[N // 2:] -= 5000  # one reversal
    t = t.cuda()

    def run():
        facts, lst = ops.time_reversals(t, want_list=True)
        sub = ops.reversal_medians(t, facts, lst, 5)
        count = int(facts[1].item())
        # (the list holds `count` indices in no particular order, and sub is written at those indices only)
        idx = torch.sort(lst[:count]).values
        return facts, idx, sub[idx], ops.time_rebuild(t, facts, torch.full((N - 1,), 1000, dtype=torch.int64).cuda())

    return run


def b_time_reversals_none(torch, ops, N=65):
    t = (torch.arange(N, dtype=torch.int64) * 1000).cuda()
    def check(facts):
        import qc_ref

        assert not qc_ref.exist_reversed(host(t)) and host(facts).tolist() == [-1, 0, 0, 0]

    return checked(lambda: ops.time_reversals(t, want_list=False)[0], check)


def b_one_time(torch, ops, entry):
    """One time stamp: no difference to look at, to take a median of or to rebuild."""
    from echopype_amd import _lib

    t = torch.tensor([1000], dtype=torch.int64).cuda()
    facts = torch.tensor([-1, 0, 0, 0], dtype=torch.int64).cuda()
    assert facts.numel() == _lib.QC_FACTS
    none = torch.zeros(1, dtype=torch.int64).cuda()[:0]
    if entry == "time_reversals":
        return checked(lambda: ops.time_reversals(t, want_list=True)[0],
                       lambda facts: host(facts).tolist() == [-1, 0, 0, 0] or pytest.fail(str(host(facts))))
    if entry == "reversal_medians":
        return lambda: ops.reversal_medians(t, facts, none, 5, none)
    return lambda: ops.time_rebuild(t, facts, none)


def b_concat_rows(torch, ops, dtype="float32", widths=(5, 65), P=(2, 3), beams=None):
    g = np.random.default_rng(31)
    tail = () if beams is None else (beams,)
    srcs = [dev(torch, g.standard_normal((2, p, w) + tail).astype(dtype) if dtype.startswith("f") else
                g.integers(-100, 100, (2, p, w) + tail).astype(dtype)) for p, w in zip(P, widths)]
    return lambda: ops.concat_rows(srcs, chan_maps=[[0, 1], [1, 0]])


def raw_file(C, P, S, short=True):
    """A byte buffer with an int16 power block and an int8 angle-pair block per (channel, ping), at odd offsets."""
    g = np.random.default_rng(32)
    parts, table, pos = [b"\x55" * 3], [], 3
    for i in range(C * P):
        count = S if not short or i % 3 else S // 2
        table.append((pos, pos + 2 * count, count))
        parts.append(g.integers(0, 256, 4 * count + 1, dtype=np.uint8).tobytes())
        pos += 4 * count + 1
    if short and C * P:
        table[0] = (table[0][0], -1, table[0][2])  # a row without an angle block
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(table, dtype=np.int64).reshape(-1, 3)


def b_raw0_unpack(torch, ops, C=2, P=3, S=65, angles="float32", empty=False):
    buf, table = raw_file(C, P, S, short=angles != "int8")
    if empty:  # no row has a sample or an angle block: what open_raw's restatement (tests/raw_cases.py) pads with NaN
        table[:, 1], table[:, 2] = -1, 0
    file_bytes, n = ops.upload_file_bytes(buf)
    run = lambda: ops.raw0_unpack(file_bytes, table, C, P, S, angles, n_bytes=n)  # noqa: E731
    return nan_in_nan_out(run, lambda r: r, "raw_cases.expected: NaN behind the recorded count") if empty else run


def b_nmea(torch, ops, n=None):
    import nmea_cases as K

    sentences = [h[1] for h in K.HAND][:n]
    buf, table = K.lay_out(sentences) if sentences else (np.zeros(16, np.uint8), np.zeros((0, 2), np.int64))
    file_bytes, nb = ops.upload_file_bytes(buf)
    return lambda: ops.nmea_positions(file_bytes, table, n_bytes=nb)


def b_range_bin_smooth(torch, ops, shape=(2, 5, 65), dtype="float64", fill="rand", value=False):
    sv = sv_like(torch, shape, tdt(torch, dtype), 33, fill)
    if value:
        rng = ramp(torch, shape, tdt(torch, dtype), 0.5, 1.0)
        return lambda: ops.range_bin_smooth(sv, range=rng, r0=1.0, bin=5.0, nbins=7)
    run = lambda: ops.range_bin_smooth(sv, nper=4)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r], "oracle.masks.index_binning_downsample_upsample: the mean of no sample is NaN")


def b_impulse_mask(torch, ops, shape=(2, 5, 65), dtype="float64", fill="rand"):
    up = sv_like(torch, shape, tdt(torch, dtype), 34, fill)
    run = lambda: ops.impulse_mask(up, 1, 10.0)  # noqa: E731
    if fill != "nan":
        return run
    def check(out):  # (a difference that is NaN counts as exceeding the threshold there: clean/utils.py:307-323)
        from oracle import masks as omask

        h = host(up).astype(np.float64)
        want = np.stack([omask.echopy_impulse_noise_mask(h[c].T, 1, 10.0).T for c in range(shape[0])])
        np.testing.assert_array_equal(host(out).astype(bool), want)

    return checked(run, check)


def b_pool_sv(torch, ops, shape=(2, 6, 40), dtype="float64", fill="rand", func="nanmean", first=2):
    sv = sv_like(torch, shape, tdt(torch, dtype), 17, fill)
    run = lambda: ops.pool_sv(sv, first, 1, 2, func=func, threshold=3.0)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r, "oracle.masks.index_binning_pool_Sv: pooled NaN, and Sv - pooled > threshold nowhere")


def b_pool_sv_value(torch, ops, shape=(2, 6, 40), dtype="float64", fill="rand", func="nanmean", ragged=False):
    C, P, S = shape
    sv = sv_like(torch, shape, tdt(torch, dtype), 17, fill)
    rng = ramp(torch, shape, tdt(torch, dtype))
    if ragged:  # the pings of channel 1 differ in their range vectors: the run tables and the staged kernels
        rng[1] *= (1.0 + 0.01 * torch.arange(P, dtype=rng.dtype, device=rng.device))[:, None]
        rng[0, 1, S - 7:] = NAN

    def run():
        nvalid, bad = ops.range_rows_check(rng)
        assert bad == 0
        return nvalid, ops.pool_sv_value(sv, rng, nvalid, 2.0, 1, 1.0, 0.0, 19.5, func=func, threshold=3.0)

    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r[1], "oracle.masks.pool_Sv: pooled NaN, and Sv - pooled > threshold nowhere")


def b_attenuated(torch, ops, shape=(2, 6, 40), dtype="float64", fill="rand"):
    sv = sv_like(torch, shape, tdt(torch, dtype), 35, fill)
    rng = ramp(torch, shape, tdt(torch, dtype))
    run = lambda: ops.attenuated_mask(sv, rng, 5.0, 12.0, 2, -4.0)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r], "oracle.masks.echopy_attenuated_signal_mask: a NaN median difference flags nothing")


def b_apply_mask(torch, ops, n=1000, dtype="float32", fill="rand", keep="some", array_fill=False, empty="fresh"):
    src = samples(torch, (n,), tdt(torch, dtype), 15, fill)
    k = torch.arange(max(n, 1))[:n]
    mask = {"some": k % 3 != 0, "none": k < 0, "all": k >= 0}[keep].to(torch.uint8).cuda()
    if n == 0 and empty == "view":  # the first none of a longer tensor (torch still hands it over as NULL) under a live mask
        src = samples(torch, (8,), tdt(torch, dtype), 15)[:0]
        mask = torch.ones(4, dtype=torch.uint8).cuda()
    fa = samples(torch, (n,), tdt(torch, dtype), 16, n_nan=0) if array_fill else None

    def run():
        one = ops.apply_mask(src, mask, -999.0 if not array_fill else NAN, fa) if n else None
        out, mm = ops.apply_masks(src, [mask, mask], fill_value=NAN, fill_array=fa, want_minmax=True)
        h = out.cpu().numpy()
        exp = [NAN, NAN] if not (h == h).any() else [float(np.nanmin(h)), float(np.nanmax(h))]
        assert _bits(mm.cpu().tolist()) == _bits(exp), (mm.cpu().tolist(), exp)
        m = host(mask).astype(bool)
        from oracle import masks as omask

        if m.size == h.size:
            np.testing.assert_array_equal(h, omask.apply_mask(host(src), [m, m]) if fa is None else np.where(m, host(src), host(fa)))
        return one, out, mm, ops.mask_and(mask, mask) if n else None

    run.has_oracle = True
    return run


def b_range_step_mean(torch, ops, shape=(2, 3, 17), dtype="float64", fill="rand"):
    rng = samples(torch, shape, tdt(torch, dtype), 16, fill)
    def check(out):  # the per-channel nanmean of the sample-to-sample step (clean/utils.py): NaN where there is none
        import warnings

        h = host(rng).astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.nanmean(np.diff(h, axis=2).reshape(shape[0], -1), axis=1) if shape[2] > 1 else np.full(shape[0], np.nan)
        same(out, want, "range_step_mean", 1e-6)

    return checked(lambda: ops.range_step_mean(rng), check)


def b_first_not_le(torch, ops, n=65, fill="rand"):
    x = samples(torch, (n,), torch.float64, 36, fill, n_nan=0).abs()
    def check(out):
        h = host(x)
        bad = np.flatnonzero(~(h <= 0.5))
        assert out == (int(bad[0]) if bad.size else h.size)

    return checked(lambda: ops.first_not_le(x, 0.5), check)


def b_geodesic(torch, ops, P=65, nan=False):
    lat = nans(torch, (P,), torch.float64) if nan else dev(torch, 45.0 + 1e-4 * np.arange(P))
    lon = dev(torch, -125.0 + 2e-4 * np.arange(P))
    def check(out):
        from oracle import nasc as onasc

        la, lo = host(lat), host(lon)
        want = np.full(P, np.nan)
        for i in range(P - 1):
            if la[i] == la[i] and la[i + 1] == la[i + 1]:
                want[i] = onasc.geodesic_m(la[i], lo[i], la[i + 1], lo[i + 1])
        same(host(out), want, "geodesic_steps", 1e-9)

    run = lambda: ops.geodesic_steps(lat, lon)  # noqa: E731
    return checked(run, check) if nan or P == 1 else run


def b_nasc(torch, ops, shape=(2, 7, 33), dtype="float64", fill="rand", range_bin=1.5, n_rbins=24):
    C, P, S = shape
    sv = sv_like(torch, shape, tdt(torch, dtype), 18, fill)
    depth = ramp(torch, shape, tdt(torch, dtype), 1.0)
    # one ping per distance bin and depths a metre apart on bins of 1.5 m: a cell sums at most two partials, in either
    # order the same bits; the pings behind the third bin lie in no bin, the fourth bin has no ping
    bs = bins_of(torch, min(P, 3), 1, 4)
    run = lambda: ops.nasc(sv, depth, bs, 4, range_bin, n_rbins, want_parts=True)  # noqa: E731
    if fill != "nan":
        return run

    def check(res):  # oracle.nasc.compute_raw_NASC with the ping number as distance (the pings behind bin 2 lie outside)
        from oracle import nasc as onasc

        dist = np.where(np.arange(P) < 3, np.arange(P, dtype=np.float64), 1e6)
        want, _ = onasc.compute_raw_NASC(host(sv).astype(np.float64), host(depth).astype(np.float64), dist,
                                         np.arange(P).astype("datetime64[s]"), np.arange(n_rbins + 1) * range_bin,
                                         np.arange(5, dtype=np.float64))
        same(host(res[0]), want.astype(host(res[0]).dtype), "NASC")

    return checked(run, check)


def b_sv_noise_fused(torch, ops, shape=(2, 8, 64), dtype="float64", fill="rand"):
    C, P, S = shape
    raw = samples(torch, shape, torch.float32, 37, fill, scale=10.0, shift=-70.0)
    coef = power_rows(torch, C, P)
    a2 = torch.full((C, P), 0.02, dtype=torch.float64).cuda()
    run = lambda: ops.sv_noise_fused(raw, coef, a2, 2, 2, dtype=tdt(torch, dtype), want_range=True, want_range_max=True,  # noqa: E731
                                     want_range_stats=True, want_edges=True)
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: r[:3], "oracle.calibrate / oracle.clean.estimate_background_noise: no sample, no noise")


def b_denoise_mvbs(torch, ops, shape=(2, 8, 64), dtype="float64", fill="rand", raw_route=False):
    C, P, S = shape
    a2 = torch.full((C, P), 0.02, dtype=torch.float64).cuda()
    bs = bins_of(torch, P, 2, 5)
    noise = torch.full((C, -(-P // 2)), -140.0, dtype=torch.float64).cuda()
    if raw_route:
        raw = samples(torch, shape, torch.float32, 38, fill, scale=10.0, shift=-70.0)
        coef = power_rows(torch, C, P)
        run = lambda: ops.sv_denoise_mvbs(raw, coef, a2, noise, 2, 3.0, bs, 5, FINE, 48, dtype=tdt(torch, dtype),  # noqa: E731
                                          want_noise=True, want_range=True, want_partials=True, want_minmax=True)
        if fill != "nan":
            return run
        return nan_in_nan_out(run, lambda r: [r["MVBS"], r["Sv_corrected"], r["echo_range"]],
                              "oracle.clean.remove_background_noise then oracle.commongrid.groupby_mean of nothing")
    sv, rng, _ = noise_inputs(torch, shape, dtype, fill)
    # (samples 0.5 m apart on bins of 0.75 m)
    run = lambda: ops.denoise_mvbs(sv, a2, noise, 2, 3.0, bs, 5, 0.75, 45, range=rng, want_noise=True, want_partials=True)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r["MVBS"], r["Sv_corrected"]],
                          "oracle.clean.remove_background_noise then oracle.commongrid.groupby_mean of nothing")


def b_edge_gather(torch, ops, typed=None, n_edges=2):
    buf = randn(torch, (4, 2, 2, 5), torch.float64, 39, n_nan=0).abs()
    off = dev(torch, np.array([0, 2, 3][:n_edges + 1], dtype=np.int32))
    slots = dev(torch, np.array([0, 3, 1], dtype=np.int32))
    return lambda: ops.edge_gather(buf, off, slots, n_edges, typed=None if typed is None else tdt(torch, typed))


def b_target_spectra(torch, ops, dtype="float64", rows="all"):
    """The fixture table of the feature's own tests: whole echoes next to rows with NaN angles, windows in the NaN tail,
    non-positive ranges and indices outside the cube."""
    import target_spectra_cases as K
    import test_gpu_target_spectra as T

    _, reps, echoes = K.scene(4, "float32")
    full = K.table(echoes, reps)
    tab = {k: v[:0] for k, v in full.items()} if rows == "none" else full
    return lambda: T._run((torch, ops), 4, "float32", 16, 41, out_dtype=dtype, tab=tab)


def b_sv_spectrum(torch, ops, dtype="float64", fill="rand"):
    import test_gpu_sv_spectrum as T

    args, kw = T._args((torch, ops), 4, "float32", 16, 23, 41, "rectangular", True)
    if fill == "nan":
        args[0], args[1] = torch.full_like(args[0], NAN), torch.full_like(args[1], NAN)
    run = lambda: ops.sv_spectrum(*args, dtype=dtype, **kw)  # noqa: E731
    if fill != "nan":
        return run
    return nan_in_nan_out(run, lambda r: [r[0]], "sv_spectrum_ref: a cell with a NaN sample is NaN")


# ---- the public API: builders of closures that return comparable dictionaries ----------------------------------------------
def _plain(v):
    if isinstance(v, (bool, int, float, np.integer, np.floating)):
        return _bits(float(v))
    if isinstance(v, (list, tuple)) and all(isinstance(x, (bool, int, float, np.integer, np.floating)) for x in v):
        return _bits([float(x) for x in v])
    if isinstance(v, np.ndarray) and v.dtype.kind in "fiub":
        return _bits(v)
    return None  # (strings: histories carry the time of the call)


def ds_bits(obj):
    """A Dataset / DataArray / tuple of them as something ``==`` compares bit for bit: values, dtypes, dims, numeric
    attributes (``actual_range`` among them)."""
    if isinstance(obj, (tuple, list)):
        return [ds_bits(o) for o in obj]
    if hasattr(obj, "data_vars"):
        out = {"attrs": {k: _plain(v) for k, v in dict(obj.attrs).items() if _plain(v) is not None}}
        for k, v in list(obj.data_vars.items()) + list(obj.coords.items()):
            out[k] = ds_bits(v)
        return out
    if hasattr(obj, "dims") and hasattr(obj, "values"):
        a = np.asarray(obj.values)
        body = a.tolist() if a.dtype == object else np.ascontiguousarray(a).tobytes()
        return (tuple(obj.dims), str(a.dtype), a.shape, body,
                {k: _plain(v) for k, v in dict(obj.attrs).items() if _plain(v) is not None})
    a = np.asarray(obj)
    return (str(a.dtype), a.shape, a.tolist() if a.dtype == object else np.ascontiguousarray(a).tobytes())


DIMS = ("channel", "ping_time", "range_sample")
T0 = np.datetime64("2024-03-01T00:00:00", "ns")


def lite_ds(ep, torch, sv, depth, on_device=True, range_name="depth"):
    C, P, S = sv.shape
    ds = ep.Dataset(coords={"channel": np.array([f"ch_{i}" for i in range(C)]),
                            "ping_time": T0 + np.arange(P) * np.timedelta64(1, "s"), "range_sample": np.arange(S)})
    wrap = (lambda a: ep.DeviceArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())) if on_device else (lambda a: a)
    ds["Sv"] = ep.DataArray(wrap(sv), DIMS, name="Sv")
    ds[range_name] = ep.DataArray(wrap(depth), DIMS, name=range_name)
    return ds


def api(fn):
    """A builder of the table from ``fn(ep, torch)`` -> closure that returns Datasets / DataArrays."""
    def build(torch, ops):
        import echopype_amd as ep

        run = fn(ep, torch)
        out = lambda: ds_bits(run())  # noqa: E731
        out.has_oracle = getattr(run, "has_oracle", False)
        return out

    return build


def a_apply_mask(variant):
    def fn(ep, torch):
        from test_gpu_masks import _scene

        sv, depth = _scene(3, 25, 80, 30)
        g = np.random.default_rng(1)
        keep = g.random((25, 80)) < 0.8
        if variant == "all_masked":
            keep[:] = False
        if variant == "all_nan":
            sv[:] = np.nan
        if variant == "empty_fresh":  # no pings: source and mask hold no element (and no pointer)
            sv, depth, keep = sv[:, :0], depth[:, :0], keep[:0]
        ds = lite_ds(ep, torch, sv, depth)
        if variant == "empty_view":  # no channels: an empty view of a resident cube, under a (ping_time, range_sample) mask
            full = torch.from_numpy(sv).cuda()
            ds = ep.Dataset(coords={"channel": np.array([], dtype="<U4"), "ping_time": ds.coords["ping_time"],
                                    "range_sample": np.arange(80)})
            ds["Sv"] = ep.DataArray(ep.DeviceArray(full[:0]), DIMS, name="Sv")
        mask = ep.DataArray(keep, DIMS[1:])

        def run():
            out = ep.mask.apply_mask(ds, mask)
            lo, hi = out["Sv"].attrs["actual_range"]
            h = np.asarray(out["Sv"].values)
            want = [NAN, NAN] if not (h == h).any() else [round(float(np.nanmin(h)), 2), round(float(np.nanmax(h)), 2)]
            assert _bits([float(lo), float(hi)]) == _bits(want), ("actual_range", [lo, hi], want)
            from oracle import masks as omask

            np.testing.assert_array_equal(h, omask.apply_mask(np.asarray(ds["Sv"].values), [keep]))
            return out

        run.has_oracle = True
        return run

    return api(fn)


def survey(ep, C=2, P=40, S=120):
    """An EK60 file with split-beam angles, a seabed band and a navigation track; fresh datasets on every call."""
    from echopype_amd import echodata, synth
    from echopype_amd.echodata import BEAM1

    d = synth.ek60_seafloor_numpy(C=C, P=P, S=S, band_top=S - 30)
    ed = echodata.from_ek60_arrays(d)
    pt = np.asarray(ed[BEAM1]["ping_time"].values)
    t = np.linspace(pt[0].astype(np.int64) + 10**9, pt[-1].astype(np.int64) - 10**9, 11).astype(np.int64)
    lat, lon = 45.0 + 4.5e-5 * (t - t[0]) / 1e9, -125.0 + 1.5e-5 * (t - t[0]) / 1e9
    plat = ep.Dataset()
    tt = t.astype("datetime64[ns]")
    plat["latitude"] = ep.DataArray(lat, ("time1",), {"time1": tt}, {"standard_name": "latitude"})
    plat["longitude"] = ep.DataArray(lon, ("time1",), {"time1": tt}, {"standard_name": "longitude"})
    ed["Platform"] = plat

    def fresh(depth=True, **kw):
        ds = ep.calibrate.compute_Sv(ed, **kw)
        return ep.consolidate.add_depth(ds) if depth else ds

    return d, ed, fresh


def a_noise(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)
        # (blocks of two samples: two column sums per block, see FINE)
        return lambda: ep.clean.remove_background_noise(fresh(False, dtype=variant), 4, 2, background_noise_max="-125.0dB",
                                                        SNR_threshold="3.0dB")

    return api(fn)


def a_mvbs(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)
        # the samples lie 0.192 m apart: range bins of 0.3 m take two columns at the most (see FINE)
        if variant == "fused":
            return lambda: ep.compute_Sv_MVBS(ed, range_bin="0.3m", ping_time_bin="4s")
        if variant == "depth":
            return lambda: ep.commongrid.compute_MVBS(fresh(), range_var="depth", range_bin="0.3m", ping_time_bin="4s")
        if variant == "index":
            return lambda: ep.commongrid.compute_MVBS_index_binning(fresh(False), range_sample_num=7, ping_num=3)
        return lambda: ep.commongrid.compute_MVBS(fresh(False), range_bin="0.3m", ping_time_bin="4s")

    return api(fn)


def a_nasc(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)
        # 0.002 nmi (3.7 m) at about 5 m/s and a ping a second: one ping per distance bin; depths 0.192 m apart on bins
        # of 0.3 m: two partials per cell at the most
        return lambda: ep.commongrid.compute_NASC(ep.consolidate.add_location(fresh(), ed), range_bin="0.3m", dist_bin="0.002nmi")

    return api(fn)


def a_location_angles(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)

        def run():
            ds = fresh()
            for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
                      "angle_offset_athwartship"):
                if k not in ds:
                    ds[k] = (("channel",), d[k])
            return ep.consolidate.add_splitbeam_angle(ep.consolidate.add_location(ds, ed), ed, "CW", "power", to_disk=False)

        return run

    return api(fn)


def a_seafloor(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)

        def run():
            ds = fresh()
            for k in ("angle_sensitivity_alongship", "angle_sensitivity_athwartship", "angle_offset_alongship",
                      "angle_offset_athwartship"):
                if k not in ds:
                    ds[k] = (("channel",), d[k])
            ds = ep.consolidate.add_splitbeam_angle(ds, ed, "CW", "power", to_disk=False)
            ch = str(np.asarray(ds["channel"].values)[1])
            bw = ep.mask.detect_seafloor(ds, "blackwell", {"var_name": "Sv", "channel": ch, "threshold": (-70.0, 1.0137, 0.6173),
                                                           "r0": 0, "r1": 1e6, "wtheta": 11, "wphi": 15})
            basic = ep.mask.detect_seafloor(ds, "basic", {"var_name": "Sv", "channel": ch, "threshold": (-60.0, 100.0),
                                                          "bin_skip_from_surface": 10})
            water = ep.mask.line_mask(ds, upper="2m", lower=basic, lower_offset=-0.5)
            return bw, basic, water, ep.mask.apply_mask(ds, water)

        return run

    return api(fn)


def a_shoal(variant):
    def fn(ep, torch):
        d, ed, fresh = survey(ep)

        def run():
            ds = fresh(False)
            ch = str(np.asarray(ds["channel"].values)[1])
            sv = np.asarray(ds["Sv"].values)[1]
            thr = float(np.nanpercentile(sv, 80)) if variant != "nothing" else 1e9
            med = ep.clean.window_filter(ds, "median", 3, 3)
            mw = ep.mask.detect_shoal(med, "weill", {"var_name": "Sv", "channel": ch, "thr": thr, "maxvgap": 2, "maxhgap": 1,
                                                     "minvlen": 3, "minhlen": 2})
            idim, jdim = np.arange(sv.shape[1] + 1) * 0.2, np.arange(sv.shape[0] + 1) * 1.0
            me = ep.mask.detect_shoal(ds, "echoview", {"var_name": "Sv", "channel": ch, "idim": idim, "jdim": jdim, "thr": thr,
                                                       "mincan": (0.4, 2.0), "maxlink": (0.4, 2.0), "minsho": (1.0, 4.0)})
            import shoal_ref as R

            np.testing.assert_array_equal(mw.values, R.weill(np.asarray(med["Sv"].values)[1], thr, 2, 1, 3, 2))
            np.testing.assert_array_equal(me.values, R.echoview(sv, idim, jdim, thr, (0.4, 2.0), (0.4, 2.0), (1.0, 4.0)))
            return med["Sv"], mw, me

        run.has_oracle = True
        return run

    return api(fn)


def a_regions(variant):
    def fn(ep, torch):
        from test_gpu_masks import _scene

        sv, depth = _scene(2, 25, 80, 33)
        # regions of two pixels, apart from one another: the float64 sums of a region are two atomics at the most
        mask = np.zeros(sv.shape[1:], dtype=bool)
        if variant != "nothing":
            mask[::3, 0::4] = mask[::3, 1::4] = True

        def run():
            ds = lite_ds(ep, torch, sv, depth)
            import region_ref as R

            lab = ep.mask.label_regions(ep.DataArray(mask, DIMS[1:]))
            want = R.label(mask, 8)
            np.testing.assert_array_equal(lab.values, want[0] if isinstance(want, tuple) else want)
            return lab, ep.mask.region_statistics(ds, ep.DataArray(mask, DIMS[1:]))

        run.has_oracle = True
        return run

    return api(fn)


def a_transient(variant):
    def fn(ep, torch):
        from test_gpu_transient import _scene_ds

        ds, _ = _scene_ds(C=2, P=70, S=420)
        f = dict(range_var="depth", r0=900, r1=1000, n=10, thr=(3, 1), roff=20, jumps=5, maxts=-35, start=0)
        m = dict(range_var="depth", start_depth=220, window_meter=450, window_ping=20, percentile=25, extend_ping=1,
                 min_window=20, delta_db=8)
        return lambda: (ep.clean.detect_transient(ds, "fielding", f), ep.clean.detect_transient(ds, "matecho", m))

    return api(fn)


def a_regrid(variant):
    def fn(ep, torch):
        from regrid_cases import volume
        from test_gpu_regrid import _dataset

        sv, r = volume(29, 3, 4, 130, np.float32 if variant == "float32" else np.float64, np.float64)

        def run():
            ds = _dataset(torch, sv, r)
            rg = ep.commongrid.regrid_Sv(ds, range_bin="0.2m")
            return rg, ep.mask.frequency_differencing(rg, freqABEq="200kHz - 38kHz >= 5dB")

        return run

    return api(fn)


def a_regrid_mask(variant):
    def fn(ep, torch):
        from test_gpu_regrid_mask import _arrays

        P, D = 70, 50
        g = np.random.default_rng(61)
        mask = g.random((P, D)) < (0.95 if variant != "nothing" else -1.0)
        ping = np.int64(T0.astype(np.int64)) + 10**9 * np.arange(P)
        m, r = _arrays(mask, ping, np.arange(D) * 1.0, device=True)

        def run():
            import regrid_mask_ref as R

            out = ep.mask.regrid_mask(m, r, range_bin="5m", ping_time_bin="20s")
            want = R.regrid(mask[None], ping, np.arange(D) * 1.0, 5.0, 20 * 10**9)[3]
            np.testing.assert_array_equal(np.asarray(out.values), want[0])
            return out

        run.has_oracle = True
        return run

    return api(fn)


def a_metrics(variant):
    def fn(ep, torch):
        import metrics_cases as K
        from test_gpu_metrics import dataset

        kind = {"base": "clean", "all_neg_inf": "all_neg_inf", "range_nan": "range_nan"}[variant]
        sv, r = K.make(kind, (2, 5), 65, np.float64)

        def run():
            import metrics_ref

            out = ep.metrics.summary(dataset({"Sv": sv, "echo_range": r}))
            want, _ = metrics_ref.rows(sv, r)
            for k in K.STATS:  # (float64: the project's 1e-9 bar; the NaN and infinity patterns are the reference's)
                same(np.asarray(out[k].values), np.asarray(want[k]), k, 1e-9)
            return out

        run.has_oracle = True
        return run

    return api(fn)


def a_targets(variant, dtype="float64"):
    def fn(ep, torch):
        import single_target_cases as K
        from test_gpu_single_target import _dataset, _params

        S = {"tile": K.TILE + 1, "tile_less_one": K.TILE - 1, "none": 65}[variant]
        d = K.scene(S, dtype)
        prm = _params(d)
        if variant == "none":
            prm = dict(prm, TS_threshold=1e9)  # nothing is a candidate: no target in any channel or ping
        track = {"gate_alongship": 5.0, "gate_athwartship": 5.0, "gate_range": 1.0, "min_targets": 2, "min_pings": 2}

        def run():
            table = ep.targets.detect_single_targets(_dataset(d), "split_beam", prm)
            if variant == "none":  # single_target_ref.candidates: no sample reaches the threshold, so no target and no track
                assert table["target"].shape == (0,) and not np.asarray(table["n_targets"].values).any()
                assert not np.asarray(table["n_candidates"].values).any()
            elif dtype == "float64":
                from test_gpu_single_target import _compare

                _compare(table, K.expected(S, dtype))
            return table, ep.targets.track_targets(table, "gated_nearest", track)

        run.has_oracle = True
        return run

    return api(fn)


def a_track(variant):
    def fn(ep, torch):
        import track_cases as K
        from test_gpu_track import _dataset

        t = K.lanes([K.TILE - 1, K.TILE, K.TILE + 1, 2, 0, 1]) if variant == "tile" else K.CASES["nothing"][0]
        prm = K.LOOSE if variant == "tile" else K.CASES["nothing"][1]
        def run():
            out = ep.targets.track_targets(_dataset(t), "gated_nearest", prm)
            if variant != "tile":
                from test_gpu_track import _compare

                _compare(out, K.expected("nothing"), len(t["channel_index"]))
            return out

        run.has_oracle = variant != "tile"
        return run

    return api(fn)


# ---- the table ------------------------------------------------------------------------------------------------------------
class Case:
    """``covers``: the allocating ops functions the row must be seen to call (checked against the stacks of the
    allocation requests, unless the row is refused).  ``no_oracle``: for a degenerate row, why no reference is applied (the
    others carry one: their closure holds the result to it).  ``all_empty``: a zero-length row all of whose outputs are
    empty, so that nothing can pass through the patch."""

    def __init__(self, name, covers, build, kind="base", zero=None, no_oracle=None, all_empty=False):
        self.name, self.covers, self.build, self.kind, self.zero = name, tuple(covers), build, kind, zero
        self.no_oracle, self.all_empty = no_oracle, all_empty
        assert kind in ("base", "degenerate", "zero") and (zero in ("returns", "raises")) == (kind == "zero"), name
        assert no_oracle is None or kind == "degenerate", name
        assert not all_empty or zero == "returns", name

    def __repr__(self):
        return self.name


CASES = []


def case(name, covers, fn, *a, kind="base", zero=None, no_oracle=None, all_empty=False, **kw):
    CASES.append(Case(name, covers if isinstance(covers, tuple) else (covers,),
                      (lambda torch, ops: fn(torch, ops, *a, **kw)) if (a or kw) else fn, kind, zero, no_oracle, all_empty))


F = ("float32", "float64")

case("power_coef_ek", "power_coef_ek", b_power_coef)
case("power_coef_ek[a ping without a pulse length]", "power_coef_ek", b_power_coef, nan_ping=True, kind="degenerate",
     no_oracle="oracle.calibrate states Sv, not the coefficient rows: they are held to it through sv_power in tests/test_gpu_kernels.py")
case("power_coef_ek[P=0]", "power_coef_ek", b_power_coef, P=0, kind="zero", zero="raises")
case("pulse_table_lookup", "pulse_table_lookup", b_pulse_table)
case("pulse_table_lookup[all NaN]", "pulse_table_lookup", b_pulse_table, nan=True, kind="degenerate",
     no_oracle="oracle.calibrate.vend_cal_params_power takes argmin of |NaN|, which NumPy leaves to the first entry: no rule to hold to")
case("pulse_table_lookup[P=0]", "pulse_table_lookup", b_pulse_table, P=0, kind="zero", zero="raises")
for S in ROWS:
    for dt in F:
        case(f"sv_power[S={S},{dt}]", "sv_power", b_sv_power, (2, 3, S), dt)
for dt in F:
    case(f"sv_power[two chunks, statistics alone,{dt}]", "sv_power", b_sv_power_stats_only, (2, 3, 1028), dt)
    case(f"sv_power[all NaN,{dt}]", "sv_power", b_sv_power, (2, 3, 65), dt, "nan", kind="degenerate")
case("sv_power[S=0]", "sv_power", b_sv_power, (2, 3, 0), kind="zero", zero="raises")
case("sv_power[P=0]", "sv_power", b_sv_power, (2, 0, 5), kind="zero", zero="raises")
for S in (5, 1028):
    case(f"range_power[S={S}]", "range_power", b_range_power, (2, 3, S))
case("range_power[all NaN,float32]", "range_power", b_range_power, (2, 3, 65), "float32", "nan", kind="degenerate")
case("range_power[C=0]", "range_power", b_range_power, (0, 3, 5), kind="zero", zero="raises")
case("time_bin_offsets", "time_bin_offsets", b_time_bin_offsets)
case("time_bin_offsets[bins without a ping, closed right]", "time_bin_offsets", b_time_bin_offsets, P=3, n_bins=9, dt=10**8,
     closed="right", kind="degenerate")
case("time_bin_offsets[P=0]", "time_bin_offsets", b_time_bin_offsets, P=0, kind="zero", zero="raises")
for dt in F:
    case(f"sv_mvbs_fused[{dt}]", ("sv_mvbs_fused", "_partials"), b_sv_mvbs_fused, dtype=dt)
    case(f"sv_mvbs_fused[all NaN, bins without a ping,{dt}]", "sv_mvbs_fused", b_sv_mvbs_fused, dtype=dt, fill="nan",
         kind="degenerate")
case("sv_mvbs_fused[odd S, closed right, no Sv]", "sv_mvbs_fused", b_sv_mvbs_fused, shape=(2, 8, 63), closed="right",
     want_sv=False, want_range_stats=False, want_range_max=True)
case("sv_mvbs_fused[one bin of all pings]", "sv_mvbs_fused", b_sv_mvbs_fused, shape=(1, 2, 257), per=2, n_tbins=1)
case("sv_mvbs_fused[P=0]", "sv_mvbs_fused", b_sv_mvbs_fused, shape=(2, 0, 65), kind="zero", zero="raises")
for dt in F:
    case(f"sv_mvbs_fused_depth[{dt}]", "sv_mvbs_fused_depth", b_sv_mvbs_fused_depth, dtype=dt)
case("sv_mvbs_fused_depth[all NaN, a bin without a ping]", "sv_mvbs_fused_depth", b_sv_mvbs_fused_depth, fill="nan",
     kind="degenerate")
case("sv_mvbs_fused_depth[S=0]", "sv_mvbs_fused_depth", b_sv_mvbs_fused_depth, shape=(2, 8, 0), kind="zero", zero="raises")
for dt in F:
    case(f"sv_mvbs_fused_i16[{dt}]", "sv_mvbs_fused_i16", b_sv_mvbs_fused_i16, dtype=dt)
case("sv_mvbs_fused_i16[every ping empty]", "sv_mvbs_fused_i16", b_sv_mvbs_fused_i16, empty_pings=True, kind="degenerate")
case("sv_mvbs_fused_i16[C=0]", "sv_mvbs_fused_i16", b_sv_mvbs_fused_i16, shape=(0, 8, 64), kind="zero", zero="raises")
for dt in F:
    case(f"mvbs[range,{dt}]", ("mvbs", "_partials"), b_mvbs, dtype=dt)
case("mvbs[coefficient rows]", "mvbs", b_mvbs, by="coef")
case("mvbs[all NaN, bins without a ping]", "mvbs", b_mvbs, fill="nan", kind="degenerate")
case("mvbs[P=0]", "mvbs", b_mvbs, shape=(2, 0, 65), kind="zero", zero="raises")
for n in (1, 255, 257):
    case(f"selftest_lin_from_db, selftest_log10[n={n}]", ("selftest_lin_from_db", "selftest_log10"), b_selftests, n=n)
case("selftest_lin_from_db, selftest_log10[n=0]", ("selftest_lin_from_db", "selftest_log10"), b_selftests, n=0, kind="zero",
     zero="raises")
for dt in ("complex64", "complex128"):
    case(f"selftest_correlate[{dt}]", "selftest_correlate", b_selftest_correlate, dt)
case("selftest_correlate[all NaN]", "selftest_correlate", b_selftest_correlate, fill="nan", kind="degenerate")
case("selftest_correlate[no tile]", "selftest_correlate", b_selftest_correlate, tiles=0, kind="zero", zero="raises")
for dt in F:
    case(f"mvbs_finalize[{dt}]", "mvbs_finalize", b_mvbs_finalize, dtype=dt)
case("mvbs_finalize[every cell empty]", "mvbs_finalize", b_mvbs_finalize, empty=True, kind="degenerate")
case("mvbs_finalize[n=0]", "mvbs_finalize", b_mvbs_finalize, shape=(2, 0, 65), kind="zero", zero="raises")
for dt in F:
    case(f"affine_rows[{dt}]", "affine_rows", b_affine_rows, dtype=dt)
case("affine_rows[all NaN]", "affine_rows", b_affine_rows, fill="nan", kind="degenerate")
case("affine_rows[S=0]", "affine_rows", b_affine_rows, shape=(2, 5, 0), kind="zero", zero="raises")
for S in (260, 261, 1, 65):
    for dt in F:
        case(f"depth_rows[range,S={S},{dt}]", "depth_rows", b_depth_rows, (2, 5, S), dt)
    case(f"depth_rows[coefficient rows,S={S}]", "depth_rows", b_depth_rows, (2, 5, S), src="coef")
case("depth_rows[all NaN]", "depth_rows", b_depth_rows, fill="nan", kind="degenerate")
case("depth_rows[all NaN, coefficient rows, odd S]", "depth_rows", b_depth_rows, (2, 5, 261), fill="nan", src="coef",
     kind="degenerate")
case("depth_rows[P=0]", "depth_rows", b_depth_rows, (2, 0, 260), kind="zero", zero="raises")
for n in (1, 255, 257, 1000):
    for dt in F:
        case(f"nanminmax[n={n},{dt}]", "nanminmax", b_nanminmax, n, dt)
case("nanminmax[all NaN]", "nanminmax", b_nanminmax, 257, fill="nan", kind="degenerate")
case("nanminmax[n=0]", "nanminmax", b_nanminmax, 0, kind="zero", zero="returns")
for dt in F:
    case(f"mvbs_index[{dt}]", "mvbs_index", b_mvbs_index, dtype=dt)
case("mvbs_index[all NaN]", "mvbs_index", b_mvbs_index, fill="nan", kind="degenerate")
case("mvbs_index[S=0]", "mvbs_index", b_mvbs_index, shape=(2, 7, 0), kind="zero", zero="raises")
for dt in F:
    case(f"noise_estimate, noise_apply[{dt}]", ("noise_estimate", "noise_apply"), b_noise, dtype=dt)
case("noise_estimate, noise_apply[all NaN]", ("noise_estimate", "noise_apply"), b_noise, fill="nan", kind="degenerate")
case("noise_estimate, noise_apply[P=0]", ("noise_estimate", "noise_apply"), b_noise, shape=(2, 0, 65), kind="zero",
     zero="raises")
for dt in F:
    case(f"noise_apply[coefficient rows,{dt}]", "noise_apply", b_noise_apply_rows, dtype=dt)
case("noise_finalize", "noise_finalize", b_noise_finalize)
case("noise_finalize[every block empty]", "noise_finalize", b_noise_finalize, empty=True, kind="degenerate")
case("noise_finalize[rows=0]", "noise_finalize", b_noise_finalize, rows=0, kind="zero", zero="raises")
for bb in (False, True):
    case(f"complex_coef_ek80[bb={bb}]", "complex_coef_ek80", b_complex_coef, bb=bb)
case("complex_coef_ek80[all NaN]", "complex_coef_ek80", b_complex_coef, nan=True, kind="degenerate",
     no_oracle="oracle.calibrate states Sv, not the coefficient rows: they are held to it through sv_complex in tests/test_gpu_kernels.py")
case("complex_coef_ek80[P=0]", "complex_coef_ek80", b_complex_coef, P=0, kind="zero", zero="raises")
for dt in F:
    case(f"range_complex[{dt}]", "range_complex", b_range_complex, dtype=dt)
case("range_complex[all NaN]", "range_complex", b_range_complex, fill="nan", kind="degenerate")
case("range_complex[S=0]", "range_complex", b_range_complex, shape=(2, 3, 0, 4), kind="zero", zero="raises")
for dt in F:
    case(f"sv_complex[fft,{dt}]", "sv_complex", b_sv_complex, dtype=dt)
    case(f"sv_complex[cw,{dt}]", "sv_complex", b_sv_complex, shape=(2, 3, 257, 4), dtype=dt, cw=True)
case("sv_complex[fft, a replica per interval]", "sv_complex", b_sv_complex, indexed=True)
case("sv_complex[direct]", "sv_complex", b_sv_complex, shape=(2, 3, 257, 4), method="direct")
case("sv_complex[direct, a replica per interval]", "sv_complex", b_sv_complex, shape=(2, 3, 257, 4), method="direct", indexed=True)
case("sv_complex[fft, all NaN]", "sv_complex", b_sv_complex, fill="nan", kind="degenerate")
case("sv_complex[cw, all NaN]", "sv_complex", b_sv_complex, shape=(2, 3, 65, 4), fill="nan", cw=True, kind="degenerate")
case("sv_complex[fft, S=0]", "sv_complex", b_sv_complex, shape=(2, 3, 0, 4), kind="zero", zero="raises")
for kind_ in ("int8", "rand", "nan"):
    case(f"splitbeam_power[{kind_}]", "splitbeam_power", b_splitbeam_power, planes=kind_,
         kind="degenerate" if kind_ == "nan" else "base")
case("splitbeam_power[float32 angles]", "splitbeam_power", b_splitbeam_power, shape=(2, 5, 257), dtype="float32")
case("splitbeam_power[P=0]", "splitbeam_power", b_splitbeam_power, shape=(2, 0, 65), kind="zero", zero="raises")
for m in ("fft", "direct", "cw"):
    case(f"splitbeam_complex[{m}]", "splitbeam_complex", b_splitbeam_complex, shape=(2, 3, 2100 if m == "fft" else 257, 4),
         method=m)
case("splitbeam_complex[fft, all NaN, a skipped channel]", "splitbeam_complex", b_splitbeam_complex, fill="nan", beam=(1, -1),
     kind="degenerate")
case("splitbeam_complex[cw, every channel skipped]", "splitbeam_complex", b_splitbeam_complex, shape=(2, 3, 65, 4), method="cw",
     beam=(-1, -1), kind="degenerate")
case("splitbeam_complex[S=0]", "splitbeam_complex", b_splitbeam_complex, shape=(2, 3, 0, 4), method="cw", kind="zero",
     zero="raises")
SEAFLOOR = ("seafloor_state", "seafloor_angle_mask", "seafloor_median", "seafloor_components", "seafloor_bottom", "seafloor_basic")
for dt in F:
    case(f"seafloor chain[{dt}]", SEAFLOOR, b_seafloor, dtype=dt)
case("seafloor chain[all NaN]", SEAFLOOR, b_seafloor, fill="nan", kind="degenerate")
case("seafloor chain[an empty angle mask]", SEAFLOOR, b_seafloor, masked=False, kind="degenerate")
case("seafloor chain[P=0]", SEAFLOOR, b_seafloor, P=0, kind="zero", zero="raises")
SHOAL = ("shoal_state", "shoal_threshold_fill", "shoal_label", "shoal_echoview_link")
for dt in F:
    case(f"shoal chain[{dt}]", SHOAL, b_shoal, dtype=dt)
case("shoal chain[4-connected, 63 x 65]", SHOAL, b_shoal, P=63, S=65, connectivity=4)
case("shoal chain[all NaN]", SHOAL, b_shoal, fill="nan", kind="degenerate")
case("shoal chain[nothing above the threshold]", SHOAL, b_shoal, thr=1e9, kind="degenerate")
case("shoal chain[P=0]", SHOAL, b_shoal, P=0, kind="zero", zero="raises")
for dt in F:
    case(f"transient_fielding, transient_matecho[{dt}]", ("transient_fielding", "transient_matecho"), b_transient, dtype=dt)
case("transient_fielding, transient_matecho[all NaN]", ("transient_fielding", "transient_matecho"), b_transient, fill="nan",
     kind="degenerate")
case("transient_fielding, transient_matecho[P=0]", ("transient_fielding", "transient_matecho"), b_transient, shape=(2, 0, 40),
     kind="zero", zero="raises")
for dt in F:
    case(f"freq_diff_mask[{dt}]", "freq_diff_mask", b_freq_diff, dtype=dt)
case("freq_diff_mask[all NaN]", "freq_diff_mask", b_freq_diff, fill="nan", kind="degenerate")
case("freq_diff_mask[P=0]", "freq_diff_mask", b_freq_diff, shape=(2, 0, 65), kind="zero", zero="raises")
case("regrid_mask", "regrid_mask", b_regrid_mask)
case("regrid_mask[two slices, a bin without a ping]", "regrid_mask", b_regrid_mask, shape=(2, 6, 8), n_tbins=3)
case("regrid_mask[nothing set]", "regrid_mask", b_regrid_mask, all_false=True, kind="degenerate")
case("regrid_mask[P=0]", "regrid_mask", b_regrid_mask, shape=(1, 0, 8), kind="zero", zero="returns")
for dt in F:
    case(f"line_mask[range,{dt}]", "line_mask", b_line_mask, dtype=dt)
    case(f"line_mask[coefficient rows,{dt}]", "line_mask", b_line_mask, dtype=dt, lazy=True)
case("line_mask[all NaN]", "line_mask", b_line_mask, fill="nan", kind="degenerate")
case("line_mask[a NaN line]", "line_mask", b_line_mask, fill="nan_line", kind="degenerate")
case("line_mask[S=0]", "line_mask", b_line_mask, shape=(2, 5, 0), kind="zero", zero="returns", all_empty=True)
for S in (1, 3, 65, 257):
    for dt in F:
        case(f"regrid_rows[S={S},{dt}]", "regrid_rows", b_regrid_rows, (2, 3, S), dt)
case("regrid_rows[all NaN]", "regrid_rows", b_regrid_rows, fill="nan", kind="degenerate")
case("regrid_rows[no range bin]", "regrid_rows", b_regrid_rows, n_rbins=0, kind="zero", zero="returns")
case("regrid_rows[P=0]", "regrid_rows", b_regrid_rows, (2, 0, 65), kind="zero", zero="returns")
for m in ("median", "mean", "min", "max"):
    for dt in F:
        case(f"window_filter[{m},{dt}]", "window_filter", b_window_filter, dtype=dt, method=m)
case("window_filter[all NaN]", "window_filter", b_window_filter, fill="nan", kind="degenerate")
case("window_filter[S=0]", "window_filter", b_window_filter, shape=(2, 18, 0), kind="zero", zero="returns", all_empty=True)
for S in ROWS:
    for dt in F:
        case(f"echo_metrics[S={S},{dt}]", "echo_metrics", b_echo_metrics, 5, S, dt)
case("echo_metrics[all NaN]", "echo_metrics", b_echo_metrics, fill="nan", kind="degenerate")
case("echo_metrics[R=0]", "echo_metrics", b_echo_metrics, R=0, kind="zero", zero="returns", all_empty=True)
for m in ("linear", "nearest"):
    case(f"align_to_ping_time[{m}]", "align_to_ping_time", b_align, method=m)
case("align_to_ping_time[every ping NaT]", "align_to_ping_time", b_align, nat=True, kind="degenerate")
case("align_to_ping_time[P=0]", "align_to_ping_time", b_align, P=0, kind="zero", zero="raises")
for N in (2, 1025, 2049):
    case(f"time_reversals, reversal_medians, time_rebuild[N={N}]", ("time_reversals", "reversal_medians", "time_rebuild"),
         b_time_rebuild, N)
case("time_reversals[no reversal]", "time_reversals", b_time_reversals_none, kind="degenerate")
case("time_reversals[N=1]", "time_reversals", b_one_time, "time_reversals", kind="zero", zero="returns")
case("reversal_medians[N=1]", "reversal_medians", b_one_time, "reversal_medians", kind="zero", zero="raises")
case("time_rebuild[N=1]", "time_rebuild", b_one_time, "time_rebuild", kind="zero", zero="raises")
for dt in ("float32", "float64", "int16"):
    case(f"concat_rows[{dt}]", "concat_rows", b_concat_rows, dt)
case("concat_rows[sectors]", "concat_rows", b_concat_rows, "float32", beams=3)
case("concat_rows[a file without pings]", "concat_rows", b_concat_rows, "float32", P=(2, 0), kind="zero", zero="raises")
for ang in ("float32", "int8", None):
    case(f"raw0_unpack[{ang}]", "raw0_unpack", b_raw0_unpack, angles=ang)
case("raw0_unpack[S=257]", "raw0_unpack", b_raw0_unpack, S=257)
case("raw0_unpack[every ping empty]", "raw0_unpack", b_raw0_unpack, empty=True, kind="degenerate")
case("raw0_unpack[P=0]", "raw0_unpack", b_raw0_unpack, P=0, kind="zero", zero="raises")
case("nmea_positions", "nmea_positions", b_nmea)
case("nmea_positions[one sentence]", "nmea_positions", b_nmea, n=1)
case("nmea_positions[n=0]", "nmea_positions", b_nmea, n=0, kind="zero", zero="returns", all_empty=True)
for dt in F:
    case(f"range_bin_smooth[index,{dt}]", "range_bin_smooth", b_range_bin_smooth, dtype=dt)
case("range_bin_smooth[value]", "range_bin_smooth", b_range_bin_smooth, value=True)
case("range_bin_smooth[all NaN]", "range_bin_smooth", b_range_bin_smooth, fill="nan", kind="degenerate")
case("range_bin_smooth[S=0]", "range_bin_smooth", b_range_bin_smooth, shape=(2, 5, 0), kind="zero", zero="raises")
for dt in F:
    case(f"impulse_mask[{dt}]", "impulse_mask", b_impulse_mask, dtype=dt)
case("impulse_mask[all NaN]", "impulse_mask", b_impulse_mask, fill="nan", kind="degenerate")
case("impulse_mask[P=0]", "impulse_mask", b_impulse_mask, shape=(2, 0, 65), kind="zero", zero="raises")
for fn_ in ("nanmean", "nanmedian"):
    for dt in F:
        case(f"pool_sv[{fn_},{dt}]", "pool_sv", b_pool_sv, dtype=dt, func=fn_)
        case(f"pool_sv_value[{fn_},{dt}]", ("pool_sv_value", "range_rows_check"), b_pool_sv_value, dtype=dt, func=fn_)
    case(f"pool_sv_value[{fn_}, pings with their own ranges]", ("pool_sv_value", "range_rows_check"), b_pool_sv_value,
         shape=(2, 9, 40), func=fn_, ragged=True)
    case(f"pool_sv[{fn_}, all NaN]", "pool_sv", b_pool_sv, func=fn_, fill="nan", kind="degenerate")
    case(f"pool_sv_value[{fn_}, all NaN]", ("pool_sv_value", "range_rows_check"), b_pool_sv_value, func=fn_, fill="nan",
         kind="degenerate")
case("pool_sv[nanmean, the first sample behind the last]", "pool_sv", b_pool_sv, first=40, kind="degenerate",
     no_oracle="oracle.masks.index_binning_pool_Sv derives the first sample from exclude_above and never places it behind the row")
case("pool_sv[S=0]", "pool_sv", b_pool_sv, shape=(2, 6, 0), kind="zero", zero="raises")
case("pool_sv_value[P=0]", ("pool_sv_value", "range_rows_check"), b_pool_sv_value, shape=(2, 0, 40), kind="zero", zero="raises")
for dt in F:
    case(f"attenuated_mask[{dt}]", "attenuated_mask", b_attenuated, dtype=dt)
case("attenuated_mask[odd S]", "attenuated_mask", b_attenuated, shape=(2, 6, 41))
case("attenuated_mask[all NaN]", "attenuated_mask", b_attenuated, fill="nan", kind="degenerate")
case("attenuated_mask[P=0]", "attenuated_mask", b_attenuated, shape=(2, 0, 40), kind="zero", zero="raises")
APPLY = ("apply_mask", "apply_masks", "mask_and")
for n in (1, 255, 256, 257, 1000):
    for dt in F:
        case(f"apply_mask, apply_masks, mask_and[n={n},{dt}]", APPLY, b_apply_mask, n, dt)
case("apply_mask, apply_masks[a fill array]", APPLY, b_apply_mask, 257, array_fill=True)
case("apply_mask, apply_masks[masks that remove everything]", APPLY, b_apply_mask, 257, keep="none", kind="degenerate")
case("apply_mask, apply_masks[all NaN]", APPLY, b_apply_mask, 257, fill="nan", keep="all", kind="degenerate")
case("apply_mask[n=0]", "apply_mask", lambda torch, ops: (lambda: ops.apply_mask(
    samples(torch, (0,), torch.float32, 1), torch.zeros(0, dtype=torch.uint8).cuda())), kind="zero", zero="raises")
case("mask_and[n=0]", "mask_and", lambda torch, ops: (lambda: ops.mask_and(
    torch.zeros(0, dtype=torch.uint8).cuda(), torch.zeros(0, dtype=torch.uint8).cuda())), kind="zero", zero="raises")
case("apply_masks[n=0: empty_no_pointers]", "apply_masks", b_apply_mask, 0, kind="zero", zero="returns")
case("apply_masks[n=0: empty_view under a live mask]", "apply_masks", b_apply_mask, 0, empty="view", kind="zero",
     zero="returns")
for dt in F:
    case(f"range_step_mean[{dt}]", "range_step_mean", b_range_step_mean, dtype=dt)
case("range_step_mean[all NaN]", "range_step_mean", b_range_step_mean, fill="nan", kind="degenerate")
case("range_step_mean[S=1]", "range_step_mean", b_range_step_mean, shape=(2, 3, 1), kind="degenerate")
case("range_step_mean[P=0]", "range_step_mean", b_range_step_mean, shape=(2, 0, 17), kind="zero", zero="raises")
case("first_not_le", "first_not_le", b_first_not_le)
case("first_not_le[all NaN]", "first_not_le", b_first_not_le, fill="nan", kind="degenerate")
case("first_not_le[n=0]", "first_not_le", b_first_not_le, n=0, kind="zero", zero="raises")
case("geodesic_steps", "geodesic_steps", b_geodesic)
case("geodesic_steps[one ping]", "geodesic_steps", b_geodesic, P=1, kind="degenerate")
case("geodesic_steps[all NaN]", "geodesic_steps", b_geodesic, nan=True, kind="degenerate")
case("geodesic_steps[P=0]", "geodesic_steps", b_geodesic, P=0, kind="zero", zero="raises")
for dt in F:
    case(f"nasc[{dt}]", "nasc", b_nasc, dtype=dt)
# 33 depths a metre apart on 8250 bins of 4 mm: 24 bytes a bin do not fit in LDS, every sample has its own cell
case("nasc[float32, a grid beyond the LDS accumulators]", "nasc", b_nasc, dtype="float32", range_bin=0.004, n_rbins=8250)
case("nasc[all NaN, a distance bin without a ping]", "nasc", b_nasc, fill="nan", kind="degenerate")
case("nasc[P=0]", "nasc", b_nasc, shape=(2, 0, 33), kind="zero", zero="raises")
for dt in F:
    case(f"sv_noise_fused[{dt}]", "sv_noise_fused", b_sv_noise_fused, dtype=dt)
    case(f"denoise_mvbs[{dt}]", ("denoise_mvbs", "_partials"), b_denoise_mvbs, dtype=dt)
    case(f"sv_denoise_mvbs[{dt}]", ("sv_denoise_mvbs", "_partials"), b_denoise_mvbs, dtype=dt, raw_route=True)
case("sv_noise_fused[odd S]", "sv_noise_fused", b_sv_noise_fused, shape=(2, 7, 65))
case("sv_noise_fused[all NaN]", "sv_noise_fused", b_sv_noise_fused, fill="nan", kind="degenerate")
case("denoise_mvbs[all NaN]", "denoise_mvbs", b_denoise_mvbs, fill="nan", kind="degenerate")
case("sv_denoise_mvbs[all NaN]", "sv_denoise_mvbs", b_denoise_mvbs, fill="nan", raw_route=True, kind="degenerate")
case("sv_noise_fused[P=0]", "sv_noise_fused", b_sv_noise_fused, shape=(2, 0, 64), kind="zero", zero="raises")
case("denoise_mvbs[S=0]", "denoise_mvbs", b_denoise_mvbs, shape=(2, 8, 0), kind="zero", zero="raises")
case("sv_denoise_mvbs[S=0]", "sv_denoise_mvbs", b_denoise_mvbs, shape=(2, 8, 0), raw_route=True, kind="zero", zero="raises")
for ty in (None, "float32", "float64"):
    case(f"edge_gather[{ty}]", "edge_gather", b_edge_gather, typed=ty)
case("edge_gather[no edge]", "edge_gather", b_edge_gather, n_edges=0, kind="zero", zero="raises")
for dt in F:
    case(f"sv_spectrum[{dt}]", "sv_spectrum", b_sv_spectrum, dt)
case("sv_spectrum[all NaN]", "sv_spectrum", b_sv_spectrum, fill="nan", kind="degenerate")
for dt in F:
    case(f"target_spectra[{dt}]", "target_spectra", b_target_spectra, dt)
case("target_spectra[N=0]", "target_spectra", b_target_spectra, rows="none", kind="zero", zero="returns", all_empty=True)

# the public API (every row: the three runs give identical values and numeric attributes)
case("api: mask.apply_mask", ("apply_masks",), a_apply_mask("base"))
case("api: mask.apply_mask[all masked]", ("apply_masks",), a_apply_mask("all_masked"), kind="degenerate")
case("api: mask.apply_mask[all NaN]", ("apply_masks",), a_apply_mask("all_nan"), kind="degenerate")
case("api: mask.apply_mask[no channels: empty_view]", ("apply_masks",), a_apply_mask("empty_view"), kind="zero", zero="returns")
case("api: mask.apply_mask[empty_no_pings]", ("apply_masks",), a_apply_mask("empty_fresh"), kind="zero", zero="returns")
for dt in F:
    case(f"api: clean.remove_background_noise[{dt}]", (), a_noise(dt))
for v in ("range", "depth", "fused", "index"):
    case(f"api: compute_MVBS[{v}]", (), a_mvbs(v))
case("api: commongrid.compute_NASC", ("nasc", "align_to_ping_time"), a_nasc("base"))
case("api: consolidate.add_location, add_splitbeam_angle", ("align_to_ping_time", "splitbeam_power"), a_location_angles("base"))
case("api: mask.detect_seafloor, line_mask, apply_mask", ("line_mask", "apply_masks"), a_seafloor("base"))
case("api: clean.window_filter, mask.detect_shoal", ("window_filter",), a_shoal("base"))
case("api: clean.window_filter, mask.detect_shoal[nothing above the threshold]", ("window_filter",), a_shoal("nothing"),
     kind="degenerate")
case("api: mask.label_regions, region_statistics", ("shoal_label", "region_labels"), a_regions("base"))
case("api: mask.label_regions, region_statistics[no region]", (), a_regions("nothing"),
     kind="degenerate")
case("api: clean.detect_transient", ("transient_fielding", "transient_matecho"), a_transient("base"))
for dt in F:
    case(f"api: commongrid.regrid_Sv, mask.frequency_differencing[{dt}]", ("regrid_rows", "freq_diff_mask"), a_regrid(dt))
case("api: mask.regrid_mask", ("regrid_mask",), a_regrid_mask("base"))
case("api: mask.regrid_mask[nothing set]", ("regrid_mask",), a_regrid_mask("nothing"), kind="degenerate")
for v in ("base", "all_neg_inf", "range_nan"):
    case(f"api: metrics.summary[{v}]", ("echo_metrics",), a_metrics(v), kind="base" if v == "base" else "degenerate")
TARGETS = ("single_target_count", "single_target_emit", "track_prepare", "track_roots", "track_table")
for v in ("tile", "tile_less_one"):
    case(f"api: targets.detect_single_targets, track_targets[{v}]", TARGETS[:4], a_targets(v))
case("api: targets.detect_single_targets, track_targets[tile,float32]", TARGETS[:4], a_targets("tile", "float32"))
case("api: targets.detect_single_targets, track_targets[no target anywhere]", ("single_target_count",), a_targets("none"), kind="degenerate")
case("api: targets.track_targets[tile edges]", TARGETS[2:], a_track("tile"))
case("api: targets.track_targets[no two targets link]", ("track_prepare", "track_roots"), a_track("nothing"), kind="degenerate")


# ---- the test -------------------------------------------------------------------------------------------------------------
def outcome(fn, may_raise):
    """``fn()`` as comparable bits, or ("ValueError", no kernel launched) for a zero-length row that is refused."""
    from echopype_amd import _lib

    if not may_raise:
        return _bits(fn())
    with _lib.launch_trace() as tr:
        try:
            res = _bits(fn())
        except ValueError:
            res = "ValueError"
    if res == "ValueError":
        assert tr.kernels == [], f"refused, but only after launching {tr.kernels}"
    return res


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_result_depends_on_inputs_alone(env, c):
    torch, ops = env
    fn = c.build(torch, ops)
    zero = c.kind == "zero"
    if c.kind == "degenerate":  # the reference on the row's inputs, or the reason there is none
        assert bool(getattr(fn, "has_oracle", False)) != bool(c.no_oracle), "a degenerate row carries its reference or its reason"
    plain = outcome(fn, zero)
    refused = plain == "ValueError"
    if zero:
        assert refused == (c.zero == "raises"), f"the table says a zero-length input {c.zero}"
    for byte in BYTES:
        with Poisoned(torch, ops, byte) as p:
            got = outcome(fn, zero)
            n_out, n_scratch = p.check()
        print(f"{c.name}: {byte:#x}: {n_out} outputs, {n_scratch} scratch buffers through the patch")
        assert refused or c.all_empty or n_out + n_scratch >= 1, "no allocation went through the patch"
        assert got == plain, f"the result under {byte:#x} differs from the plain run: memory the library did not write was read"
        assert set(p.scratch_names()) <= set(AUDIT), set(p.scratch_names()) - set(AUDIT)
        assert refused or set(c.covers) <= p.callers, f"the row does not call {sorted(set(c.covers) - p.callers)}"


def test_selftests_refuse_anything_but_float64(env):
    """The three entries take doubles: a float32 tensor would be read and written past its end."""
    torch, ops = env
    x = torch.ones(257, dtype=torch.float32).cuda()
    for call in (lambda: ops.selftest_lin_from_db(x), lambda: ops.selftest_log10(x), lambda: ops.selftest_log10(x, inline=True)):
        with pytest.raises(ValueError, match="float64 tensor expected"):
            call()
