"""Every scratch buffer ``ops`` allocates, between two guard bands: a kernel that writes outside the size the library
answered for (``epa_scratch_bytes``) changes a band, and the test names the buffer.

The fixture wraps ``ops._scratch_alloc``: each buffer gets 4096 extra bytes in front and behind, both filled with 0xA5,
and the middle is handed out (256-byte aligned, as torch's own allocations are).  All memory touched belongs to the
test.  Each case runs its wrapper once plainly and once between the bands and compares the two results bit for bit:
the bands changed nothing.  Shapes are the smallest at which an extent is at an edge of its launch plan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAND = 4096
FILL = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


class Guard:
    """``with Guard(torch, ops) as g: ...``: scratch between bands; ``g.check()`` asserts every band is intact."""

    def __init__(self, torch, ops):
        self.torch, self.ops, self.bufs, self.what = torch, ops, [], None

    def __enter__(self):
        ops = self.ops
        self._alloc, self._scratch = ops._scratch_alloc, ops._scratch

        def scratch(what, *args, **kw):  # (the name, for the message)
            self.what = what
            return self._scratch(what, *args, **kw)

        ops._scratch_alloc, ops._scratch = self.alloc, scratch
        return self

    def __exit__(self, *exc):
        self.ops._scratch_alloc, self.ops._scratch = self._alloc, self._scratch
        return False

    def alloc(self, nbytes, dtype, device, zero):
        torch = self.torch
        n = -(-nbytes // dtype.itemsize) * dtype.itemsize  # what ops._scratch_alloc hands out
        raw = torch.empty(BAND + n + BAND, dtype=torch.uint8, device=device)
        raw[:BAND] = FILL
        raw[BAND + n:] = FILL
        mid = raw[BAND:BAND + n]
        if zero:
            mid.zero_()
        assert mid.data_ptr() % 256 == 0
        self.bufs.append((self.what, raw, n))
        return mid.view(dtype)

    def check(self):
        self.torch.cuda.synchronize()
        for what, raw, n in self.bufs:
            for side, band in (("in front of", raw[:BAND]), ("behind", raw[BAND + n:])):
                bad = (band != FILL).nonzero()
                assert bad.numel() == 0, (f"{what} ({n} bytes): {bad.numel()} bytes written {side} it, the first at band "
                                          f"offset {int(bad[0])}")
        return {what for what, _, _ in self.bufs}


def _bits(x):
    """A result as something ``==`` compares bit for bit (NaN payloads included)."""
    import torch

    if isinstance(x, torch.Tensor):
        return x.detach().contiguous().cpu().numpy().tobytes()
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_bits(v) for v in x]
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


def guarded(env, fn, *names):
    """``fn()`` plainly and between the bands: the same bits, every band intact, the buffers ``names`` were allocated."""
    torch, ops = env
    plain = _bits(fn())
    with Guard(torch, ops) as g:
        got = _bits(fn())
        seen = g.check()
    assert set(names) <= seen, (names, seen)
    assert got == plain
    return seen


def randn(torch, shape, dtype, seed, n_nan=3, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g, dtype=torch.float64) * scale + shift
    flat = t.view(-1)
    if n_nan and flat.numel() > 1:
        flat[torch.randint(0, flat.numel(), (min(n_nan, flat.numel() - 1),), generator=g)] = float("nan")
    return t.to(dtype).cuda()


def power_rows(torch, C, P):
    """Power-sample coefficient rows (C, P, NCOEF): ra, rb, r0, shift, alpha2, A0, g, d = (shift - r0) / (ra * rb)."""
    row = torch.tensor([0.02, 10.0, 0.0, 0.4, 0.01, -50.0, 0.1, 2.0], dtype=torch.float64)
    rows = row.repeat(C, P, 1)
    rows[..., 5] += torch.arange(C * P, dtype=torch.float64).view(C, P) * 0.25
    return rows.cuda()


def complex_rows(torch, C, P):
    """Complex-sample coefficient rows (C, P, NCCOEF): ra, rb, shift, alpha2, A, pscale, 0, 0."""
    row = torch.tensor([1e-4, 750.0, 0.1, 0.02, -20.0, 1.0, 0.0, 0.0], dtype=torch.float64)
    return row.repeat(C, P, 1).cuda()


def replicas(torch, n, taps, seed=11):
    g = torch.Generator().manual_seed(seed)
    rep = torch.randn((n * taps, 2), generator=g, dtype=torch.float32).reshape(-1).cuda()
    off = (torch.arange(n + 1, dtype=torch.int32) * taps).cuda()
    return rep, off


# ---- K1 and its statistics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,want_range", [
    ((2, 3, 1028), False),        # two chunks of 1024 per row: the grid is rows x chunks
    ((1, 8193, 4), False),        # one row more than the 8192 workgroups aimed at
    ((1, 1, 1024 * 8193), False),  # more chunks in a row than 8192: gx clamps to 1 (34 MB of samples)
    ((2, 3, 1027), True),         # odd S: the scalar kernel, then epa_nanminmax on the range it wrote
])
def test_sv_power_range_stats(env, dtype, shape, want_range):
    torch, ops = env
    raw = randn(torch, shape, torch.float32, 1, scale=10.0, shift=-70.0)
    coef = power_rows(torch, *shape[:2])
    guarded(env, lambda: ops.sv_power(raw, coef, dtype=getattr(torch, dtype), want_range=want_range,
                                      want_range_stats=True), "sv_power_stats.workspace")


@pytest.mark.parametrize("S", [260, 261])  # 16-byte rows: one-piece workgroups and their slots; odd: a partial per workgroup
def test_depth_rows(env, S):
    torch, ops = env
    C, P = 2, 5
    rng = randn(torch, (C, P, S), torch.float64, 2, scale=30.0, shift=100.0)
    raw = randn(torch, (C, P, S), torch.float32, 3)
    scale, offset = randn(torch, (C, P), torch.float64, 4, n_nan=0), randn(torch, (C, P), torch.float64, 5, n_nan=0)
    coef = power_rows(torch, C, P)
    guarded(env, lambda: ops.depth_rows(scale, offset, range=rng), "depth_rows.workspace")
    guarded(env, lambda: ops.depth_rows(scale, offset, coef=coef, mask_raw=raw, shape=(C, P, S), dtype=torch.float64),
            "depth_rows.workspace")


@pytest.mark.parametrize("n", [1, 2**20 + 1])  # one workgroup; more blocks than the 1024 workgroups launched
def test_nanminmax(env, n):
    torch, ops = env
    x = randn(torch, (n,), torch.float32, 6)
    guarded(env, lambda: ops.nanminmax(x, with_nan_count=True), "nanminmax.workspace")


# ---- EK80 complex samples ------------------------------------------------------------------------------------------------
def test_sv_complex_fft_and_cw(env):
    torch, ops = env
    C, P, S, B, taps = 2, 3, 2100, 4, 64
    re, im = randn(torch, (C, P, S, B), torch.float32, 7), randn(torch, (C, P, S, B), torch.float32, 8)
    cc = complex_rows(torch, C, P)
    rep, off = replicas(torch, C, taps)
    kw = dict(replica=rep, replica_off=off, max_taps=taps, method="fft")
    for stats in (False, True):
        guarded(env, lambda: ops.sv_complex(re, im, cc, want_range_stats=stats, **kw), "sv_complex_fft.workspace")
    # one replica per (channel, filter interval): three replicas for two channels, the layout is that of W = 3
    rep3, off3 = replicas(torch, 3, taps)
    rid = torch.tensor([[0, 2, 0], [1, 1, 2]], dtype=torch.int32).cuda()
    guarded(env, lambda: ops.sv_complex(re, im, cc, replica=rep3, replica_off=off3, max_taps=taps, method="fft",
                                        replica_id=rid, want_range_stats=True), "sv_complex_fft.workspace")
    guarded(env, lambda: ops.sv_complex(re, im, cc, want_range_stats=True), "sv_complex_cw_stats.workspace")


def test_selftest_correlate(env):
    torch, ops = env
    g = torch.Generator().manual_seed(9)
    x = torch.randn((1, 2048), generator=g, dtype=torch.complex64).cuda()
    rep = torch.randn(64, generator=g, dtype=torch.complex64).cuda()
    guarded(env, lambda: ops.selftest_correlate(x, rep), "selftest_correlate.workspace")


def test_splitbeam_complex_fft(env):
    torch, ops = env
    C, P, S, B, taps = 2, 3, 2100, 4, 64
    re, im = randn(torch, (C, P, S, B), torch.float32, 12), randn(torch, (C, P, S, B), torch.float32, 13)
    rep, off = replicas(torch, C, taps)
    prm = [torch.tensor(v, dtype=torch.float64).cuda() for v in (23.0, 23.0, 0.1, -0.2)]
    guarded(env, lambda: ops.splitbeam_complex(re, im, [1, 1], prm, replica=rep, replica_off=off, max_taps=taps,
                                               method="fft"), "splitbeam_complex_fft.workspace")


# ---- the fused pass binned on depth ----------------------------------------------------------------------------------------
def test_sv_mvbs_fused_depth(env):
    torch, ops = env
    C, P, S = 2, 8, 64
    raw = randn(torch, (C, P, S), torch.float32, 14, scale=10.0, shift=-70.0)
    coef = power_rows(torch, C, P)
    scale = torch.ones((C, P), dtype=torch.float64).cuda()
    offset = torch.full((C, P), 5.0, dtype=torch.float64).cuda()
    bin_start = torch.tensor([0, 4, 8], dtype=torch.int32).cuda()
    guarded(env, lambda: ops.sv_mvbs_fused_depth(raw, coef, scale, offset, bin_start, 2, 2.0, 12, want_depth=True),
            "sv_mvbs_fused_depth.depth_stats_out")


# ---- masks -----------------------------------------------------------------------------------------------------------------
# epa_apply_masks launches min(ceil(n / 256), 65536) workgroups, a {min, max} pair each: 65536 is first reached at
# n = 65535 * 256 + 1
@pytest.mark.parametrize("n", [1000, 65535 * 256 + 1])
def test_apply_masks_minmax(env, n):
    torch, ops = env
    src = randn(torch, (n,), torch.float32, 15)
    mask = (torch.arange(n, device="cuda") % 3 != 0).to(torch.uint8)
    guarded(env, lambda: ops.apply_masks(src, [mask], want_minmax=True), "apply_masks.workspace")


def test_range_step_mean(env):
    torch, ops = env
    rng = randn(torch, (2, 3, 17), torch.float64, 16)
    guarded(env, lambda: ops.range_step_mean(rng), "range_step_mean.workspace")


def test_pool_sv_and_pool_sv_value(env):
    torch, ops = env
    C, P, S = 2, 6, 40
    sv = randn(torch, (C, P, S), torch.float64, 17, scale=8.0, shift=-70.0)
    guarded(env, lambda: ops.pool_sv(sv, 2, 1, 2, func="nanmean", threshold=3.0), "pool_sv.sum_ws", "pool_sv.cnt_ws")
    rng = (torch.arange(S, dtype=torch.float64) * 0.5).repeat(C, P, 1).cuda()
    nvalid, bad = ops.range_rows_check(rng)
    assert bad == 0
    for func, name in (("nanmean", "pool_sv_value.ws_mean"), ("nanmedian", "pool_sv_value.ws_median")):
        guarded(env, lambda: ops.pool_sv_value(sv, rng, nvalid, 2.0, 1, 1.0, 0.0, 19.5, func=func, threshold=3.0), name)


def test_nasc(env):
    torch, ops = env
    C, P, S = 2, 7, 33
    sv = randn(torch, (C, P, S), torch.float64, 18, scale=8.0, shift=-70.0)
    depth = (torch.arange(S, dtype=torch.float64) * 1.0).repeat(C, P, 1).cuda()
    # two pings per distance bin at the most: a cell then sums at most two workgroups' partials, in either order the
    # same bits (the comparison below is bit for bit; pings 4 .. 6 lie in no bin)
    bin_start = torch.tensor([0, 2, 4], dtype=torch.int32).cuda()
    guarded(env, lambda: ops.nasc(sv, depth, bin_start, 2, 7.0, 5, want_parts=True), "nasc.workspace")


def test_seafloor_angle_mask_and_median(env):
    torch, ops = env
    P, S, r0, R = 6, 40, 5, 30
    theta, phi = randn(torch, (P, S), torch.float64, 19, scale=3.0), randn(torch, (P, S), torch.float64, 20, scale=3.0)
    sv = randn(torch, (P, S), torch.float64, 21, scale=8.0, shift=-70.0)

    def run():
        state = ops.seafloor_state(sv.device)
        mask = ops.seafloor_angle_mask(theta, phi, r0, R, 3, 3, 4.0, 4.0, state)
        ops.seafloor_median(sv, r0, R, mask, state)
        return mask, state

    guarded(env, run, "seafloor.state", "seafloor_angle_mask.work", "seafloor_median.hist")


def test_shoal_echoview_link(env):
    torch, ops = env
    P, S = 8, 16
    sv = randn(torch, (P, S), torch.float32, 22)
    idim = torch.arange(S + 1, dtype=torch.float64).cuda()
    jdim = torch.arange(P + 1, dtype=torch.float64).cuda()

    def run():
        state = ops.shoal_state(sv.device)
        plane = ops.shoal_threshold_fill(sv, 0.0)
        parent, table = ops.shoal_label(plane, 8, state, with_groups=True)
        ops.shoal_echoview_link(plane, parent, table, idim, jdim, (1, 1), (2, 2), (2, 2), state)
        return plane, state[0]  # (the component ids, and with them the table, come in no particular order)

    guarded(env, run, "shoal.state", "shoal_echoview_link.queue")


def test_transient_masks(env):
    torch, ops = env
    C, P, S = 2, 6, 40
    sv = randn(torch, (C, P, S), torch.float64, 23, scale=8.0, shift=-70.0)
    chan = np.array([[5, 20, 2, 3], [4, 25, 1, 2]])
    guarded(env, lambda: ops.transient_fielding(sv, chan, 2, 3.0, 1.0, -40.0), "transient_fielding.todo",
            "transient_fielding.count")
    rows = np.tile(np.arange(S) * 0.5, (C, 1))
    chan_i, chan_d = np.array([[2, 30], [3, 28]]), np.array([[0.5, 19.5], [0.5, 19.5]])
    guarded(env, lambda: ops.transient_matecho(sv, rows, chan_i, chan_d, None, 2, 50.0, 3.0, 1, 1.0),
            "transient_matecho.s_hi", "transient_matecho.flag")


@pytest.mark.parametrize("N", [2, 1025, 2049])  # one tile; exactly one; one difference into the third
def test_time_rebuild(env, N):
    torch, ops = env
    t = torch.arange(N, dtype=torch.int64) * 1000
    t[N // 2:] -= 5000  # one reversal
    t = t.cuda()
    sub = torch.full((N - 1,), 1000, dtype=torch.int64).cuda()

    def run():
        facts, _ = ops.time_reversals(t, want_list=True)
        return ops.time_rebuild(t, facts, sub)

    guarded(env, run, "time_rebuild.tile_workspace")


def test_regrid_mask(env):
    torch, ops = env
    g = torch.Generator().manual_seed(24)
    mask = (torch.rand((1, 4, 8), generator=g) > 0.3).to(torch.uint8).cuda()
    rng = torch.arange(8, dtype=torch.float64).cuda()
    bin_start = torch.tensor([0, 4], dtype=torch.int32).cuda()
    # 1 x 1 x 5 cells: one byte into the second 32-bit word
    guarded(env, lambda: ops.regrid_mask(mask, rng, bin_start, 1, 2.0, 5), "regrid_mask.out")
