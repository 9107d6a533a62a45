"""The statistics folds of csrc/wg_reduce.h, with the deciding value PLACED.

A dropped wavefront slot or a wrong lane in a fold shows only when the value that decides the result sits in one
particular wavefront; random inputs rarely put it there.  Every test here walks the single smallest value, the single
largest value and the only NaNs through eight positions of a 256-lane workgroup -- lane 0 and lane 63 of each of its
four wavefronts -- and expects numpy's nanmin / nanmax / NaN count of the downloaded array, exactly.

In turn k the smallest value sits at POS[k], the largest at POS[k + 3] and the NaNs at POS[k + 5] (indices mod 8): over
the eight turns each of the three visits each position.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS = [0, 64, 128, 192, 63, 127, 191, 255]  # lane 0, then lane 63, of wavefronts 0..3
TURNS = range(len(POS))
DTYPES = ["float64", "float32"]


@pytest.fixture(scope="module")
def env():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("these tests need a GPU (run with -m 'not gpu' on CPU boxes)")
    from echopype_amd import ops

    return torch, ops


def _pos(k, i):
    return POS[(k + i) % len(POS)]


def _body(n, dtype, seed):
    """n numbers in [1, 1.5), distinct in float32 too: nothing here is the smallest, the largest or a NaN."""
    rng = np.random.default_rng(seed)
    return (1.0 + rng.permutation(n) / float(2 * n)).astype(dtype)


def _placed(n, dtype, k, where, seed=0):
    """The body with -5 (and the runner-up -4), 7 (runner-up 6) and one NaN placed: position p of the workgroup is
    element ``where(p)``; None leaves that one out.  -> (array, index of the smallest, index of the largest)"""
    x = _body(n, dtype, seed)
    at = {name: where(_pos(k, i)) for name, i in (("lo", 0), ("lo2", 1), ("hi", 3), ("hi2", 4), ("nan", 5))}
    for name, v in (("lo2", -4.0), ("hi2", 6.0), ("nan", np.nan), ("lo", -5.0), ("hi", 7.0)):
        if at[name] is not None:
            x[at[name]] = v
    return x, at["lo"], at["hi"]


def _expect(a):
    a = np.asarray(a, dtype=np.float64)
    return [float(np.nanmin(a)), float(np.nanmax(a)), float(np.isnan(a).sum())]


# ---- ops.nanminmax ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [256, 257, 1000])
def test_nanminmax_placed(env, n, dtype, aligned):
    """Unaligned (a view one element into its buffer): one element per lane, element i is lane i of workgroup i / 256.
    Aligned: a lane takes two 16-byte loads, ``per`` consecutive elements, then the tail is one element per lane; position
    p is then the first element of lane p where the input is that long."""
    torch, ops = env
    per = 32 // np.dtype(dtype).itemsize
    for k in TURNS:
        def where(p):
            return p * per if aligned and (p + 1) * per <= n // per * per else p
        x, _, _ = _placed(n, dtype, k, where, seed=n + k)
        buf = torch.empty(n + 1, dtype=getattr(torch, dtype), device="cuda")
        t = buf[:n] if aligned else buf[1:]
        assert (t.data_ptr() % 16 == 0) == aligned
        t.copy_(torch.from_numpy(x))
        lo, hi, nn = ops.nanminmax(t, with_nan_count=True)
        assert [lo, hi, float(nn)] == _expect(t.cpu().numpy()) == [-5.0, 7.0, 1.0], (k, lo, hi, nn)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nanminmax_placed_in_the_last_partial_workgroup(env, dtype):
    """Two workgroups, the second with three of its four wavefronts: everything placed sits in the second."""
    torch, ops = env
    n, tail = 256 + 192, 192
    for k in TURNS:
        x, _, _ = _placed(n, dtype, k, lambda p: 256 + p if p < tail else None, seed=k)
        buf = torch.empty(n + 1, dtype=getattr(torch, dtype), device="cuda")
        t = buf[1:]  # one element per lane
        t.copy_(torch.from_numpy(x))
        lo, hi, nn = ops.nanminmax(t, with_nan_count=True)
        assert [lo, hi, float(nn)] == _expect(t.cpu().numpy()), (k, lo, hi, nn)


# ---- ops.depth_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [261, 1024])  # a partial per workgroup (sample s is lane s % 256); one-piece workgroups
def test_depth_rows_placed(env, S, dtype):
    torch, ops = env
    C, P = 1, 2
    one = torch.ones((C, P), dtype=torch.float64, device="cuda")
    zero = torch.zeros((C, P), dtype=torch.float64, device="cuda")
    for k in TURNS:
        row = k % P
        x, _, _ = _placed(C * P * S, dtype, k, lambda p: row * S + p * (S // 256), seed=S + k)
        rng = torch.from_numpy(x.reshape(C, P, S)).cuda()
        depth, stats = ops.depth_rows(one, zero, range=rng)
        got = depth.cpu().numpy()
        np.testing.assert_array_equal(got, x.reshape(C, P, S))  # scale 1, offset 0: the depth is the placed range
        assert stats.cpu().tolist() == _expect(got) == [-5.0, 7.0, 1.0], k


# ---- ops.apply_masks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_masks_minmax_placed(env, dtype):
    """n = 512: two workgroups, element i is lane i % 256.  All kept: the placed extremes win.  The extremes masked (the
    fill is NaN): the runner-ups, placed one position further, win."""
    torch, ops = env
    n = 512
    for k in TURNS:
        block = k % 2
        x, ilo, ihi = _placed(n, dtype, k, lambda p: 256 * block + p, seed=k)
        src = torch.from_numpy(x).cuda()
        keep = np.ones(n, dtype=np.uint8)
        out, mm = ops.apply_masks(src, [torch.from_numpy(keep).cuda()], want_minmax=True)
        assert mm.cpu().tolist() == _expect(out.cpu().numpy())[:2] == [-5.0, 7.0], k
        keep[[ilo, ihi]] = 0
        out, mm = ops.apply_masks(src, [torch.from_numpy(keep).cuda()], want_minmax=True)
        assert mm.cpu().tolist() == _expect(out.cpu().numpy())[:2] == [-4.0, 6.0], k


# ---- ops.range_step_mean ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_range_step_mean_placed(env, dtype):
    """(1, 2, 513): 512 steps per row, step s is lane s % 256 of the row's workgroup.  The steps are multiples of 0.5
    below 4, so every summation order gives the same float64 sum; a NaN sample at position p makes the steps into and out
    of it NaN (p = 0: the one step out of it)."""
    torch, ops = env
    C, P, S = 1, 2, 513
    for k in TURNS:
        rng = np.random.default_rng(k)
        steps = rng.integers(1, 8, size=(C, P, S - 1)) * 0.5
        x = np.concatenate([np.zeros((C, P, 1)), np.cumsum(steps, axis=2)], axis=2).astype(dtype)
        x[0, k % P, POS[k] + 256 * ((k // 2) % 2)] = np.nan
        got = ops.range_step_mean(torch.from_numpy(x).cuda())
        exp = np.nanmean(np.diff(x, axis=2).astype(np.float64), axis=(1, 2))
        assert got.tolist() == exp.tolist(), (k, got, exp)


# ---- ops.sv_power -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1024, 1000, 37])  # float32: one-piece workgroups; float64: strided rows; 37: scalar path
def test_sv_power_range_stats_placed(env, S, dtype):
    """The echo_range is fixed by the coefficient rows, so only the NaNs are placed: NaN raw samples (the range is masked
    by them) in two wavefronts of two rows.  The statistics equal numpy's on the echo_range written."""
    torch, ops = env
    C, P = 1, 3
    # ra, rb, r0, shift, alpha2, A0, g, d = (shift - r0) / (ra * rb)
    coef = torch.tensor([0.02, 10.0, 0.0, 0.4, 0.01, -50.0, 0.1, 2.0], dtype=torch.float64).repeat(C, P, 1).cuda()
    rng = np.random.default_rng(S)
    for k in TURNS:
        raw = (-70.0 + 10.0 * rng.standard_normal((C, P, S))).astype(np.float32)
        spread = max(S // 256, 1)
        raw[0, k % P, _pos(k, 0) * spread % S] = np.nan
        raw[0, (k + 1) % P, _pos(k, 5) * spread % S] = np.nan
        _, er, stats = ops.sv_power(torch.from_numpy(raw).cuda(), coef, dtype=getattr(torch, dtype),
                                    want_range_stats=True)
        got = er.cpu().numpy()
        assert stats.cpu().tolist() == _expect(got), k
        assert np.isnan(got).sum() == 2
