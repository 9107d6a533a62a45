"""mask.detect_shoal on the GPU (csrc/shoal.hip through ops.shoal_* and the shoal_detection package): every
reference-executed golden case bit for bit (boolean results: equality, no tolerance), seeded fuzz against
tests/shoal_ref.py (sizes across the 64-sample steps and the 128-ping chunks of the fill kernels), label shapes that
make long union-find chains, one huge component among thousands of small ones, device-resident results with only the
documented host read, the chain from EK60 samples into apply_mask, and full-size planes whose expected mask is a
formula (a lattice of rectangles with chosen gaps and sizes)."""
import numpy as np
import pytest

import shoal_ref as R
from test_shoal_host import _cases, _lite_ds, _params

pytestmark = pytest.mark.gpu

W = {"var_name": "Sv", "channel": "chan1"}


@pytest.fixture(scope="module")
def g():
    return R.load_goldens()


def _to_dev(ds):
    """The same dataset with every variable as a device array."""
    import torch

    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    out = Dataset(coords={k: c for k, c in ds.coords.items()})
    for k, v in ds.data_vars.items():
        out[k] = DataArray(DeviceArray(torch.as_tensor(np.ascontiguousarray(v.values)).cuda()), v.dims, name=k)
    return out


@pytest.mark.parametrize("on_device", [False, True])
def test_every_golden_case(g, on_device):
    import torch

    import echopype_amd as ep

    n = 0
    for c in _cases(g):
        ds = _lite_ds(g[c["sv"]], c["layout"])
        if on_device:
            ds = _to_dev(ds)
        if "error" in c:
            typ, msg = c["error"]
            with pytest.raises(Exception) as ei:
                ep.mask.detect_shoal(ds, c["method"], _params(g, c))
            assert type(ei.value).__name__ == typ and str(ei.value) == msg, c["tag"]
            continue
        out = ep.mask.detect_shoal(ds, c["method"], _params(g, c))
        t = out.data.tensor
        assert t.is_cuda and t.dtype == torch.bool, c["tag"]
        want = torch.from_numpy(R.unpack_mask(g, c["tag"], c["shape"])).cuda()
        assert torch.equal(t, want), (c["tag"], int(t.sum()), c["count"])
        assert out.name == c["name"] and list(out.dims) == c["dims"], c["tag"]
        assert dict(out.attrs) == c["attrs"], c["tag"]
        np.testing.assert_array_equal(out.coords["ping_time"], np.arange(c["shape"][0]))
        np.testing.assert_array_equal(out.coords["range_sample"], np.arange(c["shape"][1]))
        n += 1
    assert n >= 60


def _run(method, sv, params, want=None):
    import torch

    import echopype_amd as ep

    prm = dict(W, **params)
    out = ep.mask.detect_shoal(_lite_ds(sv), method, prm)
    if want is None:
        kw = {k: v for k, v in params.items()}
        want = R.weill(sv, **kw) if method == "weill" else R.echoview(sv, **kw)
    got = out.data.tensor
    assert got.dtype == torch.bool
    bad = int((got != torch.from_numpy(want).cuda()).sum())
    assert bad == 0, (method, params if method == "weill" else "", bad, int(got.sum()), int(want.sum()))
    return want


@pytest.mark.parametrize("seed,P,S,dtype,prm", [
    (1, 300, 700, np.float64, dict(thr=-68.0, maxvgap=3, maxhgap=2, minvlen=4, minhlen=3)),
    (2, 517, 333, np.float32, dict(maxvgap=5, maxhgap=0, minvlen=0, minhlen=0)),       # S not a multiple of 64
    (3, 129, 65, np.float64, dict(maxvgap=70, maxhgap=140, minvlen=2, minhlen=2)),      # gaps beyond a step / a chunk
    (4, 1200, 300, np.float32, dict(thr=-66.0, maxvgap=1, maxhgap=7, minvlen=3, minhlen=9)),
    (5, 128, 64, np.float32, dict(maxvgap=2, maxhgap=2, minvlen=2, minhlen=2)),         # exactly one step, one chunk
    (6, 257, 129, np.float64, dict(maxvgap=0, maxhgap=300, minvlen=1.5, minhlen=0)),    # runs across two chunk seams
    (7, 640, 200, np.float32, dict(maxvgap=2.5, maxhgap=1.5, minvlen=0, minhlen=6)),
])
def test_weill_fuzz_against_the_oracle(seed, P, S, dtype, prm):
    from echopype_amd import synth

    sv = synth.shoal_scene(P=P, S=S, seed=seed, dtype=dtype, schools=8)
    want = _run("weill", sv, prm)
    assert 0 < want.sum() < want.size


def _axes(P, S, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return np.arange(S + 1) * 0.5, np.arange(P + 1) * 2.0
    if kind == "irregular":
        return (np.concatenate([[0.0], np.cumsum(rng.uniform(0.2, 1.5, S))]),
                np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 4.0, P))]))
    # repeated edges along both axes (zero-height samples, zero-width pings)
    return np.repeat(np.arange(S // 2 + 2) * 1.0, 2)[:S + 1], np.repeat(np.arange(P // 3 + 2) * 3.0, 3)[:P + 1]


@pytest.mark.parametrize("seed,P,S,dtype,kind,sizes", [
    (11, 300, 700, np.float64, "uniform", dict(mincan=(1.0, 4.0), maxlink=(2.0, 6.0), minsho=(4.0, 12.0))),
    (12, 517, 333, np.float32, "irregular", dict(mincan=(1.5, 3.0), maxlink=(2.0, 5.0), minsho=(3.0, 9.0))),
    (13, 129, 65, np.float64, "repeated", dict(mincan=(1.0, 3.0), maxlink=(1.0, 2.0), minsho=(2.0, 6.0))),
    (14, 1200, 300, np.float32, "uniform", dict(mincan=(0.0, 0.0), maxlink=(-3.0, -2.0), minsho=(3.0, 9.0))),
    (15, 400, 500, np.float32, "irregular", dict(mincan=(1.0, 2.0), maxlink=(-1.5, 0.0), minsho=(5.0, 20.0))),
    (16, 640, 200, np.float64, "repeated", dict(mincan=(1.0, 0.0), maxlink=(0.0, -1.0), minsho=(2.0, 6.0))),
    (17, 350, 350, np.float32, "uniform", dict(mincan=(0.5, 2.0), maxlink=(30.0, 120.0), minsho=(40.0, 200.0))),
])
def test_echoview_fuzz_against_the_oracle(seed, P, S, dtype, kind, sizes):
    from echopype_amd import synth

    sv = synth.shoal_scene(P=P, S=S, seed=seed, dtype=dtype, schools=8)
    idim, jdim = _axes(P, S, kind, seed)
    want = _run("echoview", sv, dict(idim=idim, jdim=jdim, thr=-69.0, **sizes))
    assert 0 < want.sum() < want.size


def _spiral(n):
    fg = np.zeros((n, n), dtype=bool)
    lo, hi = 1, n - 2
    while lo <= hi:  # a square spiral of 1-pixel arms, 1 pixel apart
        fg[lo, lo:hi + 1] = True
        fg[lo:hi + 1, hi] = True
        fg[hi, lo:hi + 1] = True
        if lo + 2 <= hi:
            fg[lo + 2:hi + 1, lo] = True
            fg[lo + 2, lo:lo + 3] = True
        lo, hi = lo + 2, hi - 2
    return fg


def test_spiral_is_one_component():
    n = 257
    fg = _spiral(n)
    sv = np.where(fg, -30.0, -90.0)
    ax = np.arange(n + 1, dtype=np.float64)
    # one component under both connectivities: it stands or falls as a whole with a length only the whole spiral has
    np.testing.assert_array_equal(_run("weill", sv, dict(maxvgap=0, minvlen=n - 2, minhlen=n - 2)), fg)
    assert not _run("weill", sv, dict(maxvgap=0, minvlen=n - 1)).any()
    np.testing.assert_array_equal(
        _run("echoview", sv, dict(idim=ax, jdim=ax, mincan=(n - 2.0, n - 2.0), maxlink=(0.0, 0.0),
                                  minsho=(n - 2.0, n - 2.0))), fg)
    assert not _run("echoview", sv, dict(idim=ax, jdim=ax, mincan=(n - 1.0, 1.0), maxlink=(0.0, 0.0),
                                         minsho=(1.0, 1.0))).any()


def test_checkerboard_links_only_diagonally():
    P, S = 700, 900
    fg = (np.add.outer(np.arange(P), np.arange(S)) % 2) == 0
    fg[:, :5] = False
    sv = np.where(fg, -30.0, -90.0).astype(np.float32)
    # echoview: one component as large as the board; weill: one component per pixel, none survives a length of 2
    want = _run("echoview", sv, dict(idim=np.arange(S + 1.0), jdim=np.arange(P + 1.0), mincan=(S - 5.0, P * 1.0),
                                     maxlink=(0.0, 0.0), minsho=(S - 5.0, P * 1.0)))
    np.testing.assert_array_equal(want, fg)
    assert not _run("weill", sv, dict(maxvgap=0, minvlen=2)).any()
    np.testing.assert_array_equal(_run("weill", sv, dict(maxvgap=0, minvlen=1, minhlen=1)), fg)


def test_one_huge_component_among_thousands_of_small_ones():
    """Every lane of the box kernel on one root, and a link box far above the size one wave scans."""
    P, S = 1500, 1300
    rng = np.random.default_rng(21)
    sv = np.full((P, S), -90.0, dtype=np.float32)
    sv[rng.random((P, S)) < 0.02] = -60.0        # about 39 000 specks
    sv[200:1300, 150:1100] = -40.0               # one school of 1100 x 950 pixels ...
    sv[400:900, 300:700] = -90.0                 # ... with a hole that holds specks of its own
    sv[400:900, 300:700][rng.random((500, 400)) < 0.02] = -60.0
    idim, jdim = np.arange(S + 1.0), np.arange(P + 1.0)
    want = _run("echoview", sv, dict(idim=idim, jdim=jdim, mincan=(1.0, 1.0), maxlink=(2.0, 2.0), minsho=(6.0, 6.0)))
    assert want[250, 200] and want.sum() > 800_000
    _run("echoview", sv, dict(idim=idim, jdim=jdim, mincan=(2.0, 2.0), maxlink=(1.0, 1.0), minsho=(3.0, 3.0)))
    _run("weill", sv, dict(maxvgap=2, maxhgap=2, minvlen=4, minhlen=4))


def test_results_stay_on_the_device(monkeypatch):
    """Device input: the plane is read where it is, the mask stays in HBM, and the host reads only what the docstrings
    list (one error word with labelling, nothing without); torch.cuda.synchronize is never called."""
    import torch

    import echopype_amd as ep
    from echopype_amd import synth
    from echopype_amd.mask.shoal_detection import utils

    sv = synth.shoal_scene(P=200, S=300, seed=31, dtype=np.float32)
    ds = _to_dev(_lite_ds(sv))
    reads = []
    real_read = utils._to_host
    monkeypatch.setattr(utils, "_to_host", lambda t: (reads.append(t.numel()), real_read(t))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("synchronize"))
    a = ep.mask.detect_shoal(ds, "weill", W)
    assert a.data.tensor.is_cuda and reads == []
    b = ep.mask.detect_shoal(ds, "weill", dict(W, minvlen=3, minhlen=2))
    assert b.data.tensor.is_cuda and reads == [1]
    reads.clear()
    idim, jdim = np.arange(301.0), np.arange(201.0)
    c = ep.mask.detect_shoal(ds, "echoview", dict(W, idim=idim, jdim=jdim))
    assert c.data.tensor.is_cuda and reads == [1]
    monkeypatch.undo()
    np.testing.assert_array_equal(a.values, R.weill(sv))
    np.testing.assert_array_equal(b.values, R.weill(sv, minvlen=3, minhlen=2))
    np.testing.assert_array_equal(c.values, R.echoview(sv, idim, jdim))


def test_chain_from_ek60_samples_into_apply_mask():
    """compute_Sv -> detect_shoal -> apply_mask, everything on the device, against the host's np.where."""
    import echopype_amd as ep
    from echopype_amd import echodata, synth

    d = synth.ek60_numpy(2, 96, 400)
    ds = ep.calibrate.compute_Sv(echodata.from_ek60_arrays(d))
    ch = str(np.asarray(ds["channel"].values)[1])
    sv = np.asarray(ds["Sv"].values)[1]
    thr = float(np.nanpercentile(sv, 80))
    mw = ep.mask.detect_shoal(ds, "weill", {"var_name": "Sv", "channel": ch, "thr": thr, "maxvgap": 2, "maxhgap": 1,
                                            "minvlen": 3, "minhlen": 2})
    want = R.weill(sv, thr, 2, 1, 3, 2)
    assert 0 < want.sum() < want.size and mw.attrs["channel"] == ch
    np.testing.assert_array_equal(mw.values, want)
    idim, jdim = np.arange(sv.shape[1] + 1) * 0.2, np.arange(sv.shape[0] + 1) * 1.0
    me = ep.mask.detect_shoal(ds, "echoview", {"var_name": "Sv", "channel": ch, "idim": idim, "jdim": jdim,
                                               "thr": thr, "mincan": (0.4, 2.0), "maxlink": (0.4, 2.0),
                                               "minsho": (1.0, 4.0)})
    np.testing.assert_array_equal(me.values, R.echoview(sv, idim, jdim, thr, (0.4, 2.0), (0.4, 2.0), (1.0, 4.0)))
    masked = ep.mask.apply_mask(ds, mw)
    assert masked["Sv"].data.tensor.is_cuda
    got = np.asarray(masked["Sv"].values)
    full = np.asarray(ds["Sv"].values)
    np.testing.assert_array_equal(got, np.where(want[None], full, np.nan))


def test_library_argument_checks():
    import torch

    from echopype_amd import ops

    sv = torch.full((8, 16), -90.0, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="plane expected"):
        ops.shoal_threshold_fill(sv[0], -70.0)
    with pytest.raises(ValueError, match="plane expected"):
        ops.shoal_threshold_fill(sv.half(), -70.0)
    plane = ops.shoal_threshold_fill(sv, -70.0)
    state = ops.shoal_state(sv.device)
    with pytest.raises(ValueError, match="connectivity 6"):
        ops.shoal_label(plane, 6, state)
    parent, table = ops.shoal_label(plane, 8, state, with_groups=True)
    small = dict(table, cap=table["cap"] - 1)
    with pytest.raises(ValueError, match="table capacity"):
        ops.shoal_weill_filter(plane, parent, small, 0, 0, state)
    idim = torch.arange(17, dtype=torch.float64, device="cuda")
    jdim = torch.arange(9, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="idim needs at least"):
        ops.shoal_echoview_link(plane, parent, table, idim[:16], jdim, (0, 0), (0, 0), (0, 0), state)
    with pytest.raises(ValueError, match="NULL array"):
        ops.shoal_echoview_link(plane, parent, dict(table, group=None), idim, jdim, (0, 0), (0, 0), (0, 0), state)
    ops.shoal_echoview_link(plane, parent, table, idim, jdim, (0, 0), (0, 0), (0, 0), state)
    assert not plane.any() and int(state[0]) == 0


# ---- full size: a lattice of rectangles whose expected mask is a formula ------------------------------------------------
def _segments(n, period, start, length, gap_at, gap_len, max_gap):
    """Along one axis: cell k holds [start, start + length(k)) with a gap of gap_len(k) at offset gap_at, filled when
    gap_len(k) <= max_gap.  -> (input foreground, the segment length each index belongs to after filling, 0 outside)."""
    idx = np.arange(n)
    k, o = idx // period, idx % period - start
    ln, gl = length(k), gap_len(k)
    inside = (o >= 0) & (o < ln)
    in_gap = inside & (o >= gap_at) & (o < gap_at + gl)
    filled = gl <= max_gap
    seg = np.where(filled, ln, np.where(o < gap_at, gap_at, ln - gap_at - gl))
    seg = np.where(inside & (filled | ~in_gap), seg, 0)
    return inside & ~in_gap, seg


def _lattice_weill(P, S, maxvgap=2, maxhgap=2, minvlen=5, minhlen=10):
    s_in, s_seg = _segments(S, 50, 3, lambda b: 10 + (b % 3) * 10, 4, lambda b: 1 + b % 4, maxvgap)
    p_in, p_seg = _segments(P, 40, 2, lambda a: 8 + (a % 2) * 12, 3, lambda a: 1 + a % 4, maxhgap)
    return p_in, s_in, p_seg >= max(minhlen, 1), s_seg >= max(minvlen, 1)


def _outer(p, s):
    import torch

    pt, st = torch.from_numpy(p).cuda()[:, None], torch.from_numpy(s).cuda()[None, :]
    return pt & st


def _sv_from(fg, dtype):
    import torch

    return torch.where(fg, torch.tensor(-50.0, dtype=dtype, device="cuda"), torch.tensor(-90.0, dtype=dtype,
                                                                                         device="cuda"))


def _dev_ds(sv):
    from echopype_amd.xr_lite import DataArray, Dataset, DeviceArray

    P, S = sv.shape
    ds = Dataset(coords={"channel": np.array(["chan1"]), "ping_time": np.arange(P), "range_sample": np.arange(S)})
    ds["Sv"] = DataArray(DeviceArray(sv[None]), ("channel", "ping_time", "range_sample"), name="Sv")
    return ds


def test_lattice_formula_is_the_oracle():
    """The formula of the full-size tests, checked against the oracle at a size it can run."""
    P, S = 400, 300
    p_in, s_in, p_keep, s_keep = _lattice_weill(P, S)
    sv = np.where(np.outer(p_in, s_in), -50.0, -90.0)
    want = R.weill(sv, maxvgap=2, maxhgap=2, minvlen=5, minhlen=10)
    np.testing.assert_array_equal(want, np.outer(p_keep, s_keep))
    assert 0 < want.sum() < np.outer(p_in, s_in).sum()
    pe, se, pk, sk, prm = _lattice_echoview(P, S)
    sv = np.where(np.outer(pe, se), -50.0, -90.0)
    want = R.echoview(sv, **prm)
    np.testing.assert_array_equal(want, np.outer(pk, sk))
    assert 0 < want.sum() < np.outer(pe, se).sum()


def _lattice_echoview(P, S):
    """Rectangles hs(b) x hp(a) in cells of 50 samples x 40 pings; the cells 2k, 2k + 1 along range sit 3 samples
    apart (linked with maxlink[0] = 3), pairs 40 and more apart; nothing links along pings.  Unit edges."""
    mincan, maxlink, minsho = (6.0, 9.0), (3.0, 0.0), (20.0, 12.0)
    b = np.arange(S // 50 + 1)
    hs = 4 + (b % 5) * 4                                  # 4, 8, 12, 16, 20 samples high
    start = np.where(b % 2 == 0, 50 * b + 47 - hs, 50 * b)  # even cells end at 50 b + 46, odd ones start at 50 b
    end = start + hs                                      # exclusive; even -> odd gap: 50 (b + 1) - (50 b + 47) = 3
    alive = hs >= mincan[0]
    s_in, s_keep = np.zeros(S, dtype=bool), np.zeros(S, dtype=bool)
    for k in range(0, len(b), 2):
        mem = [m for m in (k, k + 1) if m < len(b) and alive[m] and end[m] <= S]
        all_in = [m for m in (k, k + 1) if m < len(b) and end[m] <= S]
        for m in all_in:
            s_in[start[m]:end[m]] = True
        if mem and end[mem[-1]] - start[mem[0]] >= minsho[0]:
            for m in mem:
                s_keep[start[m]:end[m]] = True
    idx = np.arange(P)
    a, o = idx // 40, idx % 40 - 2
    hp = 6 + (a % 3) * 4                                   # 6, 10, 14 pings wide
    p_in = (o >= 0) & (o < hp)
    p_keep = p_in & (hp >= mincan[1]) & (hp >= minsho[1])
    prm = dict(idim=np.arange(S + 1.0), jdim=np.arange(P + 1.0), mincan=mincan, maxlink=maxlink, minsho=minsho)
    return p_in, s_in, p_keep, s_keep, prm


def test_full_size_weill():
    import torch

    import echopype_amd as ep

    P, S = 200_000, 2500
    p_in, s_in, p_keep, s_keep = _lattice_weill(P, S)
    ds = _dev_ds(_sv_from(_outer(p_in, s_in), torch.float32))
    out = ep.mask.detect_shoal(ds, "weill", dict(W, maxvgap=2, maxhgap=2, minvlen=5, minhlen=10))
    want = _outer(p_keep, s_keep)
    assert torch.equal(out.data.tensor, want) and int(want.sum()) > 10_000_000


def test_full_size_echoview():
    import torch

    import echopype_amd as ep

    P, S = 200_000, 2500
    pe, se, pk, sk, prm = _lattice_echoview(P, S)
    ds = _dev_ds(_sv_from(_outer(pe, se), torch.float32))
    out = ep.mask.detect_shoal(ds, "echoview", dict(W, **prm))
    want = _outer(pk, sk)
    assert torch.equal(out.data.tensor, want) and int(want.sum()) > 10_000_000


def test_more_than_2_to_31_pixels():
    """One plane of 1 100 000 x 2000 = 2.2e9 pixels through the whole weill path (64-bit pixel indices)."""
    import torch

    import echopype_amd as ep

    P, S = 1_100_000, 2000
    assert P * S > 2 ** 31
    p_in, s_in, p_keep, s_keep = _lattice_weill(P, S)
    ds = _dev_ds(_sv_from(_outer(p_in, s_in), torch.float32))
    out = ep.mask.detect_shoal(ds, "weill", dict(W, maxvgap=2, maxhgap=2, minvlen=5, minhlen=10))
    want = _outer(p_keep, s_keep)
    assert torch.equal(out.data.tensor, want)
    assert bool(out.data.tensor[-40:].any()) and bool(out.data.tensor[:, -100:].any())  # kept shoals in the last cells
