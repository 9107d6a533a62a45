#!/usr/bin/env python3
"""The two kernels of csrc/mask_grid.hip at a workload-sized shape, each next to the torch expression that computes the
same thing, in one run: ``epa_freq_diff_mask`` on two planes of a float32 4 x 20 000 x 4096 cube (9 B per sample: two
reads and the mask byte), ``epa_regrid_mask`` on a 20 000 x 4096 uint8 mask onto 20 s x 1 m cells with a 1-D range
(1 B per sample) and with a range per sample (9 B per sample).  Median and minimum of the timed calls in ms (HIP events
around each call), the algorithmic bytes per second, and an equality check of the two computations.  Prints one JSON
document."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echopype_amd import ops  # noqa: E402


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


res = {}
C, P, S = 4, 20000, 4096
sv = (torch.randint(-80, -20, (C, P, S), device="cuda").float() * 0.5)
n = P * S
med, mn = timed(lambda: ops.freq_diff_mask(sv, 0, 2, ">=", 10.0))
res["freq_diff_f32"] = {"shape": [C, P, S], "ms_median": med, "ms_min": mn, "bytes": 9 * n, "TB_per_s": 9 * n / med / 1e9}
med, mn = timed(lambda: (sv[0] - sv[2]) >= 10.0)
res["freq_diff_f32_torch"] = {"ms_median": med, "ms_min": mn}
assert torch.equal(ops.freq_diff_mask(sv, 0, 2, ">=", 10.0), (sv[0] - sv[2]) >= 10.0)
del sv

mask = (torch.rand((1, P, S), device="cuda") < 0.98).to(torch.uint8)
rng = torch.arange(S, dtype=torch.float64, device="cuda") * 0.19
pt = torch.arange(P, dtype=torch.int64, device="cuda") * 10**9
n_t, rb = P // 20, 1.0
n_r = int(len(np.arange(0, float(rng.max()) + 1e-8 + rb, rb)) - 1)
bs = ops.time_bin_offsets(pt, 0, 20 * 10**9, n_t)
med, mn = timed(lambda: ops.regrid_mask(mask, rng, bs, n_t, rb, n_r))
res["regrid_1d"] = {"shape": [P, S], "grid": [n_t, n_r], "ms_median": med, "ms_min": mn, "bytes": n, "TB_per_s": n / med / 1e9}
ri = torch.clamp((rng / rb).floor().long(), max=n_r - 1)
ti = torch.arange(P, device="cuda") // 20


def torch_regrid():
    cell = (ti[:, None] * n_r + ri[None, :]).reshape(-1)
    cnt = torch.zeros(n_t * n_r, dtype=torch.float32, device="cuda").index_add_(0, cell, torch.ones(n, device="cuda"))
    one = torch.zeros(n_t * n_r, dtype=torch.float32, device="cuda").index_add_(0, cell, mask.reshape(-1).float())
    return (cnt > 0) & (one == cnt)


med, mn = timed(torch_regrid, reps=5, warm=1)
res["regrid_1d_torch_index_add"] = {"ms_median": med, "ms_min": mn}
got = ops.regrid_mask(mask, rng, bs, n_t, rb, n_r)[0][0].bool()
assert torch.equal(got.reshape(-1), torch_regrid())
rng2 = rng[None, :].expand(P, S).contiguous()
med, mn = timed(lambda: ops.regrid_mask(mask, rng2, bs, n_t, rb, n_r), reps=10)
res["regrid_2d_range"] = {"ms_median": med, "ms_min": mn, "bytes": 9 * n, "TB_per_s": 9 * n / med / 1e9}
assert torch.equal(ops.regrid_mask(mask, rng2, bs, n_t, rb, n_r)[0][0].bool(), got)
print(json.dumps(res, indent=1))
