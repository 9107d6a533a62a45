#!/usr/bin/env python3
"""``open_raw_ek80`` at a survey file's size: an EK80 file of 2 channels x 50 000 pings x 2500 samples x 4 sectors of
float32 complex samples (8 B per sample and sector: 8 GB of samples), a parameter ``XML0`` in front of every ping.  The
record of one ping time is 1 byte longer than a multiple of 4, so the complex blocks start at every byte offset mod 4.
The file is laid out here with NumPy (one record broadcast over the pings, the time stamps written as columns; sample
values from a small random pool: the contents do not change what is moved).

1. the unpack KERNEL alone -- device events around ``epa_raw3_unpack`` with the file, the row table and the two outputs
   already in HBM: median, minimum and maximum of 20 runs after 3 warm-up runs.  The entry point's host checks (one pass
   over the 100 000 rows of the table) run between the two events.  Bytes counted: the file's sample bytes read once plus
   the output bytes written once, against 8 TB/s; ``raw0_unpack_kernel`` measured 0.53 of that and
   ``concat_rows_kernel`` 0.74 on this card (README) -- comparisons, not gates;
2. as a floor that does LESS, the same planes from torch on the device for a file whose blocks are all dword-aligned and
   full: a ``view(float32)`` of the file, a strided copy per plane and ``torch.where`` for the zero rule (device events,
   same runs);
3. the host half (``parse_ek80.plan``), host clock; 4. the upload of the file's bytes (``ops.to_device``), host clock ended
   by a synchronise; 5. the whole ``open_raw_ek80`` call, file on disk (page cache) to resident EchoData, in a fresh child
   process, host clock ended by a synchronise -- ``--call-reps`` runs after one warm-up run each.

The kernel's planes are compared with the torch route's bit for bit (aligned file) and with a NumPy de-interleave of the
first and last pings (unaligned file) before anything is timed.  Writes the JSON document to ``--out`` (default
profiles/open_raw_ek80_bench.json) and prints it."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raw3_cases as R  # noqa: E402  (the datagram packers and XML texts of the test fixtures)
import echopype_amd as ep  # noqa: E402,F401
from echopype_amd import _lib, ops  # noqa: E402
from echopype_amd.convert import parse_ek80  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pings", type=int, default=50_000)
ap.add_argument("--samples", type=int, default=2500)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--call-reps", type=int, default=5, help="runs of the host plan, the upload and the whole call; 0 skips the whole call")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_raw_ek80_bench.json"))
args = ap.parse_args()
C, P, S, B, REPS, WARM = 2, args.pings, args.samples, 4, args.reps, args.warmup
HBM_PEAK = 8.0e12
CHANNELS = (R.CH70, R.CH120)
NT0 = R.NT_BASE


def summary(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(min(ts)), "ms_max": float(max(ts)), "runs": len(ts)}


def build(aligned):
    """-> (uint8 buffer padded to a multiple of 16, file bytes, byte offset of the first record, record length, byte
    offsets of the two complex blocks inside a record)."""
    rng = np.random.default_rng(2026)
    chans = [R.channel_config(cid, i + 1, f) for i, (cid, f) in enumerate(zip(CHANNELS, (70000.0, 120000.0)))]
    head = R.frame(R.pack(R.xml0(NT0 - 10_000_000, R.config_xml(chans))))
    head += R.frame(R.pack(R.xml0(NT0 - 9_000_000, R.environment_xml())))
    head += b"".join(R.frame(R.pack(R.fil1(NT0 - 8_000_000, st, cid, n, d, 7))) for cid in CHANNELS for st, n, d in ((1, 47, 6), (2, 91, 2)))
    pool = (rng.integers(-2000, 2000, (S, B)) / 64 + 1j * rng.integers(1, 2000, (S, B)) / 64).astype(np.complex64)
    rec, stamps, blocks = b"", [], []
    for c, cid in enumerate(CHANNELS):
        text = R.parameter_xml(cid, 1, 0.001024, 8e-06, 750.0, 0.05, band=(45000.0, 90000.0) if c == 0 else (90000.0, 170000.0))
        want = 0 if aligned else (1 if c == 0 else 0)  # the record's length mod 4
        nul = (want - len(text)) % 4
        for d in (R.xml0(NT0, text, nul=nul), R.raw3(NT0, cid, S, B, pool)):
            stamps.append(len(rec) + 4 + 4)  # low_date of this datagram's body
            if d["kind"] == "RAW3":
                blocks.append(len(rec) + 4 + R.RAW3_HEADER)
            rec += R.frame(R.pack(d))
    if aligned:  # the configuration in front must end on a dword as well
        head += R.frame(R.pack(R.xml0(NT0 - 7_000_000, R.PING_SEQUENCE_XML, nul=(-len(head) - 20 - len(R.PING_SEQUENCE_XML)) % 4)))
        assert len(head) % 4 == 0 and len(rec) % 4 == 0 and all(b % 4 == 0 for b in blocks)
    else:
        assert len(rec) % 4 == 1
    H, L = len(head), len(rec)
    n = H + P * L
    buf = np.zeros(-(-n // 16) * 16, dtype=np.uint8)
    buf[:H] = np.frombuffer(head, np.uint8)
    body = buf[H:n].reshape(P, L)
    body[:] = np.frombuffer(rec, np.uint8)
    ticks = NT0 + np.arange(P, dtype=np.uint64) * np.uint64(10_000_000)
    low = (ticks & np.uint64(0xFFFFFFFF)).astype("<u4").view(np.uint8).reshape(P, 4)
    high = (ticks >> np.uint64(32)).astype("<u4").view(np.uint8).reshape(P, 4)
    for s in stamps:
        body[:, s:s + 4], body[:, s + 4:s + 8] = low, high
    return buf, n, H, L, blocks


def kernel_call(dev, n_bytes, table, tab_dev, re, im):
    _lib.call("epa_raw3_unpack", ops._p(dev), n_bytes, dev.numel(), table.ctypes.data_as(ctypes.c_void_p), ops._p(tab_dev), C, P, S, B,
              ops._p(re), ops._p(im), ops._stream())


def device_timed(fn):
    ts = []
    for i in range(REPS + WARM):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(a.elapsed_time(b))
    return ts


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def plan_table(buf, n_bytes):
    pl = parse_ek80.plan(buf, n_bytes)
    (g,) = pl.groups
    assert (g.descr, g.C, g.P, g.S, g.B) == ("complex_FM", C, P, S, B) and g.rows_present == C * P
    return pl, g


CHILD = """
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
import echopype_amd as ep
ts = []
for i in range(int(sys.argv[3]) + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ed = ep.open_raw_ek80(sys.argv[2])
    torch.cuda.synchronize()
    if i >= 1:
        ts.append((time.perf_counter() - t0) * 1e3)
    del ed
print(json.dumps({"ms": ts}))
"""

nan = float("nan")
res = {"device": torch.cuda.get_device_name(0)}

# ---- the aligned file: the torch floor, and the kernel against it ----------------------------------------------------------
buf, n_bytes, H, L, blocks = build(aligned=True)
pl, g = plan_table(buf, n_bytes)
dev = ops.to_device(buf)
del buf
tab_dev = ops.to_device(g.table)
re = torch.empty((C, P, S, B), dtype=torch.float32, device=dev.device)
im = torch.empty((C, P, S, B), dtype=torch.float32, device=dev.device)
re2, im2 = torch.empty_like(re), torch.empty_like(im)
f32 = dev[H:H + P * L].view(torch.float32).view(P, L // 4)
nan_t = torch.full((), nan, dtype=torch.float32, device=dev.device)


def torch_route():
    for c in range(C):
        blk = f32[:, blocks[c] // 4:blocks[c] // 4 + 2 * S * B].view(P, S, B, 2)
        re2[c].copy_(blk[..., 0])
        torch.where(blk[..., 1] == 0, nan_t, blk[..., 1], out=im2[c])


with _lib.launch_trace() as tr:
    kernel_call(dev, n_bytes, g.table, tab_dev, re, im)
assert tr.kernels == ["raw3_unpack_kernel"], tr.kernels
torch_route()
assert torch.equal(re.view(torch.int32), re2.view(torch.int32)) and torch.equal(im.view(torch.int32), im2.view(torch.int32))
t_floor = device_timed(torch_route)
t_kernel_aligned = device_timed(lambda: kernel_call(dev, n_bytes, g.table, tab_dev, re, im))
del dev, f32, re2, im2, tab_dev

# ---- the unaligned file: the kernel alone, the host half, the upload, the whole call ------------------------------------------
buf, n_bytes, H, L, blocks = build(aligned=False)
t_host = []
for i in range(max(1, args.call_reps) + 1):
    t0 = time.perf_counter()
    pl, g = plan_table(buf, n_bytes)
    if i >= 1:
        t_host.append((time.perf_counter() - t0) * 1e3)
residues = sorted({int(v) % 4 for v in g.table[:64, 0]})
assert residues == [0, 1, 2, 3] and pl.xml_count == 2 + C * P and pl.xml_texts == 2 + C
t_up = []
for i in range(max(1, args.call_reps) + 1):
    ms, dev = host_timed(lambda: ops.to_device(buf))
    if i >= 1:
        t_up.append(ms)
    if i < max(1, args.call_reps):
        del dev
tab_dev = ops.to_device(g.table)
kernel_call(dev, n_bytes, g.table, tab_dev, re, im)
for p in (0, P - 1):  # against a NumPy de-interleave of the file's own bytes
    for c in range(C):
        a = H + p * L + blocks[c]
        x = buf[a:a + 8 * S * B].view("<f4").reshape(S, B, 2)
        assert np.array_equal(re[c, p].cpu().numpy().view(np.int32), x[..., 0].view(np.int32))
        want = np.where(x[..., 1] == 0, np.float32(np.nan), x[..., 1])
        assert np.array_equal(im[c, p].cpu().numpy().view(np.int32), want.view(np.int32))
t_kernel = device_timed(lambda: kernel_call(dev, n_bytes, g.table, tab_dev, re, im))
del dev, re, im, tab_dev
t_call = None
if args.call_reps > 0:
    tmp = tempfile.mkdtemp(prefix="open_raw_ek80_bench_")
    path = os.path.join(tmp, "bench.raw")
    try:
        buf[:n_bytes].tofile(path)
        del buf
        env = {k: v for k, v in os.environ.items() if k != "ECHOPYPE_AMD_LIB"}
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, str(args.call_reps)], capture_output=True, text=True, env=env,
                           timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"open_raw_ek80 in the child process failed:\n{r.stderr[-2000:]}")
        t_call = json.loads(r.stdout.strip().splitlines()[-1])["ms"]
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(tmp)

elements = C * P * S * B
need = elements * 8 + elements * 8  # a float32 pair of the file per element read, two float32 planes written
k, ka, fl = summary(t_kernel), summary(t_kernel_aligned), summary(t_floor)
frac = lambda s: need / (s["ms_median"] * 1e-3) / HBM_PEAK  # noqa: E731
res.update({
    "workload": {"channels": C, "pings": P, "range_samples": S, "sectors": B, "file_bytes": n_bytes, "record_bytes": L,
                 "complex_block_offsets_mod_4": residues, "parameter_XML0_in_front_of_every_ping": True,
                 "XML0_datagrams": pl.xml_count, "distinct_XML0_texts_parsed": pl.xml_texts},
    "bit_equal_to_the_torch_route_and_to_numpy": True,
    "tuning": "untuned, one run: one wavefront per row, aligned dword loads + byte shift, 8 dwords in and two 16-byte "
              "non-temporal stores out per lane and step, the chunk loop unrolled twice",
    "bytes_counted": "file sample bytes (8 B per sample and sector) + output bytes (two float32 planes), once each",
    "raw3_unpack_kernel_alone_by_device_events": {**k, "TB_per_s_median": need / (k["ms_median"] * 1e-3) / 1e12,
                                                  "fraction_of_8_TB_per_s": frac(k),
                                                  "raw0_unpack_kernel_fraction_for_comparison": 0.53,
                                                  "concat_rows_kernel_fraction_for_comparison": 0.74},
    "raw3_unpack_kernel_on_the_dword_aligned_file": {**ka, "fraction_of_8_TB_per_s": frac(ka)},
    "torch_view_gather_floor_on_the_dword_aligned_file": {**fl, "fraction_of_8_TB_per_s": frac(fl)},
    "host_plan": summary(t_host),
    "upload_of_the_file_bytes": {**summary(t_up), "GB_per_s_median": n_bytes / (float(np.median(t_up)) * 1e-3) / 1e9},
    "open_raw_ek80_whole_call_in_a_fresh_process": summary(t_call) if t_call else None,
})
doc = json.dumps(res, indent=1)
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
print(doc)
