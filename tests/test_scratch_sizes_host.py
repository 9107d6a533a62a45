"""Host-side checks of the scratch sizes the library answers for (``epa_scratch_bytes``), of the three decisions ``ops``
asks it before a call, and of the plain constants of ``_lib`` against the header.  Pure host arithmetic in the built
library: no GPU.

The formulas typed here are the record of what ``ops.py`` allocated before the library sized its own scratch; the
library must keep returning exactly these values."""
import itertools
import os
import re

import pytest
import torch

from echopype_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "echopype_amd.h")

S_GRID = (1, 4, 255, 256, 257, 1024, 1025, 2100, 8388608, 8388609)  # the last two: past 8192 chunks of 1024
CP_GRID = ((1, 1), (1, 8191), (2, 4096), (1, 8193), (3, 5))          # C * P = 1, 8191, 8192, 8193, and a plain one
N_GRID = (1, 2, 1024, 1025, 1026, 2049)


def fft_ws_doubles(W, P, S):
    return 768 + 4 * W + 3 * W * 2048 + 3 * 1024 + 2 + (W * P * (S // 1025 + 1) + 63) // 64 + W * (S + 4) + 256


def expected_sizes():
    """(what, (a, b, c), bytes before this query existed) over the grid."""
    rows = []
    for S in S_GRID:
        rows.append(("sv_power_stats.workspace", (S, 0, 0), 8 * 3 * (S // 256 + 8192 + 1024)))
    for what, n in (("depth_rows.workspace", 8 * 3 * 16384), ("nanminmax.workspace", 8 * 3072),
                    ("sv_complex_cw_stats.workspace", 8 * 3072), ("sv_mvbs_fused_depth.depth_stats_out", 8 * 64),
                    ("apply_masks.workspace", 8 * 131072), ("seafloor.state", 8 * 16), ("seafloor_median.hist", 8 * 512),
                    ("shoal.state", 8 * 8), ("shoal_echoview_link.queue", 4 * 2 * 4096), ("transient_fielding.count", 4)):
        rows.append((what, (0, 0, 0), n))
    rows.append(("selftest_correlate.workspace", (1, 1, 1), 8 * fft_ws_doubles(1, 1, 1)))
    for (C, P), S in itertools.product(CP_GRID, (1, 1024, 1025, 2100)):
        for W in (C, C + 3):  # W > C: more replicas than channels
            rows.append(("sv_complex_fft.workspace", (W, P, S), 8 * fft_ws_doubles(W, P, S)))
            rows.append(("sv_complex_fft_indexed.workspace", (W, P, S), 8 * fft_ws_doubles(W, P, S)))
        rows.append(("pool_sv.sum_ws", (C, P, S), 8 * C * P * S))
        rows.append(("pool_sv.cnt_ws", (C, P, S), 4 * C * P * S))
        rows.append(("pool_sv_value.ws_mean", (C, P, S), (C * P * S * 40 + C * S * 8 + C * 8 + C * P + 7) // 8 * 8))
        rows.append(("pool_sv_value.ws_median", (C, S, 0), (2 * C * S + 2 * C) * 4))
        rows.append(("nasc.workspace", (C, P, S), 24 * C * P * S))
        rows.append(("regrid_mask.out", (C, P, S), (C * P * S + 3) // 4 * 4))
    for n in (0, 1, 2, 7):
        rows.append(("splitbeam_complex_fft.workspace", (n, 0, 0), 8 * (768 + 3 * n * 2048)))
    for C, P in CP_GRID:
        rows.append(("range_step_mean.workspace", (C, P, 0), 8 * 2 * C * P))
        rows.append(("seafloor_angle_mask.work", (C, P, 0), 8 * 2 * C * P))  # (P, R)
        rows.append(("transient_fielding.todo", (C, P, 0), 8 * C * P))
        rows.append(("transient_matecho.s_hi", (C, P, 0), 4 * C * P))
        rows.append(("transient_matecho.flag", (C, P, 0), C * P))
    for N in N_GRID:
        rows.append(("time_rebuild.tile_workspace", (N, 0, 0), 8 * ((N - 1 + 1023) // 1024)))
    return rows


def test_scratch_bytes_equal_the_sizes_allocated_before():
    rows = expected_sizes()
    for what, abc, want in rows:
        assert ops.scratch_bytes(what, *abc) == want, (what, abc)
    # every name of the header's table was asked
    txt = open(HEADER).read()
    table = txt[txt.index(" *   what "):txt.index("int epa_scratch_bytes(")]
    names = set()
    for line in table.splitlines()[1:]:
        m = re.match(r" \*   ([a-z0-9_]+\.[a-z_]+)(?: / ([a-z0-9_]*\.[a-z_]+))?", line)
        if m:
            names.add(m.group(1))
            if m.group(2):
                names.add(m.group(2) if not m.group(2).startswith(".") else m.group(1).split(".")[0] + m.group(2))
    assert len(names) >= 27 and names == {what for what, _, _ in rows}


def test_unknown_scratch_name_raises():
    with pytest.raises(ValueError, match="no scratch buffer"):
        ops.scratch_bytes("sv_power_stats.no_such_parameter")
    with pytest.raises(ValueError, match="negative"):
        ops.scratch_bytes("nasc.workspace", -1, 1, 1)


class _Ptr:
    """What ``sv_power_vectorized`` reads of a tensor."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def test_the_three_predicates_answer_as_the_python_rules_did():
    def needs_workspace(C, n_tbins, n_rbins, dtype):  # ops.reduce_needs_workspace before the library answered
        esz = 8 if dtype == torch.float64 else 4
        lds = ((n_rbins * esz + 15) & ~15) + 4 * n_rbins
        return C * n_tbins < 1024 or lds > 128 * 1024

    for (C, n_tbins), n_rbins, dtype in itertools.product(
            ((1, 1023), (1, 1024), (3, 341), (2, 512), (4, 4000)),
            (1, 100, 10922, 10923, 16384, 16385, 40000), (torch.float32, torch.float64)):
        got = ops.reduce_needs_workspace(C, n_tbins, n_rbins, dtype)
        assert got is needs_workspace(C, n_tbins, n_rbins, dtype), (C, n_tbins, n_rbins, dtype)
    # the boundaries themselves: 128 KiB of accumulators at 10922 (f64) and 16384 (f32) range bins
    assert not ops.reduce_needs_workspace(2, 512, 10922, torch.float64) and ops.reduce_needs_workspace(2, 512, 10923, torch.float64)
    assert not ops.reduce_needs_workspace(2, 512, 16384, torch.float32) and ops.reduce_needs_workspace(2, 512, 16385, torch.float32)
    assert ops.reduce_needs_workspace(1, 1023, 8, torch.float64) and not ops.reduce_needs_workspace(1, 1024, 8, torch.float64)

    for n_rbins in (0, 1, 32767, 32768, 32769, 100000):
        assert ops.regrid_needs_global_flags(n_rbins) is (4 * n_rbins > 128 * 1024), n_rbins

    for addr, S, dtype in itertools.product((4096, 4096 + 8, 4096 + 4), (1, 2, 3, 4, 6, 1027, 1028),
                                            (torch.float32, torch.float64)):
        want = S % (2 if dtype == torch.float64 else 4) == 0 and addr % 16 == 0
        assert ops.sv_power_vectorized(_Ptr(addr), S, dtype) is want, (addr, S, dtype)


# ---- the plain constants of _lib against the header ------------------------------------------------------------------
def header_constants():
    """name without EPA_ -> value, of every ``#define EPA_X <integer>`` and every enumerator (implicit values counted up)."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, val in re.findall(r"^#define EPA_(\w+)[ \t]+(0x[0-9a-fA-F]+|\d+)u?[ \t]*$", txt, flags=re.M):
        out[name] = int(val, 0)
    order = {}
    for enum, body in re.findall(r"enum (\w+)\s*\{(.*?)\}", txt, flags=re.S):
        nxt, names = 0, []
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"EPA_(\w+)(?:\s*=\s*(0x[0-9a-fA-F]+|\d+))?", item)
            assert m, (enum, item)
            nxt = int(m.group(2), 0) if m.group(2) else nxt
            out[m.group(1)] = nxt
            names.append(m.group(1))
            nxt += 1
        order[enum] = names
    return out, order, txt


def test_lib_constants_equal_the_header():
    consts, order, txt = header_constants()
    compared = set()
    for name, val in consts.items():
        if hasattr(_lib, name):
            assert getattr(_lib, name) == val, name
            compared.add(name)
    # _lib names its status codes with the prefix kept
    for name in ("OK", "EINVAL", "EHIP", "ENOMEM", "EUNSUPPORTED"):
        assert getattr(_lib, "EPA_" + name) == consts[name]
        compared.add(name)
    annotated = {"I8", "QC_FACTS", "QC_MAX_WIN", "QC_MEDIAN_WAVES", "QC_SCAN_TILE", "RAW_ZERO_TIME", "NMEA_INVALID",
                 "NMEA_LAT_FAILED", "NMEA_LON_FAILED", "NMEA_UNDECIDED", "NMEA_TYPE_SHIFT", "NMEA_TYPE_MASK",
                 "SEAFLOOR_STATE_WORDS", "SHOAL_STATE_WORDS", "SHOAL_QUEUE_BOXES", "CMP_GT", "CMP_LT", "CMP_LE", "CMP_GE",
                 "CMP_EQ", "CT_I8", "CT_I16", "CT_I32", "CT_I64", "CT_F32", "CT_F64", "RAW_ANGLE_NONE", "RAW_ANGLE_I8",
                 "RAW_ANGLE_F32", "EK80_NFFT", "NCOEF", "NCCOEF", "F32", "F64", "QC_FIRST", "QC_COUNT", "QC_NAT",
                 "QC_SLOTS"}
    assert annotated <= compared, sorted(annotated - compared)
    assert not hasattr(_lib, "APPLY_MASKS_WS_DOUBLES")  # sized by the library now
    # CCP: the order of enum epa_ccoef_param (the enumerators end in a count, which is no parameter)
    ccp = [n[len("CCP_"):].lower() for n in order["epa_ccoef_param"] if n.startswith("CCP_")]
    ccp = [n for n in ccp if n not in ("count", "n")]
    assert tuple(ccp) == _lib.CCP
    # the two structs the binding fills by hand
    sizes = {"int64_t": 8, "uint64_t": 8, "int32_t": 4, "uint32_t": 4, "long long": 8}

    def struct_fields(name):
        body = re.search(r"typedef struct " + name + r"\s*\{([^}]*)\}\s*" + name + r"\s*;", txt).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"([\w ]+?\*?)\s*(\w+(?:\s*,\s*\w+)*)", decl)
            assert m and (m.group(1) in sizes or m.group(1).endswith("*")), decl
            fields += [(f.strip(), sizes.get(m.group(1), 8)) for f in m.group(2).split(",")]  # (a pointer: 8 bytes)
        return fields

    assert sum(sz for _, sz in struct_fields("epa_raw_record")) == _lib.RAW_RECORD_BYTES
    seg = struct_fields("epa_concat_seg")
    assert all(sz == 8 for _, sz in seg) and len(seg) == _lib.CONCAT_SEG_WORDS
