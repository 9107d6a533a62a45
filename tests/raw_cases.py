"""The EK60 .raw cases of the open_raw tests (TEST INFRASTRUCTURE, data only): the field values of every datagram of every
case, from a seeded generator.  scripts/gen_open_raw_goldens.py packs them into file bytes with the REFERENCE's own
datagram packers, parses the bytes back with the reference's parsers and stores both in tests/golden/open_raw_ek60.npz;
the tests read that file through the helpers at the bottom.

Cases -- the smallest shapes at which the pieces can go wrong:
  aligned  2 channels x 4 pings x 64 samples, mode 3, nothing else: int8 angles, no padding
  ragged   3 channels x 8 ping times, counts from {0, 1, 2, 63, 64, 65, 129, 257}; NME0 sentences of every length mod 4 in
           between, so the sample blocks start at every byte offset mod 4; one channel lacks one ping time (outer join);
           one channel is mode 1 throughout; one datagram has the time stamp (0, 0); one is of a type nobody reads (TAG0);
           the channel ids are not in sorted order in CON0
  long     1 channel x 2 pings of 5000 and 4999 samples: a row takes several steps of a wavefront
  mode2    aligned with one ping of mode 2 (angle only)          -> NotImplementedError
  nocon    a file whose first datagram is RAW0                   -> ValueError
cut / bad variants of ``aligned`` are made from its bytes by ``cut_variants`` / ``bad_variants``."""
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "open_raw_ek60.npz")
SIGNATURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "open_raw_signature.json")
INDEX2POWER = np.float32(10.0 * np.log10(2.0) / 256.0)
SENTINEL = np.int16(-32768)  # a NaN of the reference's padded arrays in the int16 coding of the fixture
RAW0_FLOATS = ("transducer_depth", "frequency", "transmit_power", "pulse_length", "bandwidth", "sample_interval",
               "sound_velocity", "absorption_coefficient", "heave", "roll", "pitch", "temperature", "heading")
RAW0_INTS = ("channel", "mode", "transmit_mode", "offset", "count", "low_date", "high_date")
# 2017-09-12 23:49:10 UTC in 100-ns ticks since 1601, plus 5 ticks: every time ends on half a microsecond
NT_BASE = (1505260150 + 11644473600) * 10_000_000 + 5
FREQ = {1: 120000.0, 2: 18000.0, 3: 38000.0}
CHANNEL_ID = {1: "GPT 120 kHz 00907205794e 1-1 ES120-7C", 2: "GPT  18 kHz 009072034d45 2-1 ES18-11",
              3: "GPT  38 kHz 009072033fa2 3-1 ES38B"}  # sorted by id: 2, 3, 1


def _date(ticks):
    return {"low_date": int(ticks & 0xFFFFFFFF), "high_date": int(ticks >> 32)}


def _f32(x):
    return float(np.float32(x))


def raw0(rng, channel, ticks, mode, count):
    d = {"kind": "RAW0", "type": b"RAW0", **_date(ticks), "channel": channel, "mode": mode,
         "transducer_depth": _f32(9.15), "frequency": FREQ[channel], "transmit_power": _f32(1000.0 * channel),
         "pulse_length": _f32(0.001024), "bandwidth": _f32(1573.66552734375 + channel),
         "sample_interval": _f32(0.000256), "sound_velocity": _f32(1466.0 + rng.integers(0, 40) / 8),
         "absorption_coefficient": _f32(0.003 * channel + rng.integers(0, 100) * 1e-6),
         "heave": _f32(rng.normal()), "roll": _f32(rng.normal()), "pitch": _f32(rng.normal()),
         "temperature": _f32(4.0), "heading": _f32(rng.uniform(0, 360)), "transmit_mode": 0, "spare0": b"\x00" * 6,
         "offset": int(rng.integers(0, 3)), "count": count}
    if mode & 1:
        d["power"] = rng.integers(-12000, -2000, count).astype(np.int16)
    if mode & 2:  # one uint16 per sample: athwartship in the low byte, alongship in the high one
        athw, along = rng.integers(-128, 128, count), rng.integers(-128, 128, count)
        d["angle"] = ((athw & 0xFF) | ((along & 0xFF) << 8)).astype(np.uint16)
    return d


def nme0(ticks, text):
    return {"kind": "NME0", "type": b"NME0", **_date(ticks), "text": text}


def tag0(ticks, text):
    return {"kind": "TAG0", "type": b"TAG0", **_date(ticks), "text": text}


def con0(rng, channels):
    def s(txt, n):
        return txt.encode("latin_1").ljust(n, b"\x00")

    tx = {}
    for k in channels:
        tx[k] = {"channel_id": s(CHANNEL_ID[k], 128), "beam_type": 1, "frequency": FREQ[k], "gain": _f32(20.0 + k),
                 "equivalent_beam_angle": _f32(-17.0 - k), "beamwidth_alongship": _f32(7.0 + k / 8),
                 "beamwidth_athwartship": _f32(7.0 - k / 8), "angle_sensitivity_alongship": _f32(21.9 + k),
                 "angle_sensitivity_athwartship": _f32(22.1 + k), "angle_offset_alongship": _f32(0.05 * k),
                 "angle_offset_athwartship": _f32(-0.03 * k), "pos_x": _f32(k), "pos_y": _f32(-k), "pos_z": _f32(0.5 * k),
                 "dir_x": 0.0, "dir_y": 0.0, "dir_z": _f32(1.0) if k == 1 else 0.0,
                 "pulse_length_table": [_f32(v) for v in (0.000256, 0.000512, 0.001024, 0.002048, 0.004096)],
                 "spare1": s("", 8),
                 "gain_table": [_f32(20.0 + k + 0.1234567 * i) for i in range(5)], "spare2": s("", 8),
                 "sa_correction_table": [_f32(-0.5 + 0.0123456789 * i * k) for i in range(5)], "spare3": s("", 8),
                 "gpt_software_version": s("070413", 16), "spare4": s("", 28)}
    return {"kind": "CON0", "type": b"CON0", **_date(NT_BASE - 10_000_000), "survey_name": s("open_raw test survey", 128),
            "transect_name": s("T1", 128), "sounder_name": s("ER60", 128), "version": s("2.4.3", 30), "spare0": s("", 98),
            "transceiver_count": len(tx), "transceivers": tx}


def _ping_ticks(p):
    return NT_BASE + p * 10_000_123


def aligned(rng=None, bad_mode=None):
    rng = rng or np.random.default_rng(60)
    out = [con0(rng, (1, 2))]
    for p in range(4):
        for k in (1, 2):
            out.append(raw0(rng, k, _ping_ticks(p), 2 if bad_mode == (p, k) else 3, 64))
    return out


RAGGED_COUNTS = (0, 1, 2, 63, 64, 65, 129, 257)
NMEA = ("$GPGGA,234910.00,4704.1234,N,12503.4321,W,1,08,0.9,12.3,M,-20.1,M,,*4", "$GPGLL,4704.12,N,12503.43,W,234911,A*2",
        "$GPZDA,234912.71,12,09,2017,-1,00*7D", "$INVTG,254.1,T,,M,9.7,N,18.0,K*50", "$GPXX")  # lengths 1, 3, 0, 2, 1 mod 4


def ragged():
    rng = np.random.default_rng(61)
    out = [con0(rng, (1, 2, 3))]
    n = 0
    for p in range(8):
        for k in (1, 2, 3):
            if (k, p) == (1, 5):  # channel 1 lacks ping time 5
                continue
            out.append(raw0(rng, k, _ping_ticks(p), 1 if k == 3 else 3, RAGGED_COUNTS[(p + 3 * k) % 8]))
            out.append(nme0(_ping_ticks(p) + 1000 * k, NMEA[n % len(NMEA)]))
            n += 1
        if p == 2:
            out.append(raw0(rng, 2, 0, 3, 64))  # time stamp (0, 0): skipped
            out.append(tag0(_ping_ticks(p) + 7, "a note nobody reads"))
    return out


def long():
    rng = np.random.default_rng(62)
    return [con0(rng, (1,)), raw0(rng, 1, _ping_ticks(0), 3, 5000), nme0(_ping_ticks(0) + 9, "$GPGLL,1*2"),
            raw0(rng, 1, _ping_ticks(1), 3, 4999)]


def mode2():
    return aligned(bad_mode=(2, 1))


def nocon():
    return aligned()[1:]


CASES = {"aligned": aligned, "ragged": ragged, "long": long, "mode2": mode2, "nocon": nocon}
GOOD = ("aligned", "ragged", "long")


# ---- reading the fixture ---------------------------------------------------------------------------------------------
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def file_bytes(case):
    return golden()[f"{case}/bytes"]


def config(case):
    return json.loads(str(golden()[f"{case}/con0_json"]))


def channels_with_data(case):
    return [int(k) for k in golden()[f"{case}/channels"]]


def decode(a):
    """int16 coding of a padded array of the reference -> float32 with NaN."""
    out = a.astype(np.float32)
    out[a == SENTINEL] = np.nan
    return out


def expected(case):
    """The volumes and per-ping variables open_raw must give, assembled from the REFERENCE-parsed per-channel data of the
    fixture by the rules of set_groups_ek60.py: channels sorted by id string (those with power), ping_time the sorted union
    of the channels' times, a channel's angles only when all its pings record them.  -> dict; ``power`` is the float32
    product, ``athw`` / ``along`` float32 with NaN (None without angles), ``angles_int8`` whether nothing is padded."""
    if ("x", case) in _cache:
        return _cache["x", case]
    g, cfg = golden(), config(case)
    ks = sorted(channels_with_data(case), key=lambda k: cfg["transceivers"][str(k)]["channel_id"])
    ks = [k for k in ks if np.any(g[f"{case}/ch{k}/power"] != SENTINEL)]
    times = [g[f"{case}/ch{k}/ping_time"] for k in ks]
    pt = np.unique(np.concatenate(times))
    S = max(g[f"{case}/ch{k}/power"].shape[1] for k in ks)
    C, P = len(ks), pt.size
    e = {"transceivers": ks, "channel": [cfg["transceivers"][str(k)]["channel_id"] for k in ks], "ping_time": pt,
         "C": C, "P": P, "S": S, "power": np.full((C, P, S), np.nan, np.float32)}
    athw, along = np.full((C, P, S), np.nan, np.float32), np.full((C, P, S), np.nan, np.float32)
    hdr = {f: np.full((C, P), np.nan) for f in RAW0_FLOATS + ("mode", "transmit_mode", "offset", "count")}
    any_angle = False
    for c, k in enumerate(ks):
        p = np.searchsorted(pt, times[c])
        pw = decode(g[f"{case}/ch{k}/power"])
        e["power"][c, p, :pw.shape[1]] = pw * INDEX2POWER
        mode = g[f"{case}/ch{k}/hdr_mode"]
        if np.all(mode != 1):
            any_angle = True
            an = decode(g[f"{case}/ch{k}/angle"])
            athw[c, p, :an.shape[1]] = an[:, :, 0]
            along[c, p, :an.shape[1]] = an[:, :, 1]
        for f in hdr:
            hdr[f][c, p] = g[f"{case}/ch{k}/hdr_{f}"]
    e["athw"], e["along"] = (athw, along) if any_angle else (None, None)
    e["angles_int8"] = any_angle and not np.isnan(athw).any()
    e["hdr"] = hdr
    _cache["x", case] = e
    return e


def frames(case):
    """(offsets of the bodies, sizes) of the datagrams of a good case, as the generator laid them down."""
    g = golden()
    return g[f"{case}/rec_offset"], g[f"{case}/rec_size"]


def cut_variants():
    """``aligned`` truncated at four places -> {name: (bytes, number of complete datagrams in front)}."""
    b = file_bytes("aligned")
    off, size = frames("aligned")
    n, last = len(off), int(off[-1])
    return {"in_last_body": (b[:last + 40], n - 1), "in_last_trailer": (b[:len(b) - 2], n - 1),
            "in_a_header": (b[:last + 6], n - 1), "after_con0": (b[:int(off[0]) + int(size[0]) + 4], 1)}


def bad_variants():
    """``aligned`` with a broken frame -> {name: (bytes, byte offset the error names, complete datagrams in front)}."""
    b = file_bytes("aligned")
    off, size = frames("aligned")
    k = 3
    t = b.copy()
    t[int(off[k]) + int(size[k])] ^= 0x10  # the trailing size of datagram k
    s8 = b.copy()
    s8[int(off[k]) - 4:int(off[k])] = np.frombuffer(struct.pack("<l", 8), np.uint8)
    return {"trailer": (t, int(off[k]) - 4, k), "size8": (s8, int(off[k]) - 4, k)}
