"""The EK80 .raw cases of the open_raw_ek80 tests (TEST INFRASTRUCTURE): every datagram of every case as a small dict from
a seeded generator, and the ``struct`` packers that turn them into file bytes.  The reference has no packer for RAW3,
XML0 or FIL1 datagrams (its ``_pack_contents`` covers version 0 only), so the bytes are packed HERE, by this project's
own code; scripts/gen_open_raw_ek80_goldens.py parses them back with the REFERENCE's parsers and stores what those give
in tests/golden/open_raw_ek80.npz, which the tests read through the helpers at the bottom.

Cases -- the smallest shapes at which the pieces can go wrong:
  fm       2 channels x 3 pings of LFM, 4 sectors, counts 65 / 64 / 63; FIL1 stages 1 and 2, MRU0, NME0 of odd lengths and
           XML0 texts whose lengths put the complex blocks at all four byte offsets mod 4; imaginary parts that are exactly
           0.0 and -0.0, and a NaN sample
  mixed    one channel alternating CW and LFM pings, a 3-sector channel beside a 4-sector one, a power / angle channel, a
           channel missing a ping, an EC150 channel, a RAW4, an environment datagram that carries only the drop-keel
           fields behind the real one: three beam groups
  long     1 channel x 2 pings of 1300 and 1299 samples, 4 sectors: lanes take several unrolled steps
  edges    three channels of 1, 3 and 4 sectors, one ping per count * B in {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257} that
           the sector count divides: unpacked channel by channel, S * B is odd for some rows
broken and cut variants are made from the bytes of ``fm`` by ``bad_variants`` / ``cut_variants``; ``synth_file`` writes
the arrays of ``synth.ek80_numpy`` into a file (the product tests)."""
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "open_raw_ek80.npz")
INDEX2POWER = np.float32(10.0 * np.log10(2.0) / 256.0)
# 2017-09-12 23:49:10 UTC in 100-ns ticks since 1601, plus 5 ticks: every time ends on half a microsecond
NT_BASE = (1505260150 + 11644473600) * 10_000_000 + 5
RAW3_HEADER, FIL1_HEADER, MRU0_SIZE = 152, 148, 28
PULSE_TABLE = (0.000256, 0.000512, 0.001024, 0.002048, 0.004096)


# ---- packers -----------------------------------------------------------------------------------------------------------
def _date(ticks):
    return int(ticks & 0xFFFFFFFF), int(ticks >> 32)


def frame(body):
    return struct.pack("<l", len(body)) + body + struct.pack("<l", len(body))


def _id128(text):
    return text.encode("latin_1").ljust(128, b"\x00")


def pack(d):
    """One datagram dict -> its body (no framing)."""
    k, head = d["kind"], struct.pack("<4sLL", d["kind"].encode(), *_date(d["ticks"]))
    if k in ("XML0", "NME0"):
        return head + d["text"].encode("ascii") + b"\x00" * d.get("nul", 0)
    if k in ("RAW3", "RAW4"):
        out = head + struct.pack("<128sh2sll", _id128(d["channel_id"]), d["data_type"], b"\x00\x00", d["offset"], d["count"])
        if d.get("power") is not None:
            out += np.asarray(d["power"], "<i2").tobytes()
        if d.get("angle") is not None:
            out += np.asarray(d["angle"], "<u2").tobytes()
        if d.get("complex") is not None:
            out += np.ascontiguousarray(d["complex"], dtype="<c8").tobytes()
        return out + b"\x00" * d.get("slack", 0)
    if k == "FIL1":
        c = np.ascontiguousarray(d["coefficients"], dtype="<c8")
        return head + struct.pack("<h2s128shh", d["stage"], b"\x00\x00", _id128(d["channel_id"]), c.size,
                                  d["decimation_factor"]) + c.tobytes()
    if k in ("MRU0",):
        return head + struct.pack("<4f", d["heave"], d["roll"], d["pitch"], d["heading"])
    if k == "MRU1":
        return head + b"\x00" * 132  # (144 bytes, ek_raw_parsers.py:556-588: all fields zero)
    raise ValueError(k)


def assemble(specs):
    """-> (file bytes as a uint8 array, int64 byte offsets of the bodies, int32 sizes)."""
    blobs = [frame(pack(d)) for d in specs]
    off = np.cumsum([0] + [len(b) for b in blobs[:-1]]).astype(np.int64) + 4
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), off, np.array([len(b) - 8 for b in blobs], np.int32)


# ---- XML texts ---------------------------------------------------------------------------------------------------------
def _attrs(d):
    return " ".join(f'{k}="{v}"' for k, v in d.items())


def _list(vals):
    return ";".join(repr(float(v)) for v in vals)


def channel_config(channel_id, number, freq, *, beam_type=1, gain=None, sa=None, psi=-20.7, bw=(7.0, 7.1), sens=(23.0, 23.0),
                   off=(0.0, 0.0), impedance=5400, fs=1500000, ttype="WBT", xdcr="ES70-7C", serial="123", cal=None,
                   version="2.60", pos=(0.0, 0.0, 0.0)):
    gain = gain if gain is not None else [25.0 + 0.25 * i for i in range(5)]
    sa = sa if sa is not None else [-0.1 * i for i in range(5)]
    return dict(channel_id=channel_id, number=number, freq=freq, beam_type=beam_type, gain=gain, sa=sa, psi=psi, bw=bw, sens=sens,
                off=off, impedance=impedance, fs=fs, ttype=ttype, xdcr=xdcr, serial=serial, cal=cal, version=version, pos=pos)


def config_xml(channels, transducers=True, app_version="2.0.1"):
    out = ['<?xml version="1.0" encoding="utf-8"?>', "<Configuration>",
           f'  <Header Copyright="none" ApplicationName="EK80" Version="{app_version}" FileFormatVersion="1.20" TimeBias="0" />',
           "  <Transceivers>"]
    for c in channels:
        t = _attrs({"TransceiverName": f"{c['ttype']} {c['serial']}", "IPAddress": f"157.237.15.{c['number']}",
                    "Version": "[0] Ethernet: 00:00:00:00:00:00", "TransceiverSoftwareVersion": c["version"],
                    "TransceiverNumber": c["number"], "MarketSegment": "Scientific", "TransceiverType": c["ttype"],
                    "SerialNumber": c["serial"], "Impedance": c["impedance"], "Multiplexing": 0, "RxSampleFrequency": c["fs"]})
        ch = _attrs({"ChannelID": c["channel_id"], "ChannelIdShort": c["xdcr"], "MaxTxPowerTransceiver": 2000,
                     "PulseDuration": _list(PULSE_TABLE), "PulseDurationFM": _list(2 * v for v in PULSE_TABLE),
                     "SampleInterval": _list([8e-06] * 5), "HWChannelConfiguration": 15})
        x = _attrs({"TransducerName": c["xdcr"], "SerialNumber": c["serial"], "Frequency": repr(float(c["freq"])),
                    "FrequencyMinimum": repr(float(0.6 * c["freq"])), "FrequencyMaximum": repr(float(1.4 * c["freq"])), "BeamType": c["beam_type"],
                    "EquivalentBeamAngle": repr(float(c["psi"])), "Gain": _list(c["gain"]), "SaCorrection": _list(c["sa"]),
                    "MaxTxPowerTransducer": "750", "BeamWidthAlongship": repr(float(c["bw"][0])),
                    "BeamWidthAthwartship": repr(float(c["bw"][1])), "AngleSensitivityAlongship": repr(float(c["sens"][0])),
                    "AngleSensitivityAthwartship": repr(float(c["sens"][1])), "AngleOffsetAlongship": repr(float(c["off"][0])),
                    "AngleOffsetAthwartship": repr(float(c["off"][1])), "DirectivityDropAt2XBeamWidth": "0"})
        out += [f"    <Transceiver {t}>", "      <Channels>", f"        <Channel {ch}>", f"          <Transducer {x}>"]
        for row in c["cal"] or ():
            f, g, z = row
            out.append("            <FrequencyPar " + _attrs({
                "Frequency": int(f), "Gain": repr(float(g)), "Impedance": repr(float(z)), "Phase": "0",
                "BeamWidthAlongship": repr(float(c["bw"][0] * c["freq"] / f)), "BeamWidthAthwartship": repr(float(c["bw"][1] * c["freq"] / f)),
                "AngleOffsetAlongship": repr(float(c["off"][0])), "AngleOffsetAthwartship": repr(float(c["off"][1]))}) + " />")
        out += ["          </Transducer>", "        </Channel>", "      </Channels>", "    </Transceiver>"]
    out.append("  </Transceivers>")
    if transducers:
        out.append('  <Transducers MergeOperation="AddNodeTree">')
        for c in channels:
            out.append("    <Transducer " + _attrs({
                "TransducerName": c["xdcr"], "TransducerSerialNumber": c["serial"], "TransducerCustomName": f"{c['xdcr']} {c['serial']}",
                "TransducerMounting": "HullMounted", "TransducerOrientation": "Vertical",
                "TransducerOffsetX": repr(float(c["pos"][0])), "TransducerOffsetY": repr(float(c["pos"][1])),
                "TransducerOffsetZ": repr(float(c["pos"][2])), "TransducerAlphaX": "0", "TransducerAlphaY": "0",
                "TransducerAlphaZ": "0"}) + " />")
        out.append("  </Transducers>")
    out.append("</Configuration>")
    return "\r\n".join(out)


def parameter_xml(channel_id, pulse_form, tau, si, power, slope, freq=None, band=None, mode=0):
    a = {"ChannelID": channel_id, "ChannelMode": mode, "PulseForm": pulse_form}
    if band is not None:
        a["FrequencyStart"], a["FrequencyEnd"] = repr(float(band[0])), repr(float(band[1]))
    else:
        a["Frequency"] = repr(float(freq))
    a.update({"PulseDuration": repr(float(tau)), "SampleInterval": repr(float(si)), "TransmitPower": repr(float(power)),
              "Slope": repr(float(slope)), "SoundVelocity": "1500.0"})
    return f'<?xml version="1.0" encoding="utf-8"?>\r\n<Parameter>\r\n  <Channel {_attrs(a)} />\r\n</Parameter>'


def environment_xml(sound_speed=1500.0, temperature=10.0, salinity=35.0, depth=10.0, acidity=8.0):
    a = {"Depth": repr(depth), "Acidity": repr(acidity), "Salinity": repr(salinity), "SoundSpeed": repr(float(sound_speed)),
         "Temperature": repr(temperature), "Latitude": "45.0", "SoundVelocityProfile": "1.0;1500.0;1000.0;1500.0",
         "SoundVelocitySource": "Manual", "DropKeelOffset": "0.0", "DropKeelOffsetIsManual": 0, "WaterLevelDraft": "0.5",
         "WaterLevelDraftIsManual": 0}
    return (f'<?xml version="1.0" encoding="utf-8"?>\r\n<Environment {_attrs(a)}>\r\n'
            '  <Transducer TransducerName="Unknown" SoundSpeed="1490.0" />\r\n</Environment>')


DROP_KEEL_XML = ('<?xml version="1.0" encoding="utf-8"?>\r\n<Environment DropKeelOffset="1.5" DropKeelOffsetIsManual="1" />')
PING_SEQUENCE_XML = '<?xml version="1.0" encoding="utf-8"?>\r\n<PingSequence>\r\n  <Ping ChannelID="all" />\r\n</PingSequence>'


def xml0(ticks, text, nul=0):
    return {"kind": "XML0", "ticks": ticks, "text": text, "nul": nul}


def nme0(ticks, text):
    return {"kind": "NME0", "ticks": ticks, "text": text}


def mru0(rng, ticks):
    f = lambda: float(np.float32(rng.normal()))  # noqa: E731
    return {"kind": "MRU0", "ticks": ticks, "heave": f(), "roll": f(), "pitch": f(), "heading": float(np.float32(rng.uniform(0, 360)))}


def fil1(ticks, stage, channel_id, n, deci, seed):
    r = np.random.default_rng(seed)
    c = ((r.integers(-512, 512, n) + 1j * r.integers(-512, 512, n)) / 4096).astype(np.complex64)
    return {"kind": "FIL1", "ticks": ticks, "stage": stage, "channel_id": channel_id, "coefficients": c, "decimation_factor": deci}


def samples(rng, count, B):
    """(count, B) complex64 of few distinct values (the fixture compresses) with no imaginary part equal to 0."""
    re = rng.integers(-2000, 2000, (count, B)) / 64
    im = rng.integers(1, 2000, (count, B)) / 64 * rng.choice([-1.0, 1.0], (count, B))
    return (re + 1j * im).astype(np.complex64)


def raw3(ticks, channel_id, count, B=0, cplx=None, power=None, angle=None, offset=0, kind="RAW3", data_type=None, slack=0):
    dt = data_type if data_type is not None else ((B << 8) | 8 if B else 0) | (1 if power is not None else 0) | (2 if angle is not None else 0)
    return {"kind": kind, "ticks": ticks, "channel_id": channel_id, "data_type": dt, "offset": offset, "count": count,
            "complex": cplx, "power": power, "angle": angle, "slack": slack}


def _ping_ticks(p):
    return NT_BASE + p * 10_000_123


NMEA = ("$GPGGA,234910.00,4704.1234,N,12503.4321,W,1,08,0.9,12.3,M,-20.1,M,,*4", "$GPGLL,4704.12,N,12503.43,W,234911,A*2",
        "$GPZDA,234912.71,12,09,2017,-1,00*7D", "$INVTG,254.1,T,,M,9.7,N,18.0,K*50", "$GPGLL,4704.20,N,12503.50,W,234913,A")
CH70, CH120 = "WBT 400040-15 ES70-7C", "WBT 400041-15 ES120-7C"


def fm():
    rng = np.random.default_rng(80)
    chans = [channel_config(CH120, 2, 120000.0, xdcr="ES120-7C", serial="456", off=(0.05, -0.03), pos=(1.0, 2.0, 3.0),
                            cal=[(90000, 25.0, 75.0), (120000, 26.0, 76.0), (170000, 25.5, 74.0)]),
             channel_config(CH70, 1, 70000.0, off=(-0.02, 0.04), pos=(0.5, -0.5, 4.0))]  # (not in sorted order)
    out = [xml0(NT_BASE - 10_000_000, config_xml(chans)), xml0(NT_BASE - 9_000_000, environment_xml(1486.4))]
    for i, (cid, st, n, deci) in enumerate(((CH70, 1, 47, 6), (CH70, 2, 91, 2), (CH120, 1, 31, 8), (CH120, 2, 63, 1))):
        out.append(fil1(NT_BASE - 8_000_000, st, cid, n, deci, 800 + i))
    par = {CH70: dict(pulse_form=1, tau=0.001024, si=8e-06, power=750.0, slope=0.05, band=(45000.0, 90000.0)),
           CH120: dict(pulse_form=1, tau=0.000512, si=1.6e-05, power=250.0, slope=0.025, band=(90000.0, 170000.0))}
    n = 0
    for p, count in enumerate((65, 64, 63)):
        out.append(mru0(rng, _ping_ticks(p) - 500))
        for cid in (CH70, CH120):
            out.append(xml0(_ping_ticks(p), parameter_xml(cid, **par[cid]), nul=(n * 3) % 4))
            x = samples(rng, count, 4)
            if n == 0:
                x[3, 1] = np.complex64(complex(1.5, 0.0))
                x[4, 2] = np.complex64(complex(-2.25, -0.0))
                x[5, 0] = np.complex64(complex(np.nan, np.nan))
                x[6, 3] = np.complex64(complex(0.0, 3.0))
            out.append(raw3(_ping_ticks(p), cid, count, 4, x, offset=p))
            out.append(nme0(_ping_ticks(p) + 1000 * (n + 1), NMEA[n % len(NMEA)]))
            n += 1
    return out


CH38, CH200, CH333, CHEC = "WBT 400042-15 ES38-7", "WBT 400043-15 ES200-7C", "WBT 400044-15 ES333-7C", "EC150-3C 400050-1 EC150"


def mixed():
    rng = np.random.default_rng(81)
    chans = [channel_config(CH70, 1, 70000.0), channel_config(CH38, 3, 38000.0, xdcr="ES38-7", serial="789", beam_type=17),
             channel_config(CH200, 4, 200000.0, xdcr="ES200-7C", serial="321", ttype="GPT"),
             channel_config(CH333, 5, 333000.0, xdcr="ES333-7C", serial="654"),
             channel_config(CHEC, 6, 150000.0, xdcr="EC150", serial="999")]
    out = [xml0(NT_BASE - 10_000_000, config_xml(chans)), xml0(NT_BASE - 9_000_000, environment_xml(1492.25)),
           xml0(NT_BASE - 8_500_000, DROP_KEEL_XML)]
    for i, cid in enumerate((CH70, CH38, CH333, CHEC)):
        out.append(fil1(NT_BASE - 8_000_000, 1, cid, 15 + i, 4, 810 + i))  # (one filter_time: several, none of them a ping
        out.append(fil1(NT_BASE - 8_000_000, 2, cid, 21 + i, 2, 820 + i))  # time, leave every ping without a filter interval)
    cw = dict(pulse_form=0, tau=0.001024, si=6.4e-05, power=500.0, slope=0.5)
    for p in range(4):
        t = _ping_ticks(p)
        out.append(xml0(t - 100, PING_SEQUENCE_XML))
        out.append(mru0(rng, t - 50))
        # CH70: CW on even pings, LFM on odd ones, 4 sectors
        if p % 2:
            out.append(xml0(t, parameter_xml(CH70, 1, 0.002048, 8e-06, 750.0, 0.05, band=(45000.0, 90000.0)), nul=p))
        else:
            out.append(xml0(t, parameter_xml(CH70, freq=70000.0, **cw), nul=p))
        if p == 1:
            out.append(raw3(t, CH70, 7, 4, samples(rng, 7, 4), kind="RAW4"))
        out.append(raw3(t, CH70, 40 + p, 4, samples(rng, 40 + p, 4)))
        # CH38: CW, 3 sectors; lacks ping 2
        if p != 2:
            out.append(xml0(t, parameter_xml(CH38, freq=38000.0, **cw)))
            out.append(raw3(t, CH38, 33 - p, 3, samples(rng, 33 - p, 3), offset=1))
        # CH200: power and angle; CH333: power only
        out.append(xml0(t, parameter_xml(CH200, freq=200000.0, **cw), nul=1))
        cnt = 50 - 3 * p
        athw, along = rng.integers(-128, 128, cnt), rng.integers(-128, 128, cnt)
        out.append(raw3(t, CH200, cnt, power=rng.integers(-12000, -2000, cnt).astype(np.int16),
                        angle=((athw & 0xFF) | ((along & 0xFF) << 8)).astype(np.uint16)))
        out.append(xml0(t, parameter_xml(CH333, freq=333000.0, **cw)))
        out.append(raw3(t, CH333, 20 + p, power=rng.integers(-12000, -2000, 20 + p).astype(np.int16)))
        out.append(nme0(t + 777, NMEA[p % len(NMEA)]))
        # the ADCP channel: its parameter and samples are dropped everywhere
        out.append(xml0(t + 10, parameter_xml(CHEC, freq=150000.0, **cw)))
        out.append(raw3(t + 10, CHEC, 9, 4, samples(rng, 9, 4)))
    out.append({"kind": "MRU1", "ticks": _ping_ticks(4)})
    return out


def long():
    rng = np.random.default_rng(82)
    par = parameter_xml(CH70, 1, 0.001024, 8e-06, 750.0, 0.05, band=(45000.0, 90000.0))
    out = [xml0(NT_BASE - 10_000_000, config_xml([channel_config(CH70, 1, 70000.0)])),
           xml0(NT_BASE - 9_000_000, environment_xml())]
    for p, count in enumerate((1300, 1299)):
        out += [xml0(_ping_ticks(p), par), raw3(_ping_ticks(p), CH70, count, 4, samples(rng, count, 4)),
                nme0(_ping_ticks(p) + 9, "$GPGLL,1*2")]
    return out


EDGE_SIZES = (1, 3, 4, 5, 63, 64, 65, 0, 255, 256, 257)  # count * B; the empty ping is not a channel's first
EDGE_CHANNELS = (("WBT 400061-15 ES18", 1), ("WBT 400063-15 ES38-18", 3), ("WBT 400064-15 ES70-7C", 4))


def edges():
    rng = np.random.default_rng(83)
    chans = [channel_config(cid, i + 1, 18000.0 * (i + 1), serial=str(100 + i)) for i, (cid, _) in enumerate(EDGE_CHANNELS)]
    out = [xml0(NT_BASE - 10_000_000, config_xml(chans)), xml0(NT_BASE - 9_000_000, environment_xml())]
    n = 0
    for p, size in enumerate(EDGE_SIZES):
        for cid, B in EDGE_CHANNELS:
            if size % B:
                continue
            out.append(xml0(_ping_ticks(p), parameter_xml(cid, 0, 0.000512, 8e-06, 100.0, 0.5, freq=18000.0), nul=n % 3))
            out.append(raw3(_ping_ticks(p), cid, size // B, B, samples(rng, size // B, B)))
            n += 1
    return out


CASES = {"fm": fm, "mixed": mixed, "long": long, "edges": edges}
_cache = {}


def built(case):
    """-> (file bytes, body offsets, sizes, the datagram dicts) of a case, as packed here."""
    if ("b", case) not in _cache:
        specs = CASES[case]()
        _cache["b", case] = assemble(specs) + (specs,)
    return _cache["b", case]


def file_bytes(case):
    return built(case)[0]


def block_offsets(case):
    """[(index of the datagram, byte offset of its power / angle / complex block or -1 each)] of the RAW3 datagrams."""
    _, off, _, specs = built(case)
    out = []
    for i, d in enumerate(specs):
        if d["kind"] != "RAW3":
            continue
        b = int(off[i]) + RAW3_HEADER
        p = b if d["power"] is not None else -1
        b += 2 * d["count"] * (d["power"] is not None)
        a = b if d["angle"] is not None else -1
        b += 2 * d["count"] * (d["angle"] is not None)
        out.append((i, p, a, b if d["complex"] is not None else -1))
    return out


# ---- variants of ``fm`` --------------------------------------------------------------------------------------------------
def _rebuild(mutate):
    specs = fm()
    mutate(specs)
    data, off, size = assemble(specs)
    return data, off, size, specs


def bad_variants():
    """{name: (bytes, exception type, text the message must hold)}."""
    out = {}

    def first_raw3(specs):
        return next(i for i, d in enumerate(specs) if d["kind"] == "RAW3")

    def leaves(specs):
        d = specs[first_raw3(specs)]
        d["count"] += 1  # one sample more than the datagram holds

    data, off, _, specs = _rebuild(leaves)
    out["block_leaves"] = (data, ValueError, f"byte offset {int(off[first_raw3(specs)])}")

    def mismatch(specs):
        specs[first_raw3(specs)]["channel_id"] = CH120

    out["id_mismatch"] = (_rebuild(mismatch)[0], ValueError, "Parameter ID does not match RAW")

    def half(specs):
        d = specs[first_raw3(specs)]
        d["data_type"] = (4 << 8) | 4
        d["complex"], d["slack"] = None, 4 * d["count"] * 4  # (the bytes count float16 pairs of 4 sectors take, all zero)

    data, off, _, specs = _rebuild(half)
    out["float16"] = (data, NotImplementedError, f"byte offset {int(off[first_raw3(specs)])}")
    data, off, _, specs = _rebuild(lambda s: s.pop(0))
    out["no_configuration"] = (data, ValueError, "Configuration")

    def orphan(specs):
        i = first_raw3(specs)
        specs[1:1] = [dict(specs[i])]  # a RAW3 in front of every parameter datagram

    data, off, _, specs = _rebuild(orphan)
    out["no_parameter"] = (data, ValueError, f"byte offset {int(off[1])}")
    return out


def cut_variants():
    """``fm`` cut inside its last RAW3 -> {name: (bytes, number of complete datagrams in front)}."""
    data, off, size, specs = built("fm")
    last = max(i for i, d in enumerate(specs) if d["kind"] == "RAW3")
    return {"in_last_raw3": (data[:int(off[last]) + 200], last), "in_its_trailer": (data[:int(off[last]) + int(size[last]) + 2], last)}


# ---- the product: the arrays of synth.ek80_numpy as a file ------------------------------------------------------------------
def synth_file(d, filters, waveform):
    """The dictionary of ``synth.ek80_numpy`` (samples already float32, ``tau`` already ``float64(float32(tau))``) and the
    filters of ``synth.ek80_filters`` -> file bytes whose ``open_raw_ek80`` holds the values ``from_ek80_arrays`` builds
    from the same dictionary: every parameter is written with ``repr``."""
    C, P, S, B = d["backscatter_r"].shape
    bb = waveform == "BB"
    chans = []
    for c in range(C):
        g = float(d["gain"][c])
        chans.append(channel_config(d["channel"][c], c + 1, d["frequency_nominal"][c], gain=[g - 1, g - .5, g, g + .2, g + .3],
                                    sa=[d["sa"][c]] * 5, psi=d["psi"][c], bw=(d["beamwidth_alongship"][c], d["beamwidth_athwartship"][c]),
                                    off=(d["angle_offset_alongship"][c], d["angle_offset_athwartship"][c]),
                                    impedance=int(d["z_er"][c]), fs=int(d["fs"][c]), serial=str(500 + c),
                                    beam_type=int(np.asarray(d.get("beam_type", np.ones(C)))[c]), sens=(23.0, 23.0)))
    t0 = int(np.asarray(d["ping_time"][0]).astype("datetime64[ns]").astype(np.int64)) // 100 + 11644473600 * 10_000_000
    out = [xml0(t0 - 10_000_000, config_xml(chans, transducers=False)),
           xml0(t0 - 9_000_000, environment_xml(float(np.asarray(d["sound_speed"]).flat[0])))]
    for c in range(C):
        for stage, key, dk in ((1, "wbt_fil", "wbt_decifac"), (2, "pc_fil", "pc_decifac")):
            out.append({"kind": "FIL1", "ticks": t0 - 8_000_000, "stage": stage, "channel_id": d["channel"][c],
                        "coefficients": filters[key], "decimation_factor": int(filters[dk])})
    x = (d["backscatter_r"] + 1j * d["backscatter_i"]).astype(np.complex64)
    ticks = np.asarray(d["ping_time"]).astype("datetime64[ns]").astype(np.int64) // 100 + 11644473600 * 10_000_000
    for p in range(P):
        for c in range(C):
            kw = dict(band=(d["f_start"][c], d["f_stop"][c])) if bb else dict(freq=d["frequency_nominal"][c])
            out.append(xml0(int(ticks[p]), parameter_xml(d["channel"][c], 1 if bb else 0, d["tau"][c], d["sample_interval"][c, p],
                                                         d["transmit_power"][c], d["slope"][c], **kw), nul=(p + c) % 3))
            out.append(raw3(int(ticks[p]), d["channel"][c], S, B, x[c, p]))
    return assemble(out)[0]


# ---- reading the fixture ---------------------------------------------------------------------------------------------
def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def golden_json(case, name):
    return json.loads(str(golden()[f"{case}/{name}_json"]))


def ref_channels(case):
    """The channel ids the reference kept (EC150 dropped), in the order of their first RAW3."""
    return [str(c) for c in golden()[f"{case}/channels"]]


def ref_channel(case, cid):
    """What the reference's ``ParseEK`` holds for one channel after ``_parse_and_pad_datagram``: dict with ``ping_time``,
    ``params`` (one dict per ping) and, where the channel has them, ``real`` / ``imag`` (P, S, B) float32 with NaN,
    ``power`` (P, S) float64 and ``angle`` (P, S, 2) float32 with NaN."""
    g, k = golden(), ref_channels(case).index(cid)
    out = {"ping_time": g[f"{case}/ch{k}/ping_time"], "params": json.loads(str(g[f"{case}/ch{k}/params_json"]))}
    for name in ("real", "imag", "power", "angle"):
        if f"{case}/ch{k}/{name}" in g:
            out[name] = g[f"{case}/ch{k}/{name}"]
    return out


GROUP_ORDER = ("complex_FM", "complex_CW", "power")


def expected_groups(case):
    """The beam groups open_raw_ek80 must give, assembled from the REFERENCE-parsed per-channel data of the fixture by the
    rules of set_groups_ek80.py:1124-1232 -> {descr: dict(channel, ping_time, C, P, S, B, real, imag | power, athw, along,
    params)}; ``params`` maps a field to a (C, P) object array (None where a channel lacks the ping)."""
    if ("x", case) in _cache:
        return _cache["x", case]
    chans = {cid: ref_channel(case, cid) for cid in ref_channels(case)}
    out = {}
    for descr in GROUP_ORDER:
        rows = {}
        for cid in sorted(chans):
            ch = chans[cid]
            form = np.array([p.get("pulse_form", -1) for p in ch["params"]])
            if descr == "power":
                keep = np.ones(form.size, bool) if "power" in ch else np.zeros(form.size, bool)
            else:
                keep = (form == (1 if descr == "complex_FM" else 0)) if "real" in ch else np.zeros(form.size, bool)
            if keep.any():
                rows[cid] = np.flatnonzero(keep)
        if not rows:
            continue
        ids = sorted(rows)
        pt = np.unique(np.concatenate([chans[c]["ping_time"][rows[c]] for c in ids]))
        C, P = len(ids), pt.size
        e = {"channel": ids, "ping_time": pt, "C": C, "P": P, "params": {}}
        fields = sorted({k for c in ids for p in chans[c]["params"] for k in p})
        for f in fields:
            e["params"][f] = np.full((C, P), None, dtype=object)
        if descr == "power":
            counts = [int(chans[c]["params"][i]["count"]) for c in ids for i in rows[c]]
            S = e["S"] = max(1, max(counts))
            e["power"] = np.full((C, P, S), np.nan, np.float32)
            e["athw"], e["along"] = np.full((C, P, S), np.nan, np.float32), np.full((C, P, S), np.nan, np.float32)
            e["has_angle"] = [("angle" in chans[c]) for c in ids]
        else:
            counts = [int(chans[c]["params"][i]["count"]) for c in ids for i in rows[c]]
            S, B = max(1, max(counts)), max(chans[c]["real"].shape[2] for c in ids)
            e["S"], e["B"] = S, B
            e["real"], e["imag"] = np.full((C, P, S, B), np.nan, np.float32), np.full((C, P, S, B), np.nan, np.float32)
        for ci, c in enumerate(ids):
            ch, idx = chans[c], rows[c]
            pi = np.searchsorted(pt, ch["ping_time"][idx])
            for f in fields:
                e["params"][f][ci, pi] = [ch["params"][i].get(f) for i in idx]
            if descr == "power":
                n = min(S, ch["power"].shape[1])
                idx16 = np.rint(ch["power"][idx, :n] / (10.0 * np.log10(2.0) / 256.0))  # back to the int16 the datagram holds
                e["power"][ci, pi, :n] = idx16.astype(np.float32) * INDEX2POWER
                if "angle" in ch:
                    e["athw"][ci, pi, :n] = ch["angle"][idx, :n, 0]
                    e["along"][ci, pi, :n] = ch["angle"][idx, :n, 1]
            else:
                n, b = min(S, ch["real"].shape[1]), ch["real"].shape[2]
                e["real"][ci, pi, :n, :b] = ch["real"][idx, :n]
                e["imag"][ci, pi, :n, :b] = ch["imag"][idx, :n]
        out[descr] = e
    _cache["x", case] = out
    return out
