"""The EK60 .raw file of the ``open_raw`` benches (``bench_open_raw.py``, ``bench_nmea.py``), written with a few lines of
``struct`` and NumPy: ``CON0``, then per ping one mode-3 ``RAW0`` datagram per channel (int16 power and int8 angle pairs,
4 B per sample; sample values from a small random pool: the contents do not change what is moved) and one ``NME0`` sentence.
One builder for both benches, so that they measure the same file but for the text of its sentences."""
import struct

import numpy as np

NT0 = (1505260150 + 11644473600) * 10_000_000


def frame(body):
    return struct.pack("<l", len(body)) + body + struct.pack("<l", len(body))


def con0(C):
    body = struct.pack("<4sLL128s128s128s30s98sl", b"CON0", NT0 & 0xFFFFFFFF, NT0 >> 32, b"bench", b"", b"ER60", b"2.4.3", b"", C)
    for c in range(C):
        cid = f"GPT {18 + 20 * c:3d} kHz 00907203{c:04x} {c + 1}-1 ES{18 + 20 * c}".encode()
        tab = [0.000256, 0.000512, 0.001024, 0.002048, 0.004096]
        body += struct.pack("<128sl15f5f8s5f8s5f8s16s28s", cid, 1, 18000.0 + 20000.0 * c, 25.0, -20.0, 7.0, 7.0, 21.9, 21.9, 0.0,
                            0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, *tab, b"", *([25.0] * 5), b"", *([-0.5] * 5), b"", b"070413", b"")
    return frame(body)


def build_file(path, C, P, S, sentence, nme0_delay=5):
    """Write the file to ``path``: ``C`` channels x ``P`` pings x ``S`` samples; ``sentence(p)`` gives the bytes of the NME0 text
    behind ping p, stamped ``nme0_delay`` ticks of 100 ns behind the ping.  -> (the file's length, the sentences)."""
    rng = np.random.default_rng(20261019)
    pool = [np.concatenate([rng.integers(-12000, -2000, S).astype("<i2").view(np.uint8),
                            rng.integers(-128, 128, 2 * S).astype(np.int8).view(np.uint8)]) for _ in range(61)]
    nmea = [sentence(p) for p in range(P)]
    head = con0(C)
    dg = 8 + 84 + 4 * S
    total = len(head) + P * C * dg + sum(8 + 12 + len(s) for s in nmea)
    buf = np.empty(total, dtype=np.uint8)
    buf[:len(head)] = np.frombuffer(head, np.uint8)
    pos, n = len(head), 0
    for p in range(P):
        t = NT0 + p * 10_000_000
        for c in range(C):
            hdr = struct.pack("<l4sLLhh13fh6sll", 84 + 4 * S, b"RAW0", t & 0xFFFFFFFF, t >> 32, c + 1, 3, 9.15, 18000.0 + 20000.0 * c,
                              1000.0, 0.001024, 2425.0, 0.000256, 1480.0 + c, 0.003 * (c + 1), 0.0, 0.0, 0.0, 4.0, 0.0, 0, b"", 0, S)
            buf[pos:pos + 88] = np.frombuffer(hdr, np.uint8)
            buf[pos + 88:pos + 88 + 4 * S] = pool[n % len(pool)]
            buf[pos + 88 + 4 * S:pos + dg] = np.frombuffer(hdr[:4], np.uint8)
            pos += dg
            n += 1
        fr = frame(struct.pack("<4sLL", b"NME0", (t + nme0_delay) & 0xFFFFFFFF, (t + nme0_delay) >> 32) + nmea[p])
        buf[pos:pos + len(fr)] = np.frombuffer(fr, np.uint8)
        pos += len(fr)
    assert pos == total
    with open(path, "wb") as f:
        f.write(memoryview(buf))
    return total, nmea
