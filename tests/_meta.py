"""<prefix>.meta of `mbgc-hip c` (mbgc_amd/host/mbgc_decoder.cpp) read and written in Python, for the tests."""
import struct

FLAGS = ("sequential", "rc_in_reference", "contigs_individually_reversed", "uppercase", "single_fasta", "rc_redundancy_removal")
EMIT = 15


def parse(b):
    assert b[:8] == b"MBGCHIPM"
    version, flags, mode, k, k1, g0 = struct.unpack_from("<6I", b, 8)
    max_ref, sw, final, laps = struct.unpack_from("<4Q", b, 32)
    emit = struct.unpack_from("<%dq" % EMIT, b, 64)
    at = 64 + 8 * EMIT
    n, indexed = struct.unpack_from("<2I", b, at)
    at += 8
    targets = [struct.unpack_from("<IBBH", b, at + 8 * t)[:3] for t in range(n)]
    at += 8 * n
    index = []
    if indexed:
        index = [list(struct.unpack_from("<6Q", b, at + 48 * t)) for t in range(n + 1)]
        at += 48 * (n + 1)
    assert at == len(b)
    m = dict(version=version, mode=mode, k=k, k1=k1, g0_contigs=g0, max_ref_length=max_ref, sw_size=sw, final_ref_length=final, laps=laps,
             emit=list(emit), targets=targets, index=index)
    for i, f in enumerate(FLAGS):
        m[f] = bool(flags >> i & 1)
    return m


def build(m):
    flags = sum(1 << i for i, f in enumerate(FLAGS) if m[f])
    b = b"MBGCHIPM" + struct.pack("<6I", m["version"], flags, m["mode"], m["k"], m["k1"], m["g0_contigs"])
    b += struct.pack("<4Q", m["max_ref_length"], m["sw_size"], m["final_ref_length"], m["laps"])
    b += struct.pack("<%dq" % EMIT, *m["emit"])
    b += struct.pack("<2I", len(m["targets"]), 1 if m["index"] else 0)
    for t in m["targets"]:
        b += struct.pack("<IBBH", t[0], t[1], t[2], 0)
    for row in m["index"]:
        b += struct.pack("<6Q", *row)
    return b
