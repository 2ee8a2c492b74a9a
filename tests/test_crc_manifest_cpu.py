"""mbgc_fasta_crc_combine (host arithmetic in libmbgc_hip.so, which loads without a device as tests/test_abi.py loads it) against
zlib.crc32(a + b) and against the combine written here from zlib's definition — the lengths beyond 2^32 are given as numbers, their
bytes never exist —, and the format of <prefix>.checksums: a manifest built here is read back field by field. No GPU."""
import struct
import zlib

import numpy as np

POLY = 0xEDB88320


def mulmod(a, b):
    """a * b mod P, bit-reflected (zlib's multmodp)"""
    p, m = 0, 1 << 31
    while m:
        if a & m:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
        m >>= 1
    return p


def x_pow_8n(n):
    p, sq = 1 << 31, 1 << 23                 # 1, x^8
    while n:
        if n & 1:
            p = mulmod(sq, p)
        sq = mulmod(sq, sq)
        n >>= 1
    return p


def combine(crc_a, crc_b, len_b):
    return mulmod(x_pow_8n(len_b), crc_a) ^ crc_b


def lib_combine():
    import __graft_entry__ as g
    g.build()
    from mbgc_amd import fasta
    return fasta.crc_combine


def test_combine_equals_zlib_on_real_bytes():
    f = lib_combine()
    rng = np.random.default_rng(5)
    for la, lb in [(0, 0), (0, 1), (1, 0), (1, 1), (5, 2), (1000, 1), (3, 70_000), (70_000, 3), (16384, 16384), (16385, 255)]:
        for fill in ("random", 0x00, 0xFF):
            a = rng.integers(0, 256, la, dtype=np.uint8).tobytes() if fill == "random" else bytes([fill]) * la
            b = rng.integers(0, 256, lb, dtype=np.uint8).tobytes() if fill == "random" else bytes([fill]) * lb
            want = zlib.crc32(a + b)
            assert combine(zlib.crc32(a), zlib.crc32(b), lb) == want
            assert f(zlib.crc32(a), zlib.crc32(b), lb) == want, (la, lb, fill)


def test_combine_with_lengths_beyond_32_bits():
    f = lib_combine()
    rng = np.random.default_rng(6)
    for len_b in (0, 1, 2 ** 32 - 1, 2 ** 32 + 5):
        for _ in range(4):
            ca, cb = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))
            assert f(ca, cb, len_b) == combine(ca, cb, len_b), len_b
    # the two big lengths are told apart (a length cut to 32 bits would make 2^32 + 5 the same as 5)
    assert f(0x12345678, 0, 2 ** 32 + 5) != f(0x12345678, 0, 5)
    # ... and agree with real bytes where the split makes them small: crc(A + B + C) from (A + B, C) and from (A, B + C)
    a, b, c = b"ACGT" * 10, b"N" * 77, b"acgtn" * 1000
    assert f(zlib.crc32(a + b), zlib.crc32(c), len(c)) == f(zlib.crc32(a), zlib.crc32(b + c), len(b) + len(c)) == zlib.crc32(a + b + c)


def build_manifest(side_files, contigs):
    """the format of <prefix>.checksums, written from its description: magic, u64 N, four u32 (0 for a file that is not written), N u32"""
    out = b"MBGCCRC1" + struct.pack("<Q", len(contigs))
    out += b"".join(struct.pack("<I", zlib.crc32(s) if s is not None else 0) for s in side_files)
    return out + b"".join(struct.pack("<I", zlib.crc32(c)) for c in contigs)


def parse_manifest(data):
    assert data[:8] == b"MBGCCRC1"
    (n,) = struct.unpack_from("<Q", data, 8)
    side = struct.unpack_from("<4I", data, 16)
    assert len(data) == 32 + 4 * n
    return list(side), list(struct.unpack_from("<%dI" % n, data, 32))


def test_manifest_round_trip():
    contigs = [b"", b"A", b"ACGT" * 1000, b"acgtn", b"\xff" * 300]
    side = [b"meta bytes", b"g00.fa\ng01.fa\n", None, b"\x50\0\0\0\0\0\0\0"]
    data = build_manifest(side, contigs)
    assert len(data) == 8 + 8 + 16 + 4 * len(contigs)
    got_side, got = parse_manifest(data)
    assert got == [zlib.crc32(c) for c in contigs] and got[0] == 0
    assert got_side == [zlib.crc32(side[0]), zlib.crc32(side[1]), 0, zlib.crc32(side[3])]
    assert parse_manifest(build_manifest([None] * 4, [])) == ([0, 0, 0, 0], [])
