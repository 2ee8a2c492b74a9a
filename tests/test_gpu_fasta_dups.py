"""mbgc_fasta_dups_dev (k_fa_dups and k_fa_dups_verify: the scan of `mbgc-hip u`) through the ctypes mirror, on torch buffers, against
the referee of tests/_dups.py, bit for bit: (rep, strand) of every record and the number of classes, with and without WEAK_HASH (4
bits of fingerprint, so that the exactness step and its rounds run) and with each flag. The referee's own answer is held to show the
property a case is named after before the two are compared. Shapes: record lengths around a vector and a tile at every buffer offset
mod 16, at the buffer's first and last byte; pairs that differ in one byte at a record's edges and on either side of a tile edge;
reverse complements at other alignments; a palindrome; case; the IUPAC pairs; bytes >= 0x80; repeated, overlapping and empty ranges;
a class that is transitive across strands; foreign bytes around records; a random collection with planted copies; the refused call."""
import numpy as np
import pytest

import _dups

pytestmark = pytest.mark.gpu
TILE = 4096
FORWARD_ONLY, EXACT_CASE, WEAK_HASH = 1, 2, 4
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8193]


def rand(rng, n, alphabet=b"ACGTNacgtRY"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, a.size, n)].tobytes()


def on_device(buf, shift=0):
    """the buffer in an allocation of exactly shift + len(buf) bytes (one byte for an empty one) -> (tensor, pointer to its first byte)"""
    import torch
    dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf) + (b"" if shift + len(buf) else b"\0"), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + shift


def scan(buf, ranges, flags=0, shift=0, weak_too=True):
    """dups_dev over `buf` against the referee, with `flags` and with `flags | WEAK_HASH` -> (the referee's [(rep, strand)], classes,
    last_dups() of the weak call)"""
    from mbgc_amd import fasta
    want, classes = _dups.classes([bytes(buf[o:o + n]) for o, n in ranges], forward_only=bool(flags & FORWARD_ONLY), exact_case=bool(flags & EXACT_CASE))
    dev, ptr = on_device(buf, shift)
    p = fasta.FastaParser()
    try:
        last = None
        for f in [flags] + ([flags | WEAK_HASH] if weak_too else []):
            out, n, ms = p.dups_dev(ptr, len(buf), ranges, flags=f)
            got = [(int(r["rep"]), int(r["strand"])) for r in out]
            bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert not bad and len(got) == len(want), (f, bad[:5])
            assert n == classes, (f, n, classes)
            last = p.last_dups()
            assert last[1] >= sum(1 for i, (rep, _) in enumerate(want) if rep != i and ranges[i][1]) and last[2] <= last[1]     # every duplicate with a byte was compared
    finally:
        p.close()
    return want, classes, last


def test_the_comp_table_word_for_word():
    from mbgc_amd import fasta
    assert fasta.dups_comp_table() == _dups.COMP
    assert _dups.COMP[ord("A")] == ord("T") and _dups.COMP[ord("y")] == ord("r") and _dups.COMP[ord("N")] == ord("N") and _dups.COMP[ord("U")] == ord("U") and _dups.COMP[0x80] == 0x80


@pytest.mark.parametrize("offset", range(18))
def test_every_length_at_every_offset(offset):
    """each length three times — fresh, copied, reverse-complemented — the first at `offset` mod 16, the copies wherever they fall, and a
    near-copy that differs in its last byte; foreign bytes between all of them"""
    rng = np.random.default_rng(offset)
    buf, ranges, texts = bytearray(), [], []
    for ln in LENGTHS:
        s = rand(rng, ln)
        buf += rand(rng, (offset - len(buf)) % 16)
        assert len(buf) % 16 == offset % 16
        near = s[:-1] + bytes([s[-1] ^ 0x02]) if ln else b""
        for t in (s, s, _dups.revcomp(s), near):
            ranges.append((len(buf), len(t)))
            buf += t + rand(rng, int(rng.integers(0, 5)))
    want, classes, last = scan(bytes(buf), ranges, shift=offset % 16)
    assert sum(1 for i, (rep, st) in enumerate(want) if rep != i and st == 0) >= len(LENGTHS) and sum(st for _, st in want) >= len(LENGTHS) - 3


@pytest.mark.parametrize("ln", LENGTHS[1:])
def test_at_the_buffers_first_and_last_byte(ln):
    rng = np.random.default_rng(ln)
    s = rand(rng, ln)
    for shift in (0, 3):
        buf = s + rand(rng, 7) + _dups.revcomp(s) + rand(rng, 5) + s
        want, classes, _ = scan(buf, [(0, ln), (ln + 7, ln), (len(buf) - ln, ln)], shift=shift)
        assert [rep for rep, _ in want] == [0, 0, 0] and classes == 1


def test_one_byte_differs_at_the_edges_and_at_a_tile_edge():
    """aligned at 0, the first tile ends behind position 4095; at offset 5 behind position 4090: one byte changed in front of and behind
    each, and in the first and the last byte"""
    rng = np.random.default_rng(1)
    s = rand(rng, 2 * TILE + 100, b"ACGT")
    for start in (0, 5):
        buf, ranges = bytearray(rand(rng, start)), []
        edge = TILE - start
        for at in (None, 0, len(s) - 1, edge - 1, edge, 2 * edge + start - 1 if start else 2 * TILE - 1, 2 * TILE - start):
            t = bytearray(s)
            if at is not None:
                t[at] = ord("A") if t[at] != ord("A") else ord("C")
            ranges.append((len(buf), len(t)))
            buf += t
        want, classes, last = scan(bytes(buf), ranges)
        assert classes == len(ranges) and all(rep == i for i, (rep, _) in enumerate(want))


def test_reverse_complements_palindromes_case_iupac_and_high_bytes():
    rng = np.random.default_rng(2)
    s = rand(rng, 5000)
    pal = b"ACGT" * 1500                                             # its own reverse complement: equal both ways -> strand 0
    assert _dups.revcomp(pal) == pal
    iupac = b"ACGTRYKMBVDHNSWUacgtrykmbvdhnswu" * 40
    high = rand(rng, 300) + bytes([0x80, 0xC1, 0xFF, 0x00]) + rand(rng, 300)
    parts = [s, _dups.revcomp(s), s.lower(), s.swapcase(), pal, pal, pal.lower(), iupac, _dups.revcomp(iupac), high, _dups.revcomp(high), high]
    buf, ranges = bytearray(), []
    for i, t in enumerate(parts):
        buf += rand(rng, 1 + i % 7)                                  # different alignments
        ranges.append((len(buf), len(t)))
        buf += t
    want, classes, _ = scan(bytes(buf), ranges)
    assert want[:7] == [(0, 0), (0, 1), (0, 0), (0, 0), (4, 0), (4, 0), (4, 0)] and want[8] == (7, 1) and want[10] == (9, 1) and want[11] == (9, 0) and classes == 4
    want, classes, _ = scan(bytes(buf), ranges, flags=EXACT_CASE)
    assert want[2] == (2, 0) and want[3] == (3, 0) and want[6] == (6, 0) and want[1] == (0, 1) and classes == 7
    want, classes, _ = scan(bytes(buf), ranges, flags=FORWARD_ONLY)
    assert want[1] == (1, 0) and want[8] == (8, 0) and want[10] == (10, 0) and want[11] == (9, 0) and classes == 7
    scan(bytes(buf), ranges, flags=FORWARD_ONLY | EXACT_CASE)


def test_repeated_overlapping_empty_and_transitive():
    rng = np.random.default_rng(3)
    a = rand(rng, 4500, b"ACGT")
    b = _dups.revcomp(a)
    run = b"A" * 600                                                 # overlapping ranges of one run: equal when of equal length
    buf = a + b"xx" + b + b"yy" + b + run
    o2, o3, o4 = len(a) + 2, 2 * len(a) + 4, 3 * len(a) + 4
    ranges = [(0, len(a)), (o2, len(a)), (o3, len(a)), (0, len(a)), (o4, 500), (o4 + 50, 500), (o4 + 100, 499), (7, 0), (len(buf), 0), (10, 4000), (11, 4000)]
    want, classes, _ = scan(buf, ranges)
    assert want[:4] == [(0, 0), (0, 1), (0, 1), (0, 0)]              # c == b == RC(a): one class across strands; the same range twice
    assert want[4:7] == [(4, 0), (4, 0), (6, 0)] and want[7:9] == [(7, 0), (7, 0)] and want[9:] == [(9, 0), (10, 0)]
    assert classes == 6
    want, _, _ = scan(buf, ranges, flags=FORWARD_ONLY)
    assert want[:4] == [(0, 0), (1, 0), (1, 0), (0, 0)]


def test_foreign_bytes_around_a_record_reach_nothing():
    rng = np.random.default_rng(4)
    for ln in (1, 17, 4097):
        s = rand(rng, ln)
        buf = b"".join(pre + s + post for pre, post in ((b"", b"T"), (b"G", b"A"), (b"ACGTACGTACGTACGTA", b"\xff"), (b"\x00", b"")))
        ranges, at = [], 0
        for pre, post in ((0, 1), (1, 1), (17, 1), (1, 0)):
            ranges.append((at + pre, ln))
            at += pre + ln + post
        want, classes, _ = scan(buf, ranges)
        assert [rep for rep, _ in want] == [0, 0, 0, 0]


def test_a_random_collection_with_planted_copies():
    """300 records over ACGTNacgtRY, lengths up to 9 000 (a third of them from four fixed lengths, so that records of one length that
    are not the same sequence meet in a weak bucket), 40 % planted copies or reverse complements, some with the case changed"""
    rng = np.random.default_rng(5)
    texts = []
    for i in range(300):
        if i >= 10 and rng.random() < 0.4:
            t = texts[int(rng.integers(0, len(texts)))]
            if rng.random() < 0.5:
                t = _dups.revcomp(t)
            if rng.random() < 0.3:
                t = t.swapcase()
        else:
            ln = [16, 100, 4097, 8193][int(rng.integers(0, 4))] if rng.random() < 0.33 else int(rng.integers(0, 9001))
            t = rand(rng, ln)
        texts.append(t)
    buf, ranges = bytearray(), []
    for t in texts:
        buf += rand(rng, int(rng.integers(0, 20)))
        ranges.append((len(buf), len(t)))
        buf += t
    want, _ = _dups.classes(texts)
    assert sum(1 for i, (rep, st) in enumerate(want) if rep != i and st == 0) >= 50 and sum(st for _, st in want) >= 50
    for flags in (0, FORWARD_ONLY, EXACT_CASE):
        _, _, last = scan(bytes(buf), ranges, flags=flags, shift=9)
        assert last[2] > 0, last                                     # WEAK_HASH: the exactness step refuted pairs


def test_a_range_outside_the_buffer_is_refused_and_leaves_out_untouched():
    from mbgc_amd import binding, fasta
    buf = b"ACGT" * 100
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        out = np.full(3, 0xAB, dtype=np.uint8).view(np.uint8).repeat(8).view(fasta.DUP_DTYPE).copy()
        before = out.copy()
        for ranges in ([(0, 10), (395, 6), (0, 10)], [(401, 0), (0, 1), (0, 1)], [(0, 10), (2 ** 63, 2 ** 63), (0, 1)]):
            with pytest.raises(binding.SwsemError, match="outside the buffer"):
                p.dups_dev(ptr, len(buf), ranges, out=out)
            assert out.tobytes() == before.tobytes()
        with pytest.raises(binding.SwsemError, match="flags"):
            p.dups_dev(ptr, len(buf), [(0, 10)], flags=8, out=out)
        assert out.tobytes() == before.tobytes()
        got, n, _ = p.dups_dev(ptr, len(buf), [(0, 10), (394, 6), (4, 10)], out=out)     # (the last byte is inside)
        assert [(int(r["rep"]), int(r["strand"])) for r in got] == [(0, 0), (1, 0), (0, 0)] and n == 2
        got, n, _ = p.dups_dev(ptr, len(buf), np.zeros((0, 2), dtype=np.uint64))
        assert len(got) == 0 and n == 0
    finally:
        p.close()
