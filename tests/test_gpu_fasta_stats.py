"""mbgc_fasta_stats_dev (k_fa_stats: the scan of `mbgc-hip s`) through the ctypes mirror, on torch buffers, against the numpy referee of
tests/_stats.py: the eight counters of every record and the whole table of runs (rec, cls, start, len) must be equal, and the
referee's own table is held non-empty for the property a case is named after before the two are compared. Shapes: the smallest at
which the kernel can go wrong — record lengths around a vector and a tile at every kind of buffer offset, neighbours without a byte
between them, runs at the tiles' edges, overlapping records, a record that ends with a buffer whose size is no multiple of 16, more
tiles than a grid dimension holds, the two classes over the same bytes, the minimum lengths, every flag alone, the capacity protocol,
an edge buffer that has to grow, and the call that is refused before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _stats

pytestmark = pytest.mark.gpu
TILE = 4096
ALPHABET = np.frombuffer(b"ACGTNacgtnRYU>\0", dtype=np.uint8)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbgc_amd", "csrc", "fasta_stats.h")


def rand(rng, n, alphabet=ALPHABET):
    return alphabet[rng.integers(0, alphabet.size, n)].tobytes()


def lumpy(rng, n):
    """random bytes with stretches of N, n and lower case planted, so that runs of every length up to a few hundred stand in it"""
    out = bytearray(rand(rng, n))
    for _ in range(max(1, n // 150)):
        at, ln = int(rng.integers(0, n)), int(rng.integers(1, 300))
        piece = [b"N", b"n", b"acgtn", b"Nn"][int(rng.integers(0, 4))]
        out[at:at + ln] = (piece * ln)[:min(ln, n - at)]
    return bytes(out)


def on_device(buf, shift=0):
    """the buffer in an allocation of exactly shift + len(buf) bytes (one byte for an empty one) -> (tensor, pointer to its first byte)"""
    import torch
    dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf) + (b"" if shift + len(buf) else b"\0"), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + shift


def scan(buf, ranges, flags=7, min_n=1, min_lower=1, shift=0, run_cap=None, least=0, least_cls=None):
    """stats_dev over `buf` on the device against the referee -> (counts, the table of runs); the referee must hold at least `least`
    runs (of class least_cls, when given). shift: the buffer starts that many bytes into its allocation"""
    from mbgc_amd import fasta
    want_counts, want = _stats.table(buf, ranges, flags, min_n, min_lower)
    held = [r for r in want if least_cls is None or r[1] == least_cls]
    assert len(held) >= least, "the referee finds %d runs: the case does not test what it is named for" % len(held)
    dev, ptr = on_device(buf, shift)
    p = fasta.FastaParser()
    try:
        counts, runs, ms = p.stats_dev(ptr, len(buf), ranges, flags=flags, min_run_n=min_n, min_run_lower=min_lower, run_cap=run_cap)
    finally:
        p.close()
    table = [(int(r["rec"]), int(r["cls"]), int(r["start"]), int(r["len"])) for r in runs]
    assert table == want, (len(table), len(want), sorted(set(table) - set(want))[:5], sorted(set(want) - set(table))[:5])
    assert table == sorted(set(table))                               # sorted by (rec, cls, start), each once
    if flags & 1:
        assert np.array_equal(counts, want_counts), (counts[:4], want_counts[:4])
        assert all(int(counts[r, :6].sum()) == int(ln) for r, (_, ln) in enumerate(ranges)) and not counts[:, 7].any()
    return counts, table


@pytest.mark.parametrize("offset", [0, 1, 5, 15])
def test_lengths_around_a_vector_and_a_tile_at_every_offset(offset):
    """records of 0, 1, 15, 16, 17, T - 1, T, T + 1 and 3 T + 5 bytes, each starting at `offset` mod 16 of the buffer's addresses"""
    rng = np.random.default_rng(offset)
    buf, ranges = bytearray(), []
    for ln in [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]:
        buf += rand(rng, (offset - len(buf)) % 16)
        assert len(buf) % 16 == offset
        ranges.append((len(buf), ln))
        buf += lumpy(rng, ln) if ln else b""
    counts, table = scan(bytes(buf), ranges, least=40)
    assert {r for r, _, _, _ in table} >= {5, 6, 7, 8} and [int(c[:6].sum()) for c in counts] == [ln for _, ln in ranges]


@pytest.mark.parametrize("letters", [(b"N", b"A", 0), (b"c", b"C", 1)])
def test_neighbours_without_a_byte_between_them(letters):
    """the first record ends in three bytes of the class and the second starts with two: two runs, not one of five"""
    inside, outside, cls = letters
    first, second = outside * 20 + inside * 3, inside * 2 + outside * 20
    _, table = scan(first + second, [(0, len(first)), (len(first), len(second))], least=2, least_cls=cls)
    assert [r for r in table if r[1] == cls] == [(0, cls, 20, 3), (1, cls, 0, 2)]
    # ... also where the joint is the joint of two lanes, of two waves and of two tiles
    for joint in (16, 1024, TILE):
        first = outside * (joint - 3) + inside * 3
        _, table = scan(first + second, [(0, joint), (joint, len(second))], least=2, least_cls=cls)
        assert [r for r in table if r[1] == cls] == [(0, cls, joint - 3, 3), (1, cls, 0, 2)]


def test_runs_at_the_tiles_edges():
    T = TILE
    plant = {"starts on a tile's last position": (T - 1, 7), "ends on the next tile's first position": (T - 9, 10), "two bytes over the edge": (T - 1, 2),
             "three whole tiles": (T, 3 * T), "one byte at the edge": (T - 1, 1), "one byte behind the edge": (T, 1), "over a wave's edge": (1020, 9)}
    buf, ranges, want = bytearray(), [], []
    for start, ln in plant.values():
        rec = bytearray(b"ACGT" * (5 * T // 4))
        rec[start:start + ln] = b"n" * ln
        ranges.append((len(buf), len(rec)))
        want.append((start, ln))
        buf += rec
    _, table = scan(bytes(buf), ranges, least=2 * len(plant))
    assert [(s, ln) for _, cls, s, ln in table if cls == 0] == want == [(s, ln) for _, cls, s, ln in table if cls == 1]


def test_a_record_that_is_one_run_and_one_of_runs_of_one_byte():
    whole = b"t" * (2 * TILE + 100)
    alternating = b"aA" * 3000
    buf = b"g" * 7 + whole + b"c" * 9 + alternating + b"a"           # (lower case on both sides of both records: it is not theirs)
    ranges = [(7, len(whole)), (7 + len(whole) + 9, len(alternating))]
    counts, table = scan(buf, ranges, least=3001, least_cls=1)
    assert table[0] == (0, 1, 0, len(whole)) and [r for r in table if r[0] == 1] == [(1, 1, 2 * i, 1) for i in range(3000)]
    assert int(counts[0, 3]) == int(counts[0, 6]) == len(whole) and int(counts[1, 0]) == 6000 and int(counts[1, 6]) == 3000


def test_overlapping_records_and_the_same_record_twice():
    rng = np.random.default_rng(11)
    buf = lumpy(rng, 3 * TILE)
    ranges = [(100, 2 * TILE), (TILE, TILE + 500), (100, 2 * TILE), (0, 3 * TILE), (TILE + 7, 0), (2 * TILE, 17)]
    counts, table = scan(buf, ranges, least=30)
    assert [r[1:] for r in table if r[0] == 0] == [r[1:] for r in table if r[0] == 2] and np.array_equal(counts[0], counts[2])


@pytest.mark.parametrize("shift", [0, 3])
def test_the_last_record_ends_with_the_buffer(shift):
    """seqBytes is no multiple of 16 and the allocation ends where the buffer ends: the last vector is read byte by byte"""
    rng = np.random.default_rng(13)
    buf = lumpy(rng, TILE + 21)[:-7] + b"A" + b"nnnNNN"
    assert (len(buf) + shift) % 16
    _, table = scan(buf, [(5, 40), (len(buf) - 300, 300), (len(buf) - 3, 3), (len(buf), 0)], shift=shift, least=4)
    assert (1, 0, 294, 6) in table and (2, 0, 0, 3) in table and (1, 1, 294, 3) in table and not [r for r in table if r[:2] == (2, 1)]


def test_no_record_and_records_without_a_byte():
    counts, table = scan(b"NNNNnnnn", [], least=0)
    assert counts.shape == (0, 8) and table == []
    counts, table = scan(b"NNNNnnnn", [(0, 0), (8, 0)], least=0)
    assert counts.shape == (2, 8) and not counts.any() and table == []


def test_seventy_thousand_tiles():
    """70 000 records of one byte: more tiles than a grid dimension of 65 535 holds"""
    from mbgc_amd import fasta
    rng = np.random.default_rng(17)
    buf = rand(rng, 70_000)
    ranges = np.stack([np.arange(70_000), np.ones(70_000)], axis=1).astype(np.uint64)
    # the referee, a byte value at a time: a record of one byte has that byte's counters, and is a run of one when it is in the class
    x = np.frombuffer(buf, dtype=np.uint8)
    want_counts = np.array([_stats.counts(bytes([v])) for v in range(256)], dtype=np.uint64)[x]
    want = sorted((int(r), cls, 0, 1) for cls in (0, 1) for r in np.flatnonzero(_stats.class_mask(buf, cls)))
    assert len(want) >= 10_000 and {cls for _, cls, _, _ in want} == {0, 1}
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        counts, runs, ms = p.stats_dev(ptr, len(buf), ranges)
    finally:
        p.close()
    assert np.array_equal(counts, want_counts)
    assert list(zip(runs["rec"].tolist(), runs["cls"].tolist(), runs["start"].tolist(), runs["len"].tolist())) == want


def test_the_two_classes_over_the_same_bytes():
    text = b"ACGT" + b"n" * 50 + b"ACGT" + b"N" * 60 + b"AC"
    _, table = scan(text, [(0, len(text))], least=3)
    assert table == [(0, 0, 4, 50), (0, 0, 58, 60), (0, 1, 4, 50)]   # n: both classes; N: class 0 only


def test_minimum_lengths():
    text = b"A" + b"N" * 2 + b"C" + b"N" * 3 + b"G" + b"n" * 4 + b"T" + b"a" * 2 + b"T"
    assert [r[2:] for r in scan(text, [(0, len(text))], min_n=3, least=3)[1] if r[1] == 0] == [(4, 3), (8, 4)]
    assert [r[2:] for r in scan(text, [(0, len(text))], min_n=4, min_lower=3, least=2)[1]] == [(8, 4), (8, 4)]
    assert scan(text, [(0, len(text))], min_n=0, min_lower=0, least=5)[1] == scan(text, [(0, len(text))], min_n=1, min_lower=1, least=5)[1]


def test_every_flag_alone():
    from mbgc_amd import fasta
    rng = np.random.default_rng(19)
    buf = lumpy(rng, TILE + 50)
    ranges = [(3, TILE), (TILE - 20, 60)]
    counts, _ = scan(buf, ranges, flags=fasta.STATS_COUNTS, least=0)
    assert counts.any()
    assert {r[1] for r in scan(buf, ranges, flags=fasta.STATS_NRUNS, least=3)[1]} == {0}
    assert {r[1] for r in scan(buf, ranges, flags=fasta.STATS_LOWER, least=3)[1]} == {1}
    # without COUNTS the counts buffer is not touched
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        rows = np.asarray(ranges, dtype=np.uint64)
        cnt = np.full((2, 8), 0xABABABABABABABAB, dtype=np.uint64)
        runs = np.zeros(4096, dtype=fasta.RUN_DTYPE)
        n, ms = C.c_uint64(0), C.c_double(0)
        rc = fasta._lib().mbgc_fasta_stats_dev(p.h, ptr, len(buf), rows.ctypes.data_as(C.POINTER(fasta.CrcRec)), 2, fasta.STATS_NRUNS | fasta.STATS_LOWER, 1, 1,
                                               cnt.ctypes.data_as(C.c_void_p), runs.ctypes.data_as(C.c_void_p), 4096, C.byref(n), C.byref(ms))
        assert rc == 0 and n.value > 6 and (cnt == 0xABABABABABABABAB).all()
    finally:
        p.close()


def test_a_run_buffer_that_is_too_small():
    from mbgc_amd import fasta
    rng = np.random.default_rng(23)
    buf = lumpy(rng, 2 * TILE)
    ranges = [(0, 2 * TILE)]
    full = scan(buf, ranges, least=20)[1]
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        rows = np.asarray(ranges, dtype=np.uint64)
        for cap in (0, len(full) - 1):
            runs = np.frombuffer(b"\xab" * (fasta.RUN_DTYPE.itemsize * len(full)), dtype=fasta.RUN_DTYPE).copy()
            before = runs.tobytes()
            cnt = np.zeros((1, 8), dtype=np.uint64)
            n, ms = C.c_uint64(0), C.c_double(0)
            rc = fasta._lib().mbgc_fasta_stats_dev(p.h, ptr, len(buf), rows.ctypes.data_as(C.POINTER(fasta.CrcRec)), 1, 7, 1, 1, cnt.ctypes.data_as(C.c_void_p),
                                                   runs.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(ms))
            assert rc == -104 and n.value == len(full) and runs.tobytes() == before
        with pytest.raises(fasta.RunsTooMany) as e:
            p.stats_dev(ptr, len(buf), ranges, run_cap=len(full) - 1)
        assert e.value.needed == len(full)
    finally:
        p.close()
    assert scan(buf, ranges, run_cap=len(full), least=20)[1] == full
    many = b"nA" * 5000                                              # more runs than the mirror's first buffer: it asks again by itself
    assert len(scan(many, [(0, len(many))], least=10_000)[1]) == 10_000


def test_an_edge_buffer_that_has_to_grow():
    """more edges than the entry point's first device buffer holds (its size is read from the source): the kernel is run again, and the
    rows are exact all the same"""
    from mbgc_amd import fasta
    first = int(re.search(r"STATS_EDGES_FIRST = (\d+);", open(HEADER).read()).group(1))
    assert first >= 50_000
    runs = first // 2 + 1000                                         # two edges per run and class
    text = b"Na" * runs + b"ACGT" * 100
    assert 4 * runs > max(first, 100_000)
    want_counts, want = _stats.table(text, [(0, len(text))])
    assert len(want) == 2 * runs
    dev, ptr = on_device(text)
    p = fasta.FastaParser()
    try:
        counts, got, ms = p.stats_dev(ptr, len(text), [(0, len(text))], run_cap=2 * runs)
        edges, reruns = p.last_stats()
        again = p.stats_dev(ptr, len(text), [(0, len(text))], run_cap=2 * runs)[1]     # (the buffer has grown: no rerun now, the same rows)
        assert p.last_stats() == (4 * runs, 0)
    finally:
        p.close()
    assert [(int(r["rec"]), int(r["cls"]), int(r["start"]), int(r["len"])) for r in got] == want and got.tobytes() == again.tobytes()
    assert np.array_equal(counts, want_counts) and edges == 4 * runs and reruns == 1


def test_a_record_past_the_buffer_is_refused_and_nothing_is_launched():
    from mbgc_amd import fasta
    text = b"ACGTNNNNacgtnnnnACGTNNNNacgtnnnn"
    dev, ptr = on_device(text)
    p = fasta.FastaParser()
    try:
        with pytest.raises(fasta.binding.SwsemError, match="stats: record 1 lies outside the buffer"):
            p.stats_dev(ptr, len(text), [(0, 8), (30, 3)])
        rows = np.asarray([(0, 8), (30, 3)], dtype=np.uint64)
        cnt = np.full((2, 8), 0xABABABABABABABAB, dtype=np.uint64)
        runs = np.zeros(8, dtype=fasta.RUN_DTYPE)
        runs["start"] = 0xCDCD
        before = runs.tobytes()
        n, ms = C.c_uint64(777), C.c_double(-1.0)
        rc = fasta._lib().mbgc_fasta_stats_dev(p.h, ptr, len(text), rows.ctypes.data_as(C.POINTER(fasta.CrcRec)), 2, 7, 1, 1, cnt.ctypes.data_as(C.c_void_p),
                                               runs.ctypes.data_as(C.c_void_p), 8, C.byref(n), C.byref(ms))
        assert rc == -103 and n.value == 777 and ms.value == -1.0 and runs.tobytes() == before and (cnt == 0xABABABABABABABAB).all()
        assert p.stats_dev(ptr, len(text), [(0, 8), (29, 3)])[1].size == 3      # (one byte less: inside)
    finally:
        p.close()
