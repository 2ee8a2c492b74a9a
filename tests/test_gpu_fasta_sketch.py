"""mbgc_fasta_sketch_dev and mbgc_fasta_sketch_pairs_dev (k_fa_sketch, the sort and compaction behind it, k_fa_sketch_pairs: the scans of
`mbgc-hip k`) through the ctypes mirror, on torch buffers, against the numpy referee of tests/_sketch.py. Everything is an integer, so
everything is compared bit for bit: the groups' hash lists, their starts, the k-mer counts, the shared counts. At scale 1 every valid
position emits a row, so the check of the scan is exhaustive. Shapes: texts of a few tiles; k = 1, 2, 15, 16, 17, 31, 32 (the 32-bit
word boundary of the packed codes, the reach into the second neighbour, the 64-bit shift); several records per group, group ids out of
order, a group nobody names, the same text in two groups, a record listed twice, a record that is the reverse complement of another,
records shorter than k, an empty record, a record that ends with a buffer whose size is no multiple of 16; the buffer moved by 1, 5
and 15 bytes; the capacity protocol; a row buffer that has to grow; pairs over lists of 0, 1, 63, 64, 65 and 4097 hashes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _sketch

pytestmark = pytest.mark.gpu
TILE = 4096
KS = [1, 2, 15, 16, 17, 31, 32]
ALPHABET = np.frombuffer(b"ACGTNacgtnRYU>\0", dtype=np.uint8)
LETTERS = np.frombuffer(b"ACGTacgtU", dtype=np.uint8)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbgc_amd", "csrc", "fasta_sketch.h")


def rand(rng, n, every=40):
    """letters with a byte of the whole alphabet every `every` positions or so: k-mers of 32 survive, and many do not"""
    out = LETTERS[rng.integers(0, LETTERS.size, n)]
    other = rng.integers(0, every, n) == 0
    out[other] = ALPHABET[rng.integers(0, ALPHABET.size, int(other.sum()))]
    return out.tobytes()


def on_device(buf, shift=0):
    """the buffer in an allocation of exactly shift + len(buf) bytes (one byte for an empty one) -> (tensor, pointer to its first byte)"""
    import torch
    dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf) + (b"" if shift + len(buf) else b"\0"), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + shift


def referee(buf, ranges, groups, ngroups, k, scale):
    lists, kmers = _sketch.sketch([bytes(buf[o:o + n]) for o, n in ranges], groups, k, _sketch.max_hash(scale), ngroups)
    start = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    return lists, np.concatenate(lists + [np.zeros(0, np.uint64)]), start, np.array(kmers, dtype=np.uint64)


def scan(p, ptr, buf, ranges, groups, ngroups, k, scale, want=None, cap=None):
    lists, flat, start, kmers = want or referee(buf, ranges, groups, ngroups, k, scale)
    hashes, got_start, got_kmers, ms = p.sketch_dev(ptr, len(buf), ranges, groups, ngroups, k=k, max_hash=_sketch.max_hash(scale), cap=cap)
    assert np.array_equal(got_kmers, kmers), (k, scale, got_kmers, kmers)
    assert np.array_equal(got_start, start), (k, scale, got_start, start)
    assert np.array_equal(hashes, flat), (k, scale, hashes.size, flat.size)
    return lists, kmers


@pytest.fixture(scope="module")
def layout():
    """one text of a few tiles and the record list every case of the k sweep uses; the reverse complement of record 1 stands behind it"""
    rng = np.random.default_rng(5)
    body = rand(rng, 3 * TILE + 37)
    r1 = (TILE + 200, 2000)
    buf = body + _sketch.reverse_complement(body[r1[0]:r1[0] + r1[1]]) + rand(rng, 13)
    assert len(buf) % 16
    ranges = [(5, TILE + 100), r1, (5, TILE + 100), (5, TILE + 100), (len(body), r1[1]), (2 * TILE + 3, TILE + 30), (100, 50), (700, 0), (len(buf) - 300, 300)]
    groups = [3, 1, 3, 0, 2, 5, 5, 5, 7]                             # group 4: short records only (added per k); group 6: nobody's
    return buf, ranges, groups, 8


@pytest.mark.parametrize("k", KS)
def test_every_k_at_scale_1_3_and_1000(layout, k):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    ranges = ranges + [(900, k - 1), (3000, k - 1)]                  # records all shorter than k: an empty group
    groups = groups + [4, 4]
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        for scale in (1, 3, 1000):
            lists, kmers = scan(p, ptr, buf, ranges, groups, ngroups, k, scale)
            assert kmers[3] == 2 * kmers[0] > 0 and np.array_equal(lists[3], lists[0])       # listed twice: the k-mers double, the hashes do not
            assert np.array_equal(lists[1], lists[2]) and kmers[1] == kmers[2] > 0           # the reverse complement: the same hashes
            assert lists[4].size == 0 == kmers[4] and lists[6].size == 0 == kmers[6] and kmers[5] > 0 and kmers[7] > 0
            if scale == 1:
                assert lists[0].size > 0 and sum(x.size for x in lists) > (3 if k == 1 else 40)
                rows, reruns, sort_ms = p.last_sketch()
                assert rows == int(kmers.sum()) and reruns == 0 and sort_ms > 0              # every valid position is a row
    finally:
        p.close()


@pytest.mark.parametrize("shift", [1, 5, 15])
def test_the_buffer_moved_by_a_few_bytes(layout, shift):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    dev, ptr = on_device(buf, shift)
    p = fasta.FastaParser()
    try:
        for k in (17, 32):
            scan(p, ptr, buf, ranges, groups, ngroups, k, 1)
    finally:
        p.close()


def test_records_at_every_offset_with_ends_around_a_tile_and_a_wave():
    """a record per offset mod 16, its end k around the first tile's edge or a wave's edge (1024 positions) of its own grid"""
    from mbgc_amd import fasta
    rng = np.random.default_rng(9)
    buf = rand(rng, 2 * TILE + 64, every=300)
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        for k in (16, 31):
            ranges = []
            for off in range(16):
                grid = (ptr + off) % 16
                edge = (TILE if off % 2 else 1024) - grid
                ranges.append((off, edge + (k, -k, k - 1, 1 - k, 0, 1, -1, k + 1)[off % 8]))
            scan(p, ptr, buf, ranges, list(range(16)), 16, k, 1)
    finally:
        p.close()


def test_no_record():
    from mbgc_amd import fasta
    dev, ptr = on_device(b"ACGTACGTACGT")
    p = fasta.FastaParser()
    try:
        hashes, start, kmers, ms = p.sketch_dev(ptr, 12, [], [], 3, k=4, max_hash=_sketch.max_hash(1))
        assert hashes.size == 0 and start.tolist() == [0, 0, 0, 0] and kmers.tolist() == [0, 0, 0]
    finally:
        p.close()


def test_a_hash_buffer_that_is_too_small(layout):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    lists, flat, start, kmers = referee(buf, ranges, groups, ngroups, 21, 3)
    total = int(flat.size)
    assert total > 1000
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        rows = np.asarray(ranges, dtype=np.uint64)
        grp = np.asarray(groups, dtype=np.uint32)
        for cap in (0, total - 1, total):
            out = np.zeros(total, dtype=np.uint64)
            got_start, got_kmers = np.full(ngroups + 1, 77, dtype=np.uint64), np.full(ngroups, 77, dtype=np.uint64)
            n, ms = C.c_uint64(0), C.c_double(0)
            rc = fasta._lib().mbgc_fasta_sketch_dev(p.h, ptr, len(buf), rows.ctypes.data_as(C.POINTER(fasta.CrcRec)), len(ranges), grp.ctypes.data_as(C.c_void_p), ngroups, 21,
                                                    _sketch.max_hash(3), out.ctypes.data_as(C.c_void_p), cap, got_start.ctypes.data_as(C.c_void_p),
                                                    got_kmers.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(ms))
            assert rc == (0 if cap == total else -104) and n.value == total
            assert np.array_equal(got_start, start) and np.array_equal(got_kmers, kmers)          # filled either way
            if cap == total:
                assert np.array_equal(out, flat)
        with pytest.raises(fasta.SketchTooLarge) as e:
            p.sketch_dev(ptr, len(buf), ranges, groups, ngroups, k=21, max_hash=_sketch.max_hash(3), cap=total - 1)
        assert e.value.needed == total
    finally:
        p.close()


def test_a_row_buffer_that_has_to_grow():
    """more rows than the entry point's first device buffer holds (its size is read from the source): the kernel is run again, and the
    sketches are exact all the same"""
    from mbgc_amd import fasta
    first = int(re.search(r"SKETCH_ROWS_FIRST = (\d+);", open(HEADER).read()).group(1))
    rng = np.random.default_rng(21)
    buf = rand(rng, first + 5000, every=2000)
    ranges, groups = [(0, len(buf) // 2), (len(buf) // 2, len(buf) - len(buf) // 2)], [1, 0]
    want = referee(buf, ranges, groups, 2, 21, 1)
    assert int(want[3].sum()) > first
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        scan(p, ptr, buf, ranges, groups, 2, 21, 1, want=want, cap=int(want[1].size))      # (one call: the mirror does not ask twice)
        rows, reruns, _ = p.last_sketch()
        assert rows == int(want[3].sum()) and reruns >= 1
        scan(p, ptr, buf, ranges, groups, 2, 21, 1, want=want, cap=int(want[1].size))      # (the buffer has grown: no rerun now, the same answer)
        assert p.last_sketch()[:2] == (rows, 0)
    finally:
        p.close()


def test_refusals(layout):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        for k in (0, 33):
            with pytest.raises(fasta.binding.SwsemError, match="sketch: k = %d" % k):
                p.sketch_dev(ptr, len(buf), ranges, groups, ngroups, k=k)
        with pytest.raises(fasta.binding.SwsemError, match="sketch: record 1 lies outside the buffer"):
            p.sketch_dev(ptr, len(buf), [(0, 8), (len(buf) - 2, 3)], [0, 0], 1)
        with pytest.raises(fasta.binding.SwsemError, match="sketch: record 1 names group 2 of 2"):
            p.sketch_dev(ptr, len(buf), [(0, 8), (8, 8)], [0, 2], 2)
    finally:
        p.close()


@pytest.fixture(scope="module")
def lists():
    """lists of 0, 1, 63, 64, 65 and 4097 hashes, nested in one another; one identical to the longest, one disjoint from all, one nested
    in the longest (every third), one interleaved with it (every second of it, between hashes of its own)"""
    rng = np.random.default_rng(33)
    pool = np.unique(rng.integers(0, 2 ** 64, 12000, dtype=np.uint64))
    rng.shuffle(pool)
    own, other, third = pool[:4097], pool[4097:8000], pool[8000:10000]
    L = [np.sort(own[:n]) for n in (0, 1, 63, 64, 65, 4097)]
    L += [L[5].copy(), np.sort(other), L[5][::3].copy(), np.sort(np.concatenate([L[5][::2], third]))]
    return L


def test_pairs_over_lists_of_every_size(lists):
    from mbgc_amd import fasta
    flat = np.concatenate(lists)
    start = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    n = len(lists)
    every = [(i, j) for i in range(n) for j in range(i + 1, n)]
    want = np.array([_sketch.shared(lists[i], lists[j]) for i, j in every], dtype=np.uint32)
    at = {pair: q for q, pair in enumerate(every)}
    assert want[at[(5, 6)]] == 4097 and want[at[(5, 7)]] == 0 and want[at[(5, 8)]] == lists[8].size and want[at[(5, 9)]] == lists[5][::2].size
    assert [int(want[at[(i, 5)]]) for i in range(5)] == [0, 1, 63, 64, 65] and want[at[(2, 4)]] == 63
    p = fasta.FastaParser()
    try:
        got, ms = p.sketch_pairs_dev(flat, start)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        explicit = [(5, 5), (9, 5), (5, 9), (0, 0), (0, 5), (3, 2), (5, 9), (1, 1), (8, 6), (7, 7)]
        got, ms = p.sketch_pairs_dev(flat, start, pairs=explicit)
        assert got.tolist() == [_sketch.shared(lists[i], lists[j]) for i, j in explicit] and got[0] == 4097 and got[3] == 0
        assert p.sketch_pairs_dev(flat, start, pairs=np.zeros((0, 2), dtype=np.uint32))[0].size == 0
        assert p.sketch_pairs_dev(lists[5], [0, lists[5].size])[0].size == 0                        # one group: no pair
    finally:
        p.close()


def test_pairs_refuse_a_list_that_does_not_ascend(lists):
    from mbgc_amd import fasta
    p = fasta.FastaParser()
    try:
        for bad in ([1, 3, 3, 9], [1, 5, 2, 9]):
            with pytest.raises(fasta.binding.SwsemError, match="pairs: the hashes of group 1 do not ascend strictly"):
                p.sketch_pairs_dev(np.array([4, 7] + bad, dtype=np.uint64), [0, 2, 6])
        with pytest.raises(fasta.binding.SwsemError, match="pairs: pair 1 names group 2 of 2"):
            p.sketch_pairs_dev(np.array([4, 7, 9], dtype=np.uint64), [0, 2, 3], pairs=[(0, 1), (1, 2)])
        assert p.sketch_pairs_dev(np.array([4, 7, 4, 9], dtype=np.uint64), [0, 2, 4])[0].tolist() == [1]     # (ascending inside each group is all that is asked)
    finally:
        p.close()
