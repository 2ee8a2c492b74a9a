"""mbgc_fasta_screen_dev (k_fa_screen, the sorts and the compaction behind it: the scan of `mbgc-hip m`) through the ctypes mirror, on
torch buffers, against the referee of tests/_screen.py. Everything is an integer, so everything is compared bit for bit: the groups'
lists of found key indices, their starts, and the hit rows (pos, rec, key) in (rec, pos) order. Shapes, the smallest that can go wrong:
texts of a few tiles; k = 1, 2, 15, 16, 17, 31, 32; records at every offset mod 16 with 0, k - 1, k and k + 1 bytes; a record that ends on
the last byte of a buffer whose size is no multiple of 16; records whose k-mers straddle a tile's edge (4096) and a wave's edge (1024);
overlapping and repeated records in different groups, a group nobody names; N, lower case and U in the text; a key met only as its
reverse complement; a key that is its own reverse complement; a single key; 200 000 random keys, which set every bit of the filter so
that everything goes through the table; a text of 70 000 bytes screened with its own k-mers, where every position hits and the first row
buffer overflows; both capacity protocols; the refusals (all but the 2^24 bound, which tests/test_cli_screen_refusals.py meets)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _screen

pytestmark = pytest.mark.gpu
TILE = 4096
KS = [1, 2, 15, 16, 17, 31, 32]
ALPHABET = np.frombuffer(b"ACGTNacgtnRYU>\0", dtype=np.uint8)
LETTERS = np.frombuffer(b"ACGTacgtU", dtype=np.uint8)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbgc_amd", "csrc", "fasta_screen.h")


def rand(rng, n, every=40):
    """letters with a byte of the whole alphabet every `every` positions or so: k-mers of 32 survive, and many do not"""
    out = LETTERS[rng.integers(0, LETTERS.size, n)]
    other = rng.integers(0, every, n) == 0
    out[other] = ALPHABET[rng.integers(0, ALPHABET.size, int(other.sum()))]
    return out.tobytes()


def random_words(rng, n, k):
    """n random canonical words of 2 k bits"""
    w = rng.integers(0, 2 ** 64, n, dtype=np.uint64) >> np.uint64(64 - 2 * k)
    return np.unique(np.minimum(w, rc_words(w, k)))


def rc_words(w, k):
    out = np.zeros_like(w)
    for j in range(k):
        out |= (np.uint64(3) - ((w >> np.uint64(2 * j)) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return out


def on_device(buf, shift=0):
    """the buffer in an allocation of exactly shift + len(buf) bytes -> (tensor, pointer to its first byte)"""
    import torch
    dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf) + (b"" if shift + len(buf) else b"\0"), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + shift


def referee(buf, ranges, groups, ngroups, keys, k):
    found, hits = _screen.screen([bytes(buf[o:o + n]) for o, n in ranges], groups, ngroups, keys, k)
    start = np.concatenate([[0], np.cumsum([x.size for x in found])]).astype(np.uint64)
    rows = np.zeros(len(hits), dtype=[("pos", "<u8"), ("rec", "<u4"), ("key", "<u4")])
    if hits:
        rows["rec"], rows["pos"], rows["key"] = np.array(hits, dtype=np.int64).T
    return found, np.concatenate(found + [np.zeros(0, np.uint32)]), start, rows


def scan(p, ptr, buf, ranges, groups, ngroups, keys, k, want=None):
    found, flat, start, rows = want or referee(buf, ranges, groups, ngroups, keys, k)
    got, got_start, got_rows, ms = p.screen_dev(ptr, len(buf), ranges, groups, ngroups, keys, k=k, hits=True)
    assert np.array_equal(got_start, start), (k, got_start, start)
    assert np.array_equal(got, flat), (k, got.size, flat.size)
    assert got_rows.dtype == rows.dtype and np.array_equal(got_rows, rows), (k, got_rows.size, rows.size)
    again, again_start, none, ms = p.screen_dev(ptr, len(buf), ranges, groups, ngroups, keys, k=k)     # (without the hit rows: the same lists)
    assert none is None and np.array_equal(again, flat) and np.array_equal(again_start, start)
    assert p.last_screen()[0] == rows.size
    return found, rows


def keys_of(buf, parts, k, extra=()):
    """the canonical k-mers of the stretches parts = [(off, len)] of buf, and the words of extra"""
    own = [_screen.canons(buf[o:o + n], k)[0] for o, n in parts] + [np.asarray(extra, dtype=np.uint64)]
    return np.unique(np.concatenate(own))


@pytest.fixture(scope="module")
def layout():
    """one text of a few tiles and the record list every case of the k sweep uses; the reverse complement of record 1 stands behind it"""
    rng = np.random.default_rng(5)
    body = rand(rng, 3 * TILE + 37)
    r1 = (TILE + 200, 2000)
    buf = body + _screen.reverse_complement(body[r1[0]:r1[0] + r1[1]]) + rand(rng, 13)
    assert len(buf) % 16
    # records 0, 2, 3: the same stretch in groups 3, 3 and 0; 1 and 4: a stretch and its reverse complement; 5 overlaps 0 across the second
    # tile's edge; 6: short; 7: empty; 8: ends on the buffer's last byte
    ranges = [(5, TILE + 100), r1, (5, TILE + 100), (5, TILE + 100), (len(body), r1[1]), (TILE - 40, 2 * TILE + 90), (100, 50), (700, 0), (len(buf) - 300, 300)]
    groups = [3, 1, 3, 0, 2, 5, 5, 5, 7]                             # group 4: short records only (added per k); group 6: nobody's
    return buf, ranges, groups, 8


@pytest.mark.parametrize("k", KS)
def test_every_k(layout, k):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    ranges = ranges + [(900, k - 1), (3000, k - 1)]                  # records all shorter than k: an empty group
    groups = groups + [4, 4]
    rng = np.random.default_rng(100 + k)
    # the k-mers around the first tile's edge, around a wave's edge, of the text's last bytes and of a stretch inside the reverse
    # complement's original alone, and random words that are k-mers of nothing
    keys = keys_of(buf, [(TILE - 100, 200), (1024 - 40, 80), (len(buf) - 100, 100), (TILE + 700, 300)], k, random_words(rng, 3000, k) if k >= 15 else ())
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        found, rows = scan(p, ptr, buf, ranges, groups, ngroups, keys, k)
        assert np.array_equal(found[3], found[0]) and found[0].size > 0                    # listed twice and in two groups: the same keys
        assert np.array_equal(found[1], found[2]) and found[1].size > 0                    # the reverse complement: the same keys
        assert found[4].size == 0 and found[6].size == 0 and found[5].size > 0 and found[7].size > 0
        assert rows.size > 500 and (k < 15 or rows.size < sum(n for _, n in ranges))       # (at k >= 15 most positions are no hit)
        passes = p.last_screen()[1]
        assert passes >= rows.size
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
            scan(p, ptr, buf, ranges, groups, ngroups, keys_of(buf, [(TILE - 100, 200), (len(buf) - 100, 100)], k), k)
    finally:
        p.close()


def test_records_at_every_offset_with_short_lengths_and_ends_around_a_tile_and_a_wave():
    """a record per offset mod 16 with 0, k - 1, k and k + 1 bytes, and one whose end stands k around the first tile's edge or a wave's
    edge (1024 positions) of its own grid; every k-mer of the text is a key, so every valid position must come back"""
    from mbgc_amd import fasta
    rng = np.random.default_rng(9)
    buf = rand(rng, 2 * TILE + 64, every=300)
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        for k in (16, 31):
            keys = keys_of(buf, [(0, len(buf))], k)
            ranges = []
            for off in range(16):
                grid = (ptr + off) % 16
                edge = (TILE if off % 2 else 1024) - grid
                ranges.append((off, edge + (k, -k, k - 1, 1 - k, 0, 1, -1, k + 1)[off % 8]))
                ranges.append((200 + off, (0, k - 1, k, k + 1)[off % 4]))
                ranges.append((517 + 33 * off, (0, k - 1, k, k + 1)[(off + 1) % 4]))
            found, rows = scan(p, ptr, buf, ranges, list(range(len(ranges))), len(ranges), keys, k)
            assert rows.size > 16 * 500
    finally:
        p.close()


def test_reverse_complement_only_a_palindrome_a_single_key_n_lower_case_and_u():
    from mbgc_amd import fasta
    k = 16
    gene = b"ACGGTCATTGCAGCTA"                                            # met only as its reverse complement, in lower case with a u
    rc = _screen.reverse_complement(gene).lower().replace(b"t", b"u", 1)
    pal = b"ACGTTGCAtgcaACGT"                                             # its own reverse complement
    assert _screen.reverse_complement(pal).upper() == pal.upper() and rc.count(b"u") == 1
    buf = b"N" * 37 + rc + b"NNN" + pal + b"n" * 50 + gene[:15] + b"N" + gene[1:] + b"RY" + pal.lower() + b"NN"
    assert gene not in buf.upper()
    key_gene, key_pal = int(_screen.canons(gene, k)[0][0]), int(_screen.canons(pal, k)[0][0])
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        ranges, groups = [(0, len(buf)), (37, 16), (38, 16)], [0, 1, 2]
        for keys in ([key_gene], [key_pal], sorted([key_gene, key_pal])):
            found, rows = scan(p, ptr, buf, ranges, groups, 3, np.array(keys, dtype=np.uint64), k)
            assert found[2].size == 0
        assert [len(f) for f in found] == [2, 1, 0] and rows["pos"].tolist()[:3] == [37, 56, len(buf) - 18]
        found, rows = scan(p, ptr, buf, ranges, groups, 3, np.array([key_gene ^ 1], dtype=np.uint64), k)      # a single key nobody holds
        assert rows.size == 0 and all(f.size == 0 for f in found)
    finally:
        p.close()


def test_200_000_random_keys_saturate_the_filter(layout):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    k = 21
    rng = np.random.default_rng(77)
    keys = keys_of(buf, [(TILE - 100, 200), (TILE + 700, 300)], k, random_words(rng, 200_000, k))
    assert keys.size > 199_000
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        found, rows = scan(p, ptr, buf, ranges, groups, ngroups, keys, k)
        valid = sum(_screen.canons(buf[o:o + n], k)[0].size for o, n in ranges)
        rows_dev, passes, reruns, sort_ms = p.last_screen()
        assert rows.size > 300 and valid > 5 * rows.size and passes > 0.7 * valid          # 1 - exp(-200000 / 2^17) = 78 % of the filter's bits are set
    finally:
        p.close()


def test_every_position_hits_and_the_row_buffer_grows():
    """70 000 bytes screened with their own k-mers: more rows than the entry point's first device buffer holds (its size is read from the
    source), the kernel is run again, and the answer is exact all the same"""
    from mbgc_amd import fasta
    first = int(re.search(r"SCREEN_ROWS_FIRST = (\d+);", open(HEADER).read()).group(1))
    k = 21
    rng = np.random.default_rng(21)
    buf = LETTERS[rng.integers(0, LETTERS.size, 70_000)].tobytes()
    keys = keys_of(buf, [(0, len(buf))], k)
    ranges, groups = [(0, len(buf) // 2 + k - 1), (len(buf) // 2, len(buf) - len(buf) // 2)], [1, 0]
    want = referee(buf, ranges, groups, 2, keys, k)
    assert want[3].size == len(buf) - k + 1 > first == 65536
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        got, start, rows, ms = p.screen_dev(ptr, len(buf), ranges, groups, 2, keys, k=k, found_cap=int(want[1].size), hits=True, hit_cap=int(want[3].size))     # (one call)
        assert np.array_equal(got, want[1]) and np.array_equal(start, want[2]) and np.array_equal(rows, want[3])
        n, passes, reruns, sort_ms = p.last_screen()
        assert n == want[3].size == passes and reruns >= 1 and sort_ms > 0
        scan(p, ptr, buf, ranges, groups, 2, keys, k, want=want)
        assert p.last_screen()[2] == 0                                                     # (the buffer has grown: no rerun now)
    finally:
        p.close()


def test_both_capacity_protocols(layout):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    k = 17
    keys = keys_of(buf, [(TILE - 100, 200), (TILE + 700, 300)], k)
    found, flat, start, rows = referee(buf, ranges, groups, ngroups, keys, k)
    total, nhits = int(flat.size), int(rows.size)
    assert total > 500 and nhits > total
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        rec = np.asarray(ranges, dtype=np.uint64)
        grp = np.asarray(groups, dtype=np.uint32)

        def raw(found_cap, hit_cap, want_hits=True):
            out, got_start = np.full(total + 1, 77, dtype=np.uint32), np.full(ngroups + 1, 77, dtype=np.uint64)
            hits = np.full(nhits + 1, 77, dtype=fasta.SCREEN_HIT_DTYPE)
            t, n, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
            rc = fasta._lib().mbgc_fasta_screen_dev(p.h, ptr, len(buf), rec.ctypes.data_as(C.POINTER(fasta.CrcRec)), len(ranges), grp.ctypes.data_as(C.c_void_p), ngroups, k,
                                                    keys.ctypes.data_as(C.c_void_p), keys.size, out.ctypes.data_as(C.c_void_p), found_cap, got_start.ctypes.data_as(C.c_void_p),
                                                    C.byref(t), hits.ctypes.data_as(C.c_void_p) if want_hits else None, hit_cap, C.byref(n), C.byref(ms))
            assert t.value == total and n.value == nhits                                   # exact either way
            assert np.array_equal(got_start, start)                                        # filled either way
            return rc, out, hits
        for cap in (0, total - 1):
            rc, out, hits = raw(cap, nhits)
            assert rc == -104 and np.all(hits["pos"] == 77)
        for cap in (0, nhits - 1):
            rc, out, hits = raw(total, cap)
            assert rc == -104 and np.all(hits["pos"] == 77) and np.all(hits["key"] == 77)  # no hit is written
        rc, out, hits = raw(total, nhits)
        assert rc == 0 and np.array_equal(out[:total], flat) and np.array_equal(hits[:nhits], rows) and out[total] == 77 and hits[nhits]["pos"] == 77
        rc, out, hits = raw(total, 0, want_hits=False)                                     # (no hit buffer: its capacity does not matter)
        assert rc == 0 and np.array_equal(out[:total], flat)
        with pytest.raises(fasta.ScreenTooLarge) as e:
            p.screen_dev(ptr, len(buf), ranges, groups, ngroups, keys, k=k, found_cap=total - 1)
        assert e.value.needed == total
        with pytest.raises(fasta.HitsTooMany) as e:
            p.screen_dev(ptr, len(buf), ranges, groups, ngroups, keys, k=k, hits=True, hit_cap=nhits - 1)
        assert e.value.needed == nhits
    finally:
        p.close()


def test_no_record_and_no_k_mer():
    from mbgc_amd import fasta
    dev, ptr = on_device(b"ACGTACGTACGT")
    p = fasta.FastaParser()
    try:
        for ranges, groups in (([], []), ([(0, 3), (5, 0)], [2, 0])):
            found, start, rows, ms = p.screen_dev(ptr, 12, ranges, groups, 3, [27], k=4, hits=True)
            assert found.size == 0 and start.tolist() == [0, 0, 0, 0] and rows.size == 0
    finally:
        p.close()


def test_refusals(layout):
    from mbgc_amd import fasta
    buf, ranges, groups, ngroups = layout
    dev, ptr = on_device(buf)
    p = fasta.FastaParser()
    try:
        ok = [5, 9, 100]
        for k in (0, 33):
            with pytest.raises(fasta.binding.SwsemError, match="screen: k = %d" % k):
                p.screen_dev(ptr, len(buf), ranges, groups, ngroups, ok, k=k)
        for bad in ([5, 9, 9], [5, 100, 9]):
            with pytest.raises(fasta.binding.SwsemError, match="screen: the keys do not ascend strictly \\(at 2\\)"):
                p.screen_dev(ptr, len(buf), ranges, groups, ngroups, bad, k=21)
        with pytest.raises(fasta.binding.SwsemError, match="screen: key 2 has bits above 2 k = 6"):
            p.screen_dev(ptr, len(buf), ranges, groups, ngroups, [5, 9, 64], k=3)
        p.screen_dev(ptr, len(buf), ranges, groups, ngroups, [5, 9, 63], k=3)                        # (63: the largest word of 6 bits)
        p.screen_dev(ptr, len(buf), ranges, groups, ngroups, [5, 9, 2 ** 64 - 1], k=32)              # (k = 32: every bit is a key's)
        with pytest.raises(fasta.binding.SwsemError, match="screen: 0 keys in one call"):
            p.screen_dev(ptr, len(buf), ranges, groups, ngroups, [], k=21)
        with pytest.raises(fasta.binding.SwsemError, match="screen: record 1 lies outside the buffer"):
            p.screen_dev(ptr, len(buf), [(0, 8), (len(buf) - 2, 3)], [0, 0], 1, ok)
        with pytest.raises(fasta.binding.SwsemError, match="screen: record 1 names group 2 of 2"):
            p.screen_dev(ptr, len(buf), [(0, 8), (8, 8)], [0, 2], 2, ok)
        # a refusal leaves the outputs as they were
        rec, grp, keys = np.asarray([(0, 8), (8, 8)], dtype=np.uint64), np.asarray([0, 2], dtype=np.uint32), np.asarray(ok, dtype=np.uint64)
        out, start, hits = np.full(4, 77, dtype=np.uint32), np.full(3, 77, dtype=np.uint64), np.full(4, 77, dtype=fasta.SCREEN_HIT_DTYPE)
        t, n, ms = C.c_uint64(77), C.c_uint64(77), C.c_double(77)
        rc = fasta._lib().mbgc_fasta_screen_dev(p.h, ptr, len(buf), rec.ctypes.data_as(C.POINTER(fasta.CrcRec)), 2, grp.ctypes.data_as(C.c_void_p), 2, 21,
                                                keys.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p), 4, start.ctypes.data_as(C.c_void_p), C.byref(t),
                                                hits.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(ms))
        assert rc == -103 and np.all(out == 77) and np.all(start == 77) and np.all(hits["pos"] == 77) and (t.value, n.value, ms.value) == (77, 77, 77.0)
    finally:
        p.close()
