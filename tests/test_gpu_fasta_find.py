"""mbgc_fasta_find_dev (k_fa_find: the scan of `mbgc-hip f`) through the ctypes mirror, on torch buffers, against the numpy brute force
of tests/_find.py: the whole table of hits (rec, pos, pattern, mismatches) must be equal, and the referee's own table is held
non-empty for every class of case before the two are compared. Shapes: the smallest at which the kernel can go wrong — hits at every
start around the edges of its tiles of fasta.FIND_TILE positions, a pattern over three tiles, records at their own edges, next to each
other, listed twice and out of order, repeats, both cases, every seed as the only exact one at K = 1, 2, 3, a table too large for
LDS, the retry of a hit buffer that is too small, and the calls that are refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import _find

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def rand(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(0, alphabet.size, n)].tobytes()


def search(buf, ranges, patterns, k=0, shift=0, hit_cap=None, least=1):
    """find_dev over `buf` on the device against the brute force -> the table; the referee must hold at least `least` hits.
    shift: the buffer starts that many bytes into its allocation (any alignment of the pointer)"""
    import torch
    from mbgc_amd import fasta
    want = _find.brute_force(buf, ranges, patterns, k)
    assert len(want) >= least, "the referee finds %d hits: the case does not test what it is named for" % len(want)
    dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf) + (b"" if buf else b"\0"), dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        got, ms = p.find_dev(dev.data_ptr() + shift, len(buf), ranges, patterns, max_mismatches=k, hit_cap=hit_cap)
    finally:
        p.close()
    table = [(int(h["rec"]), int(h["pos"]), int(h["pattern"]), int(h["mismatches"])) for h in got]
    assert table == want, (len(table), len(want), sorted(set(table) - set(want))[:5], sorted(set(want) - set(table))[:5])
    assert not got["reserved"].any()
    return table


@pytest.mark.parametrize("L", [8, 9, 63, 64, 65])
@pytest.mark.parametrize("shift", [0, 5])
def test_a_hit_at_every_start_around_the_tiles_edges(L, shift):
    """one record of 3 T + 5 bytes per planted start (a copy each, 16-byte strides, so that with shift 0 every copy's tiles are cut at its
    positions T and 2 T): the pattern at every start of [T - L, T + 1] and [2 T - L, 2 T + 1]"""
    from mbgc_amd import fasta
    T = fasta.FIND_TILE
    rng = np.random.default_rng(L)
    n, stride = 3 * T + 5, (3 * T + 5 + 15) // 16 * 16
    base, pat = bytearray(rand(rng, n)), rand(rng, L)
    starts = list(range(T - L, T + 2)) + list(range(2 * T - L, 2 * T + 2))
    buf, ranges = bytearray(), []
    for s in starts:
        copy = bytearray(base)
        copy[s:s + L] = pat
        ranges.append((len(buf), n))
        buf += copy + b"N" * (stride - n)
    table = search(bytes(buf), ranges, [pat], shift=shift, least=len(starts))
    assert {(r, s) for r, s in enumerate(starts)} <= {(r, p) for r, p, _, _ in table}


def test_a_pattern_over_three_tiles():
    from mbgc_amd import fasta
    T = fasta.FIND_TILE
    rng = np.random.default_rng(3)
    n, L = 3 * T + 5, 2 * T + 3
    pat = rand(rng, L)
    buf, ranges, starts = bytearray(), [], [0, 5, T - 3, T, T + 1, n - L]
    for s in starts:
        copy = bytearray(rand(rng, n))
        copy[s:s + L] = pat
        ranges.append((len(buf), n))
        buf += copy + b"N" * 11
    table = search(bytes(buf), ranges, [pat, pat[:64], pat[-9:]], least=3 * len(starts))
    assert [(r, p) for r, p, q, _ in table if q == 0] == list(enumerate(starts))


def test_the_edges_of_records():
    rng = np.random.default_rng(5)
    pat = b"GATTACAGATTACA"
    body = rand(rng, 40)
    a = pat + body + pat                                             # a hit at position 0 and one that ends on the last byte
    short = pat[:-1]                                                 # the pattern is one byte longer than the record
    left, right = rand(rng, 30) + pat[:6], pat[6:] + rand(rng, 30)   # the pattern stands over the joint of two neighbours only
    buf = a + short + left + right + b"ACGTACGTAC"
    ranges = [(0, len(a)), (len(a), len(short)), (len(a) + len(short), len(left)), (len(a) + len(short) + len(left), len(right))]
    end = len(a) + len(short) + len(left) + len(right)
    ranges += [(end, 0), (end, 1), (end, 7), (end, 8)]               # records of 0, 1, 7 and 8 bytes ("ACGTACGT")
    ranges += [(0, len(a))]                                          # the first record once more
    table = search(buf, ranges, [pat, b"ACGTACGT"], least=5)
    assert [(r, p) for r, p, q, _ in table if q == 0] == [(0, 0), (0, len(a) - len(pat)), (8, 0), (8, len(a) - len(pat))]
    assert (7, 0, 1, 0) in table and not any(r in (1, 2, 3, 4, 5, 6) for r, _, _, _ in table)
    # the same records in descending offset order, and the whole buffer as one record: the joint is inside it
    flipped = search(buf, ranges[:8][::-1], [pat, b"ACGTACGT"], least=3)
    assert [(r, p) for r, p, q, _ in flipped if q == 0] == [(7, 0), (7, len(a) - len(pat))]
    whole = search(buf, [(0, len(buf))], [pat], least=3)
    assert (0, len(a) + len(short) + len(left) - 6, 0, 0) in whole
    # the buffer ends with the last record's last byte, at any alignment of its first
    search(buf[:end + 8], ranges[:8], [b"ACGTACGT"], shift=3, least=1)


def test_repeats_prefixes_shared_grams_and_a_pattern_given_twice():
    rng = np.random.default_rng(7)
    run = rand(rng, 50) + b"A" * 200 + rand(rng, 50, np.frombuffer(b"CGT", dtype=np.uint8))
    table = search(run, [(0, len(run))], [b"A" * 8], least=193)
    assert len([h for h in table if 50 <= h[1] <= 242]) == 193
    text = rand(rng, 3000)
    long, other = text[1000:1040], text[1000:1008] + b"TTTTTTTT"     # `other` shares its first 8 bytes with `long`
    text = text[:2000] + other + text[2016:]
    pats = [long, long[:20], other, long, long[:8]]                  # a prefix of another, a shared gram, the same pattern twice
    table = search(text, [(0, len(text)), (900, 300)], pats, least=9)
    assert {(0, 1000, q, 0) for q in (0, 1, 3, 4)} <= set(table) and (0, 2000, 2, 0) in table and (1, 100, 3, 0) in table


def test_letters_are_compared_without_case_and_nothing_else_is_folded():
    text = b"ttgac" + b"gattacag" + b"NNNNnnnnNNNN" + b"acgt" + b"GATTACAGATTACA".lower() + b"[[[[[[[[{{{{{{{{@@@@@@@@````````"
    table = search(text, [(0, len(text))], [b"GATTACAG", b"gattacag", b"NNNNNNNN", b"nnnnnnnn"], least=6)
    assert [(p, q) for _, p, q, _ in table if q < 2] == [(5, 0), (5, 1), (29, 0), (29, 1)]
    assert [p for _, p, q, _ in table if q == 2] == [13, 14, 15, 16, 17] == [p for _, p, q, _ in table if q == 3]
    # an upper-case text against a lower-case pattern; '[' is no 'K', '{' no '[', '@' no '`' (0x20 apart, and no letters)
    assert search(text.upper().replace(b"{", b"["), [(0, len(text))], [b"gattacag"], least=2)
    assert _find.brute_force(b"[[[[[[[[{{{{{{{{@@@@@@@@````````", [(0, 32)], [b"KKKKKKKK"]) == []


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_mismatches_with_every_seed_as_the_only_exact_one(K, extra):
    rng = np.random.default_rng(10 * K + extra)
    L = 8 * (K + 1) + extra
    step = L // (K + 1)
    pat = rand(rng, L)
    other = {65: 67, 67: 71, 71: 84, 84: 65}                         # A -> C -> G -> T -> A: never the same base

    def with_mismatches(at):
        copy = bytearray(pat)
        for j in at:
            copy[j] = other[copy[j]]
        return bytes(copy)

    pieces = [with_mismatches([j * step + (e + j) % 8 for j in range(K + 1) if j != e]) for e in range(K + 1)]   # seed e alone is exact: K mismatches
    pieces.append(with_mismatches([0] + [L - 1] * (K > 1)))          # on the first byte (and, from K = 2 on, the last one)
    pieces.append(with_mismatches([L - 1]))
    pieces.append(pat)                                               # every seed exact: once, with 0 mismatches
    too_many = with_mismatches([j * step + 3 for j in range(K + 1)])  # K + 1: one in every seed
    buf, ranges = bytearray(), []
    for piece in pieces + [too_many]:
        ranges.append((len(buf), 7 + L + 9))
        buf += rand(rng, 7, np.frombuffer(b"N", dtype=np.uint8)) + piece + b"N" * 9 + b"N" * int(rng.integers(0, 5))
    table = search(bytes(buf), ranges, [pat], k=K, least=len(pieces))
    assert [(r, p, d) for r, p, _, d in table] == [(e, 7, K) for e in range(K + 1)] + [(K + 1, 7, min(K, 2)), (K + 2, 7, 1), (K + 3, 7, 0)]


def test_a_run_of_one_base_under_one_mismatch():
    text = b"C" * 9 + b"A" * 120 + b"C" * 9
    table = search(text, [(0, len(text))], [b"A" * 16, b"A" * 21], k=1, least=100)
    assert [p for _, p, q, _ in table if q == 0] == list(range(8, 115)) and [p for _, p, q, _ in table if q == 1] == list(range(8, 110))


def test_twenty_thousand_patterns():
    """a table far beyond LDS: it is read from global memory; 50 of the patterns stand in the text"""
    rng = np.random.default_rng(20)
    text = bytearray(rand(rng, 65536))
    pats = [rand(rng, 20) for _ in range(20000)]
    planted = rng.choice(20000, 50, replace=False)
    for i, q in enumerate(planted):
        at = 1000 * i + int(rng.integers(0, 900))
        text[at:at + 20] = pats[q]
    table = search(bytes(text), [(0, 65536)], pats, least=50)
    assert set(planted.tolist()) <= {q for _, _, q, _ in table}


def test_a_hit_buffer_that_is_too_small():
    from mbgc_amd import fasta
    rng = np.random.default_rng(30)
    text = rand(rng, 500) + b"ACGTACGT" * 40 + rand(rng, 500)
    full = search(text, [(0, len(text))], [b"ACGTACGT", b"GTACGTAC"], least=70)
    with pytest.raises(fasta.HitsTooMany) as e:
        search(text, [(0, len(text))], [b"ACGTACGT", b"GTACGTAC"], hit_cap=len(full) - 1)
    assert e.value.needed == len(full)
    assert search(text, [(0, len(text))], [b"ACGTACGT", b"GTACGTAC"], hit_cap=e.value.needed) == full
    assert search(text, [(0, len(text))], [b"ACGTACGT", b"GTACGTAC"], hit_cap=None) == full      # (4096 rows at first: no retry here)
    many = b"A" * 6000                                               # more hits than the mirror's first buffer: it asks again by itself
    assert len(search(many, [(0, 6000)], [b"A" * 8], least=5993)) == 5993


@pytest.mark.parametrize("case", ["a pattern of 7 bytes", "a digit in a pattern", "four mismatches", "a record past the buffer", "too short for two mismatches"])
def test_refused_calls_launch_nothing(case):
    """-103 and a message; the count, the rows and — no event was recorded — the kernel's time are as they were"""
    import torch
    from mbgc_amd import fasta
    text = b"ACGTACGTACGTACGTACGTACGTACGTACGT"
    pattern, k, ranges = {"a pattern of 7 bytes": (b"ACGTACG", 0, [(0, 32)]), "a digit in a pattern": (b"ACGT4CGTA", 0, [(0, 32)]),
                          "four mismatches": (b"ACGT" * 10, 4, [(0, 32)]), "a record past the buffer": (b"ACGTACGT", 0, [(0, 8), (30, 3)]),
                          "too short for two mismatches": (b"ACGT" * 5 + b"ACG", 2, [(0, 32)])}[case]
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        with pytest.raises(fasta.binding.SwsemError, match="find: "):
            p.find_dev(dev.data_ptr(), len(text), ranges, [pattern], max_mismatches=k)
        rows = np.asarray(ranges, dtype=np.uint64)
        hits = np.full(4, 0xAB, dtype=fasta.HIT_DTYPE)
        before = hits.tobytes()
        n, ms = C.c_uint64(777), C.c_double(-1.0)
        off = np.array([0, len(pattern)], dtype=np.uint64)
        rc = fasta._lib().mbgc_fasta_find_dev(p.h, dev.data_ptr(), len(text), rows.ctypes.data_as(C.POINTER(fasta.CrcRec)), len(ranges), pattern,
                                              off.ctypes.data_as(C.POINTER(C.c_uint64)), 1, k, hits.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(ms))
        assert rc == -103 and n.value == 777 and hits.tobytes() == before and ms.value == 0.0
    finally:
        p.close()
