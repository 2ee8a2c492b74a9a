"""mbgc_fasta_find_iupac_dev (k_fa_find_iupac: the scan of `mbgc-hip f --iupac`) through the ctypes mirror, on a torch buffer, against
the numpy brute force of tests/_find_iupac.py: the whole table of hits (rec, pos, pattern, mismatches) must be equal, and the referee's
own table is held non-empty for every class of case before the two are compared. One buffer of 40 KiB and thirteen records, made once:
a record over three tiles that starts at off % 16 == 5, one of 4096 + 7 bytes with a hit across its tile edge and one that ends on its
last byte, the buffer's tail, an empty record, one shorter than 8, neighbours, an overlap and a repeat; lower case, U, runs of N and
ambiguity letters in the text, some of them inside would-be hits; patterns of 8, 9, 19, 32 and 300 letters with degenerate letters in
and beside their seeds.
The kernel has no size-picked variant: the bitmap of 8 KiB is in LDS and the rows are in global memory whatever the patterns are, so
there is no threshold between two paths to name; the few-rows case and the 600-pattern case run the same code on a small and a large
row table."""
import ctypes as C

import numpy as np
import pytest

import _find
import _find_iupac as ref

pytestmark = pytest.mark.gpu
TILE = 4096
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def instance(rng, pattern):
    """a concrete sequence the pattern stands for: one base of every letter's set"""
    return bytes(ord(ref.SETS[chr(c).upper()][int(rng.integers(0, len(ref.SETS[chr(c).upper()])))]) for c in pattern)


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    """the buffer, the records, the patterns — and, filled when first asked for, the referee's table per K"""
    rng = np.random.default_rng(77)
    n = 40 * 1024
    buf = bytearray(ACGT[rng.integers(0, 4, n)].tobytes())
    # the patterns: degenerate letters inside the best window (p8: all of it is the window), beside it, and runs of N
    p8 = b"ACRYGTNA"                                                  # 2 * 2 * 4 = 16 grams
    p9 = b"NGATTACAS"                                                 # the window is letters 1..8 (2 grams), not the first (4)
    p19 = b"GTGYCAGCMGCCGCGGTAA"                                      # a primer: K = 0: a window without a code; K = 1: segments of 9
    p32 = b"ACGTNNNNACGTWSKMTTGACCRYACBDGTHV"                         # K = 3: segments of 8, the first one of exactly 256 grams
    p300 = bytearray(ACGT[rng.integers(0, 4, 300)].tobytes())
    for j in rng.choice(300, 60, replace=False):
        p300[j] = ord("RYSWKMBDHVN"[int(rng.integers(0, 11))])
    p300 = bytes(p300)
    C_ = Case()
    C_.patterns = [p8, p9, p19, p32, p300, p19.lower(), p19.replace(b"T", b"U")]      # (the same pattern three times: every index is reported)
    assert ref.expansion(p32[:8]) == 256 and ref.expansion(p9[:8]) > ref.expansion(p9[1:9])
    # the records
    a_off, a_len = 16 * 3 + 5, 2 * TILE + 200                        # three tiles: 5 + 8392 positions - 7 > 2 * 4096
    b_off, b_len = 9000, TILE + 7                                    # (9000 % 16 == 8: the tile edge is at position 4088)
    tail_off = 30000
    recs = [(a_off, a_len), (b_off, b_len), (tail_off, n - tail_off), (20000, 0), (20000, 7), (14000, 500), (14500, 500), (14250, 500), (14000, 500),
            (16000, 8), (16008, 19), (20000, 3000), (22000, 1500)]
    C_.recs = recs

    def plant(at, pattern, spoil=()):
        """an instance of `pattern` at buffer offset `at`, in mixed case with U for some T; spoil: (offset, byte) put over it afterwards"""
        s = bytearray(instance(rng, pattern))
        for j in range(len(s)):
            if s[j] == ord("T") and rng.integers(0, 3) == 0:
                s[j] = ord("U")
            if rng.integers(0, 3) == 0:
                s[j] |= 0x20
        for j, b in spoil:
            s[j] = b
        buf[at:at + len(s)] = s

    # record A: hits at its first position, over both tile edges (addresses 4096 and 8192 of the buffer's grid), at its last position
    plant(a_off, p19); plant(4096 - 150, p300); plant(8192 - 10, p32); plant(a_off + a_len - 9, p9); plant(a_off + 700, p9)
    # record B: a hit across the tile edge (its position 4088), one that ends on its last byte, would-be hits with an N, an R, a '-' inside
    edge = (b_off // 16) * 16 + TILE                                  # the address where B's second tile starts
    plant(edge - 5, p9); plant(b_off + b_len - 8, p8)
    plant(b_off + 100, p19, [(5, ord("N"))]); plant(b_off + 200, p19, [(3, ord("Y"))]); plant(b_off + 300, p19, [(0, ord("-")), (18, ord("n"))])
    plant(b_off + 400, p32, [(4, ord("N"))]); plant(b_off + 500, p32, [(2, ord("R")), (30, 0)]); plant(b_off + 1000, p300, [(7, ord("N")), (150, ord("N")), (299, ord("N"))])
    plant(b_off + 2000, p8, [(6, ord("N"))]); plant(b_off + 2100, p9, [(0, ord("N"))])
    # the tail: a hit that ends with the buffer, hits over its tile edges (30000 is a multiple of 16), runs of N, a run of one base
    plant(tail_off + TILE - 3, p8); plant(tail_off + 2 * TILE - 5, p9)
    plant(n - 300, p300); plant(n - 8 - 400, p8); plant(n - 1000, p19); plant(n - 1100, p9)
    buf[31000:31040] = b"N" * 40; buf[31500:31509] = b"n" * 9; buf[32000:32100] = b"a" * 100
    # the neighbours, the overlap and the repeat: a hit over the joint of two neighbours (no record's), one inside the overlap, short records
    plant(14500 - 9, p19); plant(14300, p19); plant(14600, p32); plant(16000, p8); plant(16008, p19)
    plant(20000, p8); plant(20500, p19); plant(21000, p300, [(20, ord("R"))]); plant(22000, p32, [(9, ord("n")), (17, ord("Y"))])
    C_.buf = bytes(buf)
    assert a_off % 16 == 5 and len(C_.buf) == n
    tables = {}

    def want(k):
        if k not in tables:
            pats = [p for p in C_.patterns if len(p) >= 8 * (k + 1)]
            for p in pats:                                           # (every segment has a window within the cap: the call is not refused)
                step = len(p) // (k + 1)
                assert all(min(ref.expansion(p[j * step + w:j * step + w + 8]) for w in range(step - 7)) <= 256 for j in range(k + 1)), (p, k)
            tables[k] = (pats, ref.brute_force(C_.buf, recs, pats, k))
        return tables[k]
    C_.want = want
    return C_


class Device:
    """the buffer on the device and a handle, for one test"""
    def __init__(self, buf, shift=0):
        import torch
        from mbgc_amd import fasta
        self.fasta = fasta
        self.dev = torch.from_numpy(np.frombuffer(b"\x00" * shift + bytes(buf), dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr, self.n = self.dev.data_ptr() + shift, len(buf)
        self.p = fasta.FastaParser()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.p.close()

    def table(self, ranges, patterns, k=0, hit_cap=None, iupac=True):
        got, _ = (self.p.find_iupac_dev if iupac else self.p.find_dev)(self.ptr, self.n, ranges, patterns, max_mismatches=k, hit_cap=hit_cap)
        assert not got["reserved"].any()
        return [(int(h["rec"]), int(h["pos"]), int(h["pattern"]), int(h["mismatches"])) for h in got]


def differ(table, want):
    return (len(table), len(want), sorted(set(table) - set(want))[:5], sorted(set(want) - set(table))[:5])


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_table_equals_the_referee(case, k):
    pats, want = case.want(k)
    assert len(pats) == (7, 5, 2, 2)[k]
    # what the case is named for stands in the referee's table: hits of every pattern, in the first ten records but the empty and the
    # short one, at a record's first and last position, over the tile edges, and — from K = 1 on — with mismatches
    assert {q for _, _, q, _ in want} == set(range(len(pats)))
    assert {r for r, _, _, _ in want} >= ({0, 1, 2, 5, 6, 7, 8, 11} if k < 2 else {0, 1, 2, 11, 12}) and not {3, 4} & {r for r, _, _, _ in want}
    assert any(p == 0 for _, p, _, _ in want) and any(p + len(pats[q]) == case.recs[r][1] for r, p, q, _ in want)
    if k:
        assert sum(1 for h in want if h[3]) >= 3
    with Device(case.buf) as d:
        table = d.table(case.recs, pats, k)
        rows, walked = d.p.find_iupac_last()
    assert table == want, differ(table, want)
    assert rows == ref.table_rows(pats, k) and walked == ref.rows_walked(case.buf, case.recs, pats, k) >= len({h[:2] for h in want})


def test_the_planted_places(case):
    """the hits the layout was made for, by name, at K = 0"""
    pats, want = case.want(0)
    p8, p9, p19, p32, p300 = range(5)
    a_off, b_off, n = case.recs[0][0], case.recs[1][0], len(case.buf)
    edge = (b_off // 16) * 16 + TILE
    for hit in [(0, 0, p19, 0), (0, 4096 - 150 - a_off, p300, 0), (0, 8192 - 10 - a_off, p32, 0), (2, TILE - 3, p8, 0), (2, 2 * TILE - 5, p9, 0), (0, case.recs[0][1] - 9, p9, 0),
                (1, edge - 5 - b_off, p9, 0), (1, case.recs[1][1] - 8, p8, 0), (2, n - 300 - 30000, p300, 0),
                (9, 0, p8, 0), (10, 0, p19, 0), (7, 50, p19, 0), (5, 300, p19, 0), (8, 300, p19, 0), (0, 0, 5, 0), (0, 0, 6, 0)]:
        assert hit in want, hit
    # ... and the would-be hits the text's N, R, Y and '-' spoil: not at K = 0; at K = 1 with one mismatch where one byte was spoiled
    for r, p, q in [(1, 100, p19), (1, 200, p19), (1, 300, p19), (1, 400, p32), (1, 1000, p300), (1, 2000, p8), (1, 2100, p9), (11, 1000, p300)]:
        assert not any(h[:3] == (r, p, q) for h in want), (r, p, q)
    pats1, want1 = case.want(1)
    assert (1, 100, pats1.index(pats[p19]), 1) in want1 and (1, 200, pats1.index(pats[p19]), 1) in want1 and (11, 1000, pats1.index(pats[p300]), 1) in want1
    assert not any(h[:2] == (1, 300) for h in want1)                 # (two spoiled bytes)
    # the hit over the joint of the two neighbours is no record's but the overlapping one's
    assert {r for r, p, q, _ in want if q == p19 and case.recs[r][0] + p == 14500 - 9} == {7}


def test_a_buffer_at_any_alignment_and_a_record_that_ends_with_it(case):
    pats, want = case.want(0)
    with Device(case.buf, shift=3) as d:
        table = d.table(case.recs, pats, 0)
    assert table == want, differ(table, want)
    assert any(case.recs[r][0] + p + len(pats[q]) == len(case.buf) for r, p, q, _ in want)


def test_six_hundred_patterns_with_expansions(case):
    """a row table of thousands of rows; every pattern is cut from the text and widened, so every one has a hit; K = 1"""
    rng = np.random.default_rng(600)
    text = case.buf[:12000]                                          # (A, C, G, T only up to record A's plants: the cuts avoid those)
    pats = []
    while len(pats) < 600:
        at = int(rng.integers(100, 4000))
        q = text[at:at + 20].upper()
        if not set(q) <= set(b"ACGT"):
            continue
        q = ref.widen(rng, q, rng.choice(20, 5, replace=False), keep=True)
        pats.append(ref.widen(rng, q, rng.choice(20, 1), keep=False) if len(pats) % 3 == 0 else q)
    ranges = [(0, 12000), (37, 5000)]
    want = ref.brute_force(text, ranges, pats, 1)
    assert {q for _, _, q, _ in want} == set(range(600)) and sum(1 for h in want if h[3] == 1) >= 150
    with Device(text) as d:
        table = d.table(ranges, pats, 1)
        rows, walked = d.p.find_iupac_last()
    assert table == want, differ(table, want)
    assert rows == ref.table_rows(pats, 1) > 5000 and walked == ref.rows_walked(text, ranges, pats, 1) >= 600
    few = pats[:2]
    with Device(text) as d:
        assert d.table(ranges, few, 1) == ref.brute_force(text, ranges, few, 1)
        assert d.p.find_iupac_last()[0] == ref.table_rows(few, 1) < 200


def test_a_hit_buffer_of_one_row(case):
    pats, want = case.want(0)
    assert len(want) > 20
    with Device(case.buf) as d:
        with pytest.raises(d.fasta.HitsTooMany) as e:
            d.table(case.recs, pats, 0, hit_cap=1)
        assert e.value.needed == len(want)
        assert d.table(case.recs, pats, 0, hit_cap=e.value.needed) == want
        # the raw call: -104, the exact count, the caller's rows as they were
        rows = np.asarray(case.recs, dtype=np.uint64)
        hits = np.full(1, 0xAB, dtype=d.fasta.HIT_DTYPE)
        before = hits.tobytes()
        blob, off = b"".join(pats), np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.uint64)
        cnt = C.c_uint64(0)
        rc = d.fasta._lib().mbgc_fasta_find_iupac_dev(d.p.h, d.ptr, d.n, rows.ctypes.data_as(C.POINTER(d.fasta.CrcRec)), len(case.recs), blob,
                                                      off.ctypes.data_as(C.POINTER(C.c_uint64)), len(pats), 0, hits.ctypes.data_as(C.c_void_p), 1, C.byref(cnt), None)
        assert rc == -104 and cnt.value == len(want) and hits.tobytes() == before


REFUSED = {
    "four mismatches": ([b"ACGT" * 10], 4, [(0, 64)]),
    "a pattern of 7 letters": ([b"ACGTACG"], 0, [(0, 64)]),
    "a pattern too short for two mismatches": ([b"ACGTRYACGTACGTACGTACGTA"], 2, [(0, 64)]),
    "a pattern of 65536 letters": ([b"ACGT" * 16384], 0, [(0, 64)]),
    "a letter outside the table": ([b"ACGTACGTACGT", b"ACGTEACGTACGT"], 0, [(0, 64)]),
    "a byte that is no letter": ([b"ACGTACGT-ACGT"], 0, [(0, 64)]),
    "a window of 1024 grams": ([b"ACGTACGTACGT", b"ACNNNNNTG"], 0, [(0, 64)]),
    "a window past the cap in the second segment": ([b"ACGTACGTACGTNNNNNNNN"], 1, [(0, 64)]),
    "a record past the buffer": ([b"ACGTACGT"], 0, [(0, 8), (60, 5)]),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_calls_launch_nothing(name):
    """-103 and a message; the count, the rows and — no event was recorded — the kernel's time are as they were"""
    pats, k, ranges = REFUSED[name]
    text = b"ACGTACGTACGTACGTACGTACGTACGTACGT" * 2
    with Device(text) as d:
        with pytest.raises(d.fasta.binding.SwsemError, match="find-iupac: "):
            d.table(ranges, pats, k)
        rows = np.asarray(ranges, dtype=np.uint64)
        hits = np.full(4, 0xAB, dtype=d.fasta.HIT_DTYPE)
        before = hits.tobytes()
        n, ms = C.c_uint64(777), C.c_double(-1.0)
        blob, off = b"".join(pats), np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.uint64)
        rc = d.fasta._lib().mbgc_fasta_find_iupac_dev(d.p.h, d.ptr, d.n, rows.ctypes.data_as(C.POINTER(d.fasta.CrcRec)), len(ranges), blob,
                                                      off.ctypes.data_as(C.POINTER(C.c_uint64)), len(pats), k, hits.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(ms))
        assert rc == -103 and n.value == 777 and hits.tobytes() == before and ms.value == 0.0
        message = d.fasta._lib().mbgc_fasta_last_error().decode()
    if "window" in name:                                             # the message names the pattern, the segment and what its best window stands for
        want = {"a window of 1024 grams": "pattern 1, segment 0 (letters 1 to 9): its best window of 8 letters stands for 1024 sequences",
                "a window past the cap in the second segment": "pattern 0, segment 1 (letters 11 to 20): its best window of 8 letters stands for 4096 sequences"}[name]
        assert want in message, message


def test_exactly_256_grams_are_accepted():
    text = b"TTTTACGGTCGTTTTT" + b"ACAAAAGT" + b"ACNNNNGT"
    with Device(text) as d:
        table = d.table([(0, len(text))], [b"ACNNNNGT"], 0)
        assert d.p.find_iupac_last()[0] == 256
    assert table == ref.brute_force(text, [(0, len(text))], [b"ACNNNNGT"], 0) == [(0, 4, 0, 0), (0, 16, 0, 0)]


def test_without_degenerate_letters_and_without_n_the_hits_are_the_literal_searchs(case):
    """patterns of A, C, G, T over a text of acgtACGT: mbgc_fasta_find_dev, mbgc_fasta_find_iupac_dev and both referees agree"""
    rng = np.random.default_rng(5)
    text = bytearray(ACGT[rng.integers(0, 4, 3 * TILE)].tobytes())
    for j in rng.choice(len(text), 2000, replace=False):
        text[j] |= 0x20
    text[5000:5200] = b"A" * 200
    text = bytes(text)
    pats = [text[100:124].upper(), text[4090:4122].lower(), b"A" * 24, text[8000:8032].upper(), text[12000:12040].upper()]
    sub = bytearray(pats[3]); sub[5] = ord("A") if sub[5] != ord("A") else ord("C"); sub[20] = ord("G") if sub[20] != ord("G") else ord("T")
    pats.append(bytes(sub))
    ranges = [(0, len(text)), (4000, 300), (7, 9000)]
    for k in (0, 2):
        want = ref.brute_force(text, ranges, pats, k)
        assert want == _find.brute_force(text, ranges, pats, k) and len(want) > 200 and (k == 0 or any(h[3] == 2 for h in want))
        with Device(text) as d:
            assert d.table(ranges, pats, k) == want
            assert d.table(ranges, pats, k, iupac=False) == want
