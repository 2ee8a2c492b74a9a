"""The decoder's one walk over the chosen units (chosenUnits / mergedRanges, mbgc_amd/host/mbgc_decoder_streams.h) against a
straight restatement of the three loops MBGC_Decoder::decode held before they became one: the output ranges of the sequence
files, the resident units of `mbgc-hip r` and the units of `d --fasta` / `v`. No device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    P = C.POINTER(C.c_uint64)
    L.mbgc_decoder_units.argtypes = [C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8), C.c_int, P, C.c_uint64, P, P, C.c_uint64, P]
    L.mbgc_decoder_units.restype = C.c_int
    return L


def units(L, g0n, seq_count, unit_sel, t1, cap=None):
    T = len(seq_count)
    cap = T + 1 if cap is None else cap
    sc = np.asarray(seq_count, dtype=np.uint32)
    us = np.asarray(unit_sel, dtype=np.uint8)
    rows = np.zeros((max(cap, 1), 3), dtype=np.uint64)
    ranges = np.zeros((max(cap, 1), 2), dtype=np.uint64)
    nrows, nranges = C.c_uint64(), C.c_uint64()
    P = C.POINTER(C.c_uint64)
    r = L.mbgc_decoder_units(g0n, sc.ctypes.data_as(C.POINTER(C.c_uint32)), T, us.ctypes.data_as(C.POINTER(C.c_uint8)), int(t1),
                             rows.ctypes.data_as(P), cap, C.byref(nrows), ranges.ctypes.data_as(P), cap, C.byref(nranges))
    return r, [tuple(int(v) for v in x) for x in rows[:nrows.value]] if r == 0 else nrows.value, \
        [tuple(int(v) for v in x) for x in ranges[:nranges.value]] if r == 0 else nranges.value


# ---- the three loops as they stood, one by one
def out_ranges(g0n, seq_count, unit_sel, t1):
    """the sequence files: the chosen units' contigs as merged ranges, clipped at outFrom"""
    out_from = g0n if t1 else 0
    ranges, c = [], 0
    for u in range(len(seq_count) + 1):
        n = g0n if u == 0 else seq_count[u - 1]
        if unit_sel[u] and c + n > out_from and n:
            frm = max(c, out_from)
            if ranges and ranges[-1][1] == frm:
                ranges[-1] = (ranges[-1][0], c + n)
            else:
                ranges.append((frm, c + n))
        c += n
    return ranges


def resident_units(g0n, seq_count, unit_sel, t1):
    """`mbgc-hip r`: the units handed over"""
    rows, c = [], 0
    for u in range(len(seq_count) + 1):
        n = g0n if u == 0 else seq_count[u - 1]
        c0 = c
        c += n
        if (u == 0 and t1) or not unit_sel[u]:
            continue
        rows.append((u, c0, c0 + n))
    return rows


def fasta_units(g0n, seq_count, unit_sel, t1):
    """`d --fasta` / `v`: the units formatted"""
    rows, c = [], 0
    for u in range(len(seq_count) + 1):
        n = g0n if u == 0 else seq_count[u - 1]
        x = (u, c, c + n)
        c += n
        if u == 0 and t1:
            continue
        if not unit_sel[u]:
            continue
        rows.append(x)
    return rows


def cases():
    for T in (1, 2, 3, 4):
        counts = [(3, 0, 2, 1)[:T], (0, 1, 0, 0)[:T], (1, 1, 1, 1)[:T]]
        for seq_count in counts:
            for g0n in (0, 2):
                for t1 in (False, True):
                    if T <= 3:
                        sels = itertools.product((0, 1), repeat=T + 1)
                    else:
                        sels = [(1,) * 5, (0, 1, 0, 1, 1), (1, 0, 0, 0, 1), (0, 0, 1, 1, 0), (0,) * 5]
                    for sel in sels:
                        yield g0n, list(seq_count), list(sel), t1


def test_the_walk_is_the_three_loops(host):
    n = 0
    for g0n, seq_count, sel, t1 in cases():
        r, rows, ranges = units(host, g0n, seq_count, sel, t1)
        what = "g0n=%d seqCount=%s unitSel=%s t1=%s" % (g0n, seq_count, sel, t1)
        assert r == 0, what
        assert rows == resident_units(g0n, seq_count, sel, t1), what
        assert rows == fasta_units(g0n, seq_count, sel, t1), what
        assert ranges == out_ranges(g0n, seq_count, sel, t1), what
        # what the sequence files count per unit (.seqCounts) is the walk's too
        counts = ([g0n] if not t1 and sel[0] else []) + [seq_count[t] for t in range(len(seq_count)) if sel[t + 1]]
        assert [c1 - c0 for _, c0, c1 in rows] == counts, what
        n += 1
    assert n > 300


def test_the_cases_cover_what_they_should():
    seen = list(cases())
    assert {len(c[1]) for c in seen} == {1, 2, 3, 4}
    assert any(0 in c[1] for c in seen) and {c[0] for c in seen} == {0, 2} and {c[3] for c in seen} == {False, True}
    for T in (1, 2, 3):
        for t1 in (False, True):
            assert {tuple(c[2]) for c in seen if len(c[1]) == T and c[3] == t1 and c[0] == 2} == set(itertools.product((0, 1), repeat=T + 1))


def test_a_cap_too_small_is_reported(host):
    r, nrows, nranges = units(host, 2, [1, 0, 2], [1, 0, 1, 1], False, cap=1)
    assert r == -2 and nrows == 3 and nranges == 2
