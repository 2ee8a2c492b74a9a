"""The decoder's walk under --select-seq (chosenUnits with a per-contig chosen set / mergedRanges, mbgc_amd/host/
mbgc_decoder_streams.h, through the export mbgc_decoder_runs) against a restatement written the obvious way: a chosen unit
contributes its maximal runs of chosen contigs, a run never reaches over a unit's end (a row is one file's), the merged output
ranges do. Without a chosen set the export is mbgc_decoder_units. No device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P64 = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    L.mbgc_decoder_runs.argtypes = [C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int, P64, C.c_uint64, P64,
                                    P64, C.c_uint64, P64]
    L.mbgc_decoder_runs.restype = C.c_int
    L.mbgc_decoder_units.argtypes = [C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint8), C.c_int, P64, C.c_uint64, P64, P64, C.c_uint64, P64]
    L.mbgc_decoder_units.restype = C.c_int
    return L


def runs(L, g0n, seq_count, unit_sel, contig_sel, t1, cap=64):
    sc = np.asarray(seq_count, dtype=np.uint32)
    us = np.asarray(unit_sel, dtype=np.uint8)
    cs = None if contig_sel is None else np.asarray(list(contig_sel) + [0], dtype=np.uint8)
    rows, ranges = np.zeros((max(cap, 1), 3), dtype=np.uint64), np.zeros((max(cap, 1), 2), dtype=np.uint64)
    nrows, nranges = C.c_uint64(), C.c_uint64()
    r = L.mbgc_decoder_runs(g0n, sc.ctypes.data_as(C.POINTER(C.c_uint32)), len(seq_count), us.ctypes.data_as(C.POINTER(C.c_uint8)),
                            None if cs is None else cs.ctypes.data_as(C.POINTER(C.c_uint8)), int(t1), rows.ctypes.data_as(P64), cap, C.byref(nrows),
                            ranges.ctypes.data_as(P64), cap, C.byref(nranges))
    if r:
        return r, nrows.value, nranges.value
    return r, [tuple(int(v) for v in x) for x in rows[:nrows.value]], [tuple(int(v) for v in x) for x in ranges[:nranges.value]]


def restated(g0n, seq_count, unit_sel, contig_sel, t1):
    """the walk, contig by contig: (rows, ranges)"""
    rows, ranges, c = [], [], 0
    for u in range(len(seq_count) + 1):
        n = g0n if u == 0 else seq_count[u - 1]
        for k in range(c, c + n):
            if not unit_sel[u] or (u == 0 and t1) or not contig_sel[k]:
                continue
            if rows and rows[-1][0] == u and rows[-1][2] == k:
                rows[-1] = (u, rows[-1][1], k + 1)
            else:
                rows.append((u, k, k + 1))
            if ranges and ranges[-1][1] == k:
                ranges[-1] = (ranges[-1][0], k + 1)
            else:
                ranges.append((k, k + 1))
        c += n
    return rows, ranges


def test_all_none_and_alternate_contigs_of_a_unit(host):
    seq_count, g0n = [4, 3], 2                                                       # contigs: G0 0-1, target 0 2-5, target 1 6-8
    every = [1] * 9
    assert runs(host, g0n, seq_count, [1, 1, 1], every, False)[1:] == ([(0, 0, 2), (1, 2, 6), (2, 6, 9)], [(0, 9)])
    none_of_t0 = [1, 1, 0, 0, 0, 0, 1, 1, 1]
    assert runs(host, g0n, seq_count, [1, 1, 1], none_of_t0, False)[1:] == ([(0, 0, 2), (2, 6, 9)], [(0, 2), (6, 9)])
    alternate = [0, 0, 1, 0, 1, 0, 0, 0, 0]
    assert runs(host, g0n, seq_count, [1, 1, 1], alternate, False)[1:] == ([(1, 2, 3), (1, 4, 5)], [(2, 3), (4, 5)])
    # a unit that --select left out holds no row, whatever its contigs' headers say
    assert runs(host, g0n, seq_count, [1, 0, 1], every, False)[1:] == ([(0, 0, 2), (2, 6, 9)], [(0, 2), (6, 9)])


def test_a_run_across_a_units_end_is_split_per_file_and_merged_in_the_ranges(host):
    seq_count, g0n = [3, 2, 2], 1                                                    # G0 0, target 0 1-3, target 1 4-5, target 2 6-7
    sel = [0, 0, 0, 1, 1, 1, 1, 0]
    r, rows, ranges = runs(host, g0n, seq_count, [1, 1, 1, 1], sel, False)
    assert r == 0
    assert rows == [(1, 3, 4), (2, 4, 6), (3, 6, 7)]                                 # three files
    assert ranges == [(3, 7)]                                                        # one download


def test_g0_under_t1_is_no_unit(host):
    seq_count, g0n = [3, 2], 1                                                       # G0 0 (= target 0's first contig again, 1), target 0 1-3, target 1 4-5
    sel = [1, 1, 0, 1, 0, 1]
    r, rows, ranges = runs(host, g0n, seq_count, [1, 1, 1], sel, True)
    assert r == 0
    assert rows == [(1, 1, 2), (1, 3, 4), (2, 5, 6)] and ranges == [(1, 2), (3, 4), (5, 6)]
    r, rows, ranges = runs(host, g0n, seq_count, [1, 1, 1], sel, False)              # without -t1 G0's unit is a file like any other
    assert rows == [(0, 0, 1), (1, 1, 2), (1, 3, 4), (2, 5, 6)] and ranges == [(0, 2), (3, 4), (5, 6)]


def test_every_small_case_equals_the_restatement(host):
    n = 0
    for g0n, seq_count in ((0, [2, 1]), (2, [0, 3]), (1, [2, 2, 1]), (1, [1])):
        total = g0n + sum(seq_count)
        for t1 in (False, True):
            for unit_sel in itertools.product((0, 1), repeat=len(seq_count) + 1):
                for contig_sel in itertools.product((0, 1), repeat=total):
                    r, rows, ranges = runs(host, g0n, seq_count, unit_sel, contig_sel, t1)
                    assert r == 0
                    assert (rows, ranges) == restated(g0n, seq_count, unit_sel, contig_sel, t1), (g0n, seq_count, unit_sel, contig_sel, t1)
                    n += 1
    assert n > 1000


def test_without_a_chosen_set_it_is_the_walk_over_whole_units(host):
    seq_count, g0n, unit_sel = [3, 0, 2], 2, [1, 0, 1, 1]
    r, rows, ranges = runs(host, g0n, seq_count, unit_sel, None, False)
    assert r == 0 and rows == [(0, 0, 2), (2, 5, 5), (3, 5, 7)] and ranges == [(0, 2), (5, 7)]   # (the unit without a contig has its row)
    sc, us = np.asarray(seq_count, dtype=np.uint32), np.asarray(unit_sel, dtype=np.uint8)
    urows, uranges = np.zeros((8, 3), dtype=np.uint64), np.zeros((8, 2), dtype=np.uint64)
    nrows, nranges = C.c_uint64(), C.c_uint64()
    assert host.mbgc_decoder_units(g0n, sc.ctypes.data_as(C.POINTER(C.c_uint32)), 3, us.ctypes.data_as(C.POINTER(C.c_uint8)), 0, urows.ctypes.data_as(P64), 8,
                                   C.byref(nrows), uranges.ctypes.data_as(P64), 8, C.byref(nranges)) == 0
    assert [tuple(int(v) for v in x) for x in urows[:nrows.value]] == rows and [tuple(int(v) for v in x) for x in uranges[:nranges.value]] == ranges


def test_a_cap_too_small_is_reported(host):
    r, nrows, nranges = runs(host, 0, [5], [0, 1], [1, 0, 1, 0, 1], False, cap=2)
    assert r == -2 and nrows == 3 and nranges == 3
