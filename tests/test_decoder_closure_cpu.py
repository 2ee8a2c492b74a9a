"""The provenance table of `mbgc-hip d --select` (mbgc_amd/host/mbgc_decoder.cpp: whose bytes lie where in the reference buffer,
at every moment of the load schedule) through mbgc_decoder_provenance, against an owner map this test builds from the schedule
alone by replaying the segments byte by byte. No device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP, FROM_REF, NONE = -1, -2, -1
FIRST = 2                                                      # contigs 0 and 1 are the initial reference's: nobody's


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    P = C.POINTER(C.c_uint64)
    I = C.POINTER(C.c_int64)
    L.mbgc_decoder_provenance.argtypes = [I, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, I, C.c_uint64, P]
    L.mbgc_decoder_schedule.argtypes = [P, P, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, P, P, C.c_int, C.c_int, I, C.c_uint64, P]
    return L


def owners(host, segs, total, n_before, p0, p1):
    """-> per physical position of [p0, p1): the owner mbgc_decoder_provenance reports, NONE where it reports none"""
    a = np.ascontiguousarray(np.array(segs, dtype=np.int64).reshape(-1, 5))
    out = np.zeros((4 * len(segs) + 8, 3), dtype=np.int64)
    n = C.c_uint64()
    r = host.mbgc_decoder_provenance(a.ctypes.data_as(C.POINTER(C.c_int64)), len(segs), total, FIRST, n_before, p0, p1,
                                     out.ctypes.data_as(C.POINTER(C.c_int64)), len(out), C.byref(n))
    assert r == 0, r
    got = np.full(max(p1 - p0, 0), NONE, dtype=np.int64)
    for a0, b0, o in out[:n.value]:
        assert p0 <= a0 < b0 <= p1 and o >= 0, (a0, b0, o)
        assert (got[a0 - p0:b0 - p0] == NONE).all()            # (no position is reported twice)
        got[a0 - p0:b0 - p0] = o
    return got


def replay(segs, total, n_before, strict):
    """the owner of every physical byte after the first n_before segments, byte by byte. strict: a separator written over the last
    loaded byte takes the byte from its owner (what the buffer really holds); not strict: it is ignored (the superset rule)"""
    own = np.full(total, NONE, dtype=np.int64)
    pos = 1
    for contig, offset, length, ref_pos, rc in segs[:n_before]:
        if contig == SEP and length == 1 and ref_pos == pos - 1:
            if strict:
                own[ref_pos] = NONE
            continue
        if contig == FROM_REF:
            src = own[offset:offset + length].copy()
            vals = src[::-1] if rc else src
        else:
            vals = np.full(length, contig - FIRST if contig >= FIRST else NONE, dtype=np.int64)
        for i in range(length):
            own[ref_pos + i] = vals[i]
        pos = ref_pos + length
    return own


def check_everywhere(host, segs, total, step=1):
    """every moment of the schedule, every range on a grid: the reported owners are the replayed ones"""
    for n_before in range(len(segs) + 1):
        want = replay(segs, total, n_before, False)
        real = replay(segs, total, n_before, True)
        assert ((real == NONE) | (real == want)).all()         # (what is read is within what is reported)
        for p0 in range(0, total, step):
            for p1 in range(p0 + 1, total + 3, step):
                got = owners(host, segs, total, n_before, p0, p1)
                exp = want[p0:min(p1, total)]
                assert (got[:len(exp)] == exp).all(), (n_before, p0, p1, got.tolist(), exp.tolist())
                assert (got[len(exp):] == NONE).all()          # (nothing lies beyond the buffer)


class Loader:
    """a hand-built schedule: the loader as MBGC_Decoder::loadRef moves it, without a lock position"""

    def __init__(self, total):
        self.total, self.pos, self.laps, self.segs = total, 1, 0, []

    def load(self, contig, length):
        left, at = length, 0
        while left:
            if self.pos == self.total:
                self.laps += 1
                self.pos = 1
            n = min(left, self.total - self.pos)
            self.segs.append([contig, at, n, self.pos, 0])
            self.pos += n
            at += n
            left -= n
        return self


def test_before_the_first_lap(host):
    ld = Loader(100).load(0, 20).load(3, 30)
    got = owners(host, ld.segs, 100, 2, 10, 80)                # the loader stands at 51
    assert (got[:11] == NONE).all() and (got[11:41] == 1).all()  # G0 is nobody's, contig 3 is owner 1
    assert (got[41:] == NONE).all()                            # above the loader: never written, no owner
    check_everywhere(host, ld.segs, 100, step=7)


@pytest.mark.parametrize("laps", [1, 2])
def test_after_laps_the_latest_owner_is_reported(host, laps):
    total = 64
    ld = Loader(total).load(0, 10)
    c = FIRST
    while ld.laps < laps or ld.pos < 30:
        ld.load(c, 9 + c % 5)
        c += 1
    assert ld.laps == laps
    want = replay(ld.segs, total, len(ld.segs), True)
    got = owners(host, ld.segs, total, len(ld.segs), 0, total)
    assert (got == want).all()
    # above the loader the bytes are the lap before's — not what lay there a lap earlier still
    above = got[ld.pos + 2]
    assert above != NONE
    if laps == 2:
        older = [s for s in ld.segs if s[3] <= ld.pos + 2 < s[3] + s[2]]
        assert len(older) >= 2 and above == older[-1][0] - FIRST and above != older[-2][0] - FIRST
    assert got[0] == NONE                                      # (position 0 is never loaded)
    check_everywhere(host, ld.segs, total, step=5)


def test_range_straddles_the_loader_position(host):
    total = 50
    ld = Loader(total).load(0, 5).load(2, 30).load(3, 14).load(4, 20)   # contig 4 wraps: [49 ..], then [1, 20)
    assert ld.laps == 1 and ld.pos == 21
    got = owners(host, ld.segs, total, len(ld.segs), 15, 30)
    assert (got[:6] == 2).all() and (got[6:] == 0).all()       # below the loader contig 4 (this lap), from it on contig 2 (the lap before)
    check_everywhere(host, ld.segs, total, step=3)


def test_range_spans_three_segments(host):
    ld = Loader(80).load(0, 9).load(2, 10).load(3, 10).load(4, 10).load(5, 10)
    got = owners(host, ld.segs, 80, len(ld.segs), 15, 45)
    assert got.tolist() == [0] * 5 + [1] * 10 + [2] * 10 + [3] * 5
    check_everywhere(host, ld.segs, 80, step=6)


def schedule(host, total, lazy, individually, lock, ref_pos, first, lengths, factor=255):
    pos, laps, n = C.c_uint64(ref_pos), C.c_uint64(0), C.c_uint64()
    ln = (C.c_uint64 * len(lengths))(*lengths)
    un = (C.c_uint64 * len(lengths))(*lengths)                 # nothing matched: every contig is loaded
    segs = np.zeros((64, 5), dtype=np.int64)
    r = host.mbgc_decoder_schedule(C.byref(pos), C.byref(laps), total, lazy, 1, individually, lock, first, len(lengths), ln, un, factor, factor,
                                   segs.ctypes.data_as(C.POINTER(C.c_int64)), len(segs), C.byref(n))
    assert r == 0
    return segs[:n.value].tolist(), pos.value


@pytest.mark.parametrize("wraps", [False, True])
def test_from_ref_reverse_complement_is_resolved_mirrored(host, wraps):
    """the per-target reverse complement (decodeTarget :608-616) as the scheduler itself writes it: FROM_REF segments"""
    total = 120
    pre = Loader(total).load(0, 10)
    if wraps:
        pre.load(2, 85)                                        # the target starts at 96 and goes round the end
    segs, _ = schedule(host, total, 0, 0, 60 if wraps else total, pre.pos, 5, [9, 12, 7])
    segs = pre.segs + segs
    assert any(s[0] == FROM_REF and s[4] for s in segs)
    start = pre.pos
    want = replay(segs, total, len(segs), True)
    got = owners(host, segs, total, len(segs), 0, total)
    assert (got == want).all()
    if not wraps:
        # forward: contigs 5, 6, 7 = owners 3, 4, 5; behind them their reverse complement as one text: 5, 4, 3
        assert got[start:start + 56].tolist() == [3] * 9 + [4] * 12 + [5] * 7 + [5] * 7 + [4] * 12 + [3] * 9
    else:
        assert {3, 4, 5} <= set(got.tolist()) and sum(1 for s in segs if s[0] == FROM_REF) >= 2
    check_everywhere(host, segs, total, step=7)


def test_separator_inside_a_segment_keeps_the_owner(host):
    """lazy mode: a load that reaches the lock position gets a separator written over its last byte"""
    total = 100
    pre = Loader(total).load(0, 10)
    segs, pos = schedule(host, total, 1, 1, 40, pre.pos, 2, [20, 30])
    segs = pre.segs + segs
    over = [s for s in segs if s[0] == SEP and s[3] == 39]
    assert over and pos == 40
    got = owners(host, segs, total, len(segs), 30, 45)
    real = replay(segs, total, len(segs), True)
    assert real[39] == NONE and got[9] != NONE                  # the byte is a separator now; its segment's owner is still reported
    assert got[9] == got[8]
    check_everywhere(host, segs, total, step=7)
