"""The -m3 reverse-complement pass over the literal stream: the C restatement
(oracle/rcmatch_oracle.c) against the reference's own SimpleSequenceMatcher::rcMatchSequence / CopMEMMatcher compiled into
oracle/_ref (build container), and the decoder's inverse as a size-independent property."""
import numpy as np
import pytest

import _orc
import _rcdata

CASES = _rcdata.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_and_rewrite_equal_reference(refh, name):
    s = CASES[name]
    if s.size >= 55:
        got, params, _ = _orc.rc_find_matches(s)
        want = refh.rc_find_matches(s)
        assert params[:3] == (40, 5, 3)                               # L = 55 -> K = 40, k1 = 5, k2 = 3
        assert got.shape == want.shape and np.array_equal(got, want), name
    a = _orc.rc_match_sequence(s)
    b = refh.rc_match_sequence(s)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], name
    if name not in ("tiny",):
        assert (len(a[1]) > 0) == (name != "short" or len(a[1]) > 0)


@pytest.mark.parametrize("target,min_len", [(55, 0xFFFFFFFF), (32, 0xFFFFFFFF), (80, 60), (120, 0xFFFFFFFF), (55, 44)])
def test_other_lengths_equal_reference(refh, target, min_len):
    s = _rcdata.literal_like(150_000, 11, copies=50, longest=1500)
    got, _, _ = _orc.rc_find_matches(s, target, min_len)
    assert np.array_equal(got, refh.rc_find_matches(s, target, min_len))
    assert _orc.rc_match_sequence(s, target, min_len)[:3] == refh.rc_match_sequence(s, target, min_len)


@pytest.mark.parametrize("target,group,content", _rcdata.EDGE_ITEMS)
def test_edge_lengths_equal_reference(refh, target, group, content):
    """texts of block-boundary, tail and text-edge lengths (_rcdata.edge_inputs): rows in push order, the derived parameters,
    the rewritten stream and both maps, with the default minimum"""
    item = _rcdata.edge_item(target, group, content)
    assert item, "no input fits"
    for name, s in item:
        if s.size >= target:
            got, params, _ = _orc.rc_find_matches(s, target)
            want, wparams = refh.rc_find_matches_params(s, target)
            assert params == wparams and params[:3] == _rcdata.edge_params(target), name
            assert got.shape == want.shape and np.array_equal(got, want), name
            _rcdata.edge_expect(name, s, got, target)
            a = _orc.rc_match_sequence(s, target)
            assert a == _orc.rc_apply_matches(s, got, target), name              # (what test_gpu_rcmatch_edges.py compares with)
        else:
            a = _orc.rc_match_sequence(s, target)
            assert a == (s.tobytes(), b"", b"", (0, 0, 0)), name
        assert a[:3] == refh.rc_match_sequence(s, target), name


def test_edge_inputs_cover_what_they_name():
    """the lengths sit where the number of whole blocks and the tail's size change, and every content is there at every length
    of its group at which it can fit (needs no reference build)"""
    for target in _rcdata.EDGE_TARGETS:
        K, k1, k2 = _rcdata.edge_params(target)
        lengths = _rcdata.edge_lengths(target)
        B = [K + 256 * k2 * (m + 1) for m in range(3)]
        for m in range(3):
            assert _rcdata.edge_geometry(B[m] - 1, K, k2) == (m, 256 * k2 * m)                  # a tail of 256 samples
            assert _rcdata.edge_geometry(B[m], K, k2) == (m + 1, 256 * k2 * (m + 1))            # a tail of one
            assert {B[m] - 1, B[m], B[m] + 1} <= set(lengths["m%d" % m])
        assert {B[1] + k2 - 1, B[1] + k2} <= set(lengths["m1"])
        names = [name for name, _ in _rcdata.edge_inputs(target)]
        assert len(names) == len(set(names))
        for g in _rcdata.EDGE_GROUPS:
            for c in ("none", "whole", "at", "acgt", "aatt"):
                assert len(_rcdata.edge_item(target, g, c)) == len(lengths[g]), (target, g, c)
            if g != "t":
                m = int(g[1])
                assert len(_rcdata.edge_item(target, g, "ends")) == len(lengths[g])
                assert [s.size for _, s in _rcdata.edge_item(target, g, "tail_only")] == [B[m] - 1]
                # a text with no whole block has no boundary to reach over: B(0) - 1 is left out
                assert [s.size for _, s in _rcdata.edge_item(target, g, "into_tail")] == [n for n in lengths[g] if n >= B[0]]


def restore(seq, map_off, map_len, org_len):
    """SimpleSequenceMatcher::restoreRCMatchedSequence, matching/SimpleSequenceMatcher.cpp:178-211 (the decoder's inverse)"""
    def byte_frugal(buf, at):
        v, base = 0, 1
        while True:
            y = buf[at]; at += 1
            v += base * (y % 128); base *= 128
            if y < 128:
                return v, at
    comp = _rcdata.COMP.copy()
    out = bytearray()
    min_len, lp = byte_frugal(map_len, 0)
    op = 0
    for b in seq:
        if b != 0xA4:                                                 # RC_MATCH_MARK = '$' + 128
            out.append(b)
            continue
        src = int.from_bytes(map_off[op:op + 4], "little"); op += 4
        ln, lp = byte_frugal(map_len, lp)
        ln += min_len
        piece = bytes(out[src:src + ln]) if src + ln <= len(out) else None
        assert piece is not None
        out += bytes(comp[np.frombuffer(piece, dtype=np.uint8)][::-1])
    assert len(out) == org_len
    return bytes(out)


@pytest.mark.parametrize("name", ["planted", "long_copies", "manyfold"])
def test_rewritten_stream_restores(name):
    s = CASES[name].copy()
    s[s == 0xA4] = ord("A")                                           # (the mark itself must not occur in the input)
    s[(s >= ord("a")) & (s <= ord("z"))] = ord("C")                   # upper-case input: the restore complements with the upper table
    s[s == ord("N")] = ord("G")
    seq, off, ln, st = _orc.rc_match_sequence(s)
    assert st[1] > 0 and len(seq) < s.size
    assert restore(seq, off, ln, s.size) == s.tobytes()
