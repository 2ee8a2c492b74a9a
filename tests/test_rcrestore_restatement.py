"""tests/_rcrestore.py, the Python restatement of SimpleSequenceMatcher::restoreRCMatchedSequence the device tests are held to,
against the oracle's forward pass (oracle/rcmatch_oracle.c, pinned on the reference): what rcMatchSequence cuts comes back."""
import numpy as np
import pytest

import _orc
import _rcrestore

INPUTS = _rcrestore.inputs()


@pytest.mark.parametrize("name", _rcrestore.CASES)
def test_the_oracles_forward_pass_comes_back(name):
    s = INPUTS[name]
    cut, map_off, map_len, stats = _orc.rc_match_sequence(s)
    if name != "tiny":
        assert stats[1] > 0 and cut.count(bytes([_rcrestore.MARK])) * 4 == len(map_off)
    else:
        assert (cut, map_off, map_len) == (s.tobytes(), b"", b"")
    assert _rcrestore.restore(cut, map_off, map_len) == s.tobytes()


def test_the_table_is_an_involution_but_for_127():
    lut = _rcrestore.LUT
    twice = lut[lut]
    assert [i for i in range(256) if twice[i] != i] == [127]
    assert np.array_equal(lut[twice], lut)                                       # lut . lut . lut == lut, 127 included


def test_byte_frugal_values():
    for v in (0, 1, 127, 128, 16383, 16384, 2 ** 32 - 1, 2 ** 63):
        b = _rcrestore.put_byte_frugal(v)
        assert _rcrestore.read_byte_frugal(b + b"\x00", 0) == (v, len(b))
    assert [len(_rcrestore.put_byte_frugal(v)) for v in (127, 128, 16383, 16384)] == [1, 2, 2, 3]


def test_substr_semantics():
    x = b"ACGTTGCA" * 4
    cut = x + bytes([_rcrestore.MARK])
    off, ln = _rcrestore.build_maps(0, [(30, 10)])                               # runs over the end: truncated to 2 bytes
    assert _rcrestore.restore(cut, off, ln) == x + _rcrestore.LUT[np.frombuffer(x[30:], dtype=np.uint8)][::-1].tobytes()
    off, ln = _rcrestore.build_maps(0, [(33, 1)])                                # begins beyond the end: substr throws
    with pytest.raises(IndexError):
        _rcrestore.restore(cut, off, ln)
    off8, ln8 = _rcrestore.build_maps(3, [(4, 9)], off_bytes=8)
    off4, ln4 = _rcrestore.build_maps(3, [(4, 9)])
    assert len(off8) == 8 and _rcrestore.restore(cut, off8, ln8, 8) == _rcrestore.restore(cut, off4, ln4)
