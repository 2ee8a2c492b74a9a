"""The inverse of the `-m3` reverse-complement pass on the device (mbgc_amd/csrc/copmem_restore.h through the C ABI of
include/mbgc_copmem.h): the round trip with the device's own forward pass, hand-built streams against tests/_rcrestore.py (the
restatement of SimpleSequenceMatcher::restoreRCMatchedSequence), and the refusals of the plan."""
import numpy as np
import pytest

import _rcrestore
from _rcrestore import MARK, build_maps

pytestmark = pytest.mark.gpu
INPUTS = _rcrestore.inputs()
M = bytes([MARK])


@pytest.fixture(scope="module")
def ssm():
    from mbgc_amd import copmem
    m = copmem.SimpleSequenceMatcher()
    yield m
    m.close()


@pytest.mark.parametrize("name", _rcrestore.CASES)
def test_round_trip(ssm, name):
    s = INPUTS[name]
    cut, map_off, map_len, fwd = ssm.rc_match_sequence(s)
    back, stats = ssm.rc_restore_sequence(cut, map_off, map_len)
    assert back == s.tobytes(), name
    assert stats["marks"] == cut.count(M) and stats["restored_from_matches"] == fwd[1]
    if name != "tiny":
        assert stats["marks"] >= 1 and stats["min_match_length"] == 55 and stats["max_chain"] >= 1
    else:
        assert stats["marks"] == 0 and map_len == b""


def hand_built():
    """-> (cut stream, [(source, length)], minMatchLength 0); positions in restored coordinates in the comments"""
    rng = np.random.default_rng(31)
    x = bytes(np.frombuffer(b"ACGTacgtNnRYKMBDHVWSU", dtype=np.uint8)[rng.integers(0, 21, 200)])
    lit = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])
    parts, matches = [], []
    parts += [M]; matches.append((0, 0))                     # d = 0: a zero-length match as the stream's first byte
    parts += [x]                                             # [0, 200)
    parts += [M]; matches.append((0, 200))                   # d = 200: all of X                                       -> [200, 400)
    parts += [lit(7)]                                        # [400, 407)
    parts += [M]; matches.append((150, 100))                 # d = 407: the end of X and the head of the first match   -> [407, 507)
    parts += [lit(3)]                                        # [507, 510)
    parts += [M]; matches.append((210, 150))                 # d = 510: inside match 1 (depth 2)                       -> [510, 660)
    parts += [M]; matches.append((523, 101))                 # d = 660: back to back; inside match 3 (depth 3)         -> [660, 761)
    parts += [M]; matches.append((665, 90))                  # d = 761: inside match 4 (depth 4)                       -> [761, 851)
    parts += [lit(21)]                                       # [851, 872)
    parts += [M]; matches.append((771, 101))                 # d = 872: its source ends exactly where it starts        -> [872, 973)
    parts += [lit(5)]                                        # [973, 978)
    parts += [M]; matches.append((3, 37))                    # d = 978: off the 16-byte grid at both ends              -> [978, 1015)
    parts += [lit(40)]                                       # [1015, 1055)
    parts += [M]; matches.append((1001, 33))                 # d = 1055: literals and a match, the stream's last byte  -> [1055, 1088)
    return b"".join(parts), matches


def test_hand_built_stream(ssm):
    cut, matches = hand_built()
    assert cut[0] == MARK and cut[-1] == MARK and matches[6][0] + matches[6][1] == 872
    map_off, map_len = build_maps(0, matches)
    want = _rcrestore.restore(cut, map_off, map_len)
    assert len(want) == 1088
    got, stats = ssm.rc_restore_sequence(cut, map_off, map_len)
    assert got == want
    assert stats["marks"] == len(matches) and stats["max_chain"] >= 3 and stats["min_match_length"] == 0
    assert stats["restored_from_matches"] == sum(ln for _, ln in matches)


def test_eight_byte_offsets(ssm):
    cut, matches = hand_built()
    off4, ln = build_maps(0, matches)
    off8, _ = build_maps(0, matches, off_bytes=8)
    a, _ = ssm.rc_restore_sequence(cut, off4, ln)
    b, _ = ssm.rc_restore_sequence(cut, off8, ln, off_bytes=8)
    assert a == b == _rcrestore.restore(cut, off8, ln, 8)
    from mbgc_amd import binding
    with pytest.raises(binding.SwsemError, match="8-byte offsets"):          # the reference's rule: a stream this short has 4-byte offsets
        ssm.rc_restore_sequence(cut, off8, ln)


def test_a_device_destination(ssm):
    import torch
    cut, matches = hand_built()
    map_off, map_len = build_maps(0, matches)
    n, _, _ = ssm.rc_restore_plan(cut, map_off, map_len)
    t = torch.zeros(n + 5, dtype=torch.uint8, device="cuda")
    host, _, _ = ssm.rc_restore_fill(n, cap=n + 5, dst_dev=t.data_ptr())
    assert bytes(t.cpu().numpy()[:n]) == host == _rcrestore.restore(cut, map_off, map_len) and not t[n:].any()


def test_varints(ssm):
    """deltas of 127, 128, 16383 and 16384 over a minimal length of two bytes (200): sources built by doubling"""
    rng = np.random.default_rng(32)
    x = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 600)])
    min_len = 200
    parts, matches, have = [x], [], 600
    for ln in (600, 1200, 2400, 4800, 9600, 19200):                        # each doubles what is there
        parts.append(M); matches.append((0, have)); have *= 2
    assert have == 38400
    for delta in (127, 128, 16383, 16384, 0):
        parts.append(b"TTGACA" + M); have += 6
        matches.append((have - 6 - (min_len + delta) - 11, min_len + delta)); have += min_len + delta
    cut = b"".join(parts)
    map_off, map_len = build_maps(min_len, matches)
    assert map_len[:2] == _rcrestore.put_byte_frugal(200) and len(map_len[:2]) == 2 and have < 100_000
    got, stats = ssm.rc_restore_sequence(cut, map_off, map_len)
    assert len(got) == have and got == _rcrestore.restore(cut, map_off, map_len)
    assert stats["min_match_length"] == 200 and stats["max_chain"] >= 6


def refusals():
    cut, matches = hand_built()
    off, ln = build_maps(0, matches)
    m = len(matches)
    bad_src = list(matches); bad_src[2] = (308, 100)                        # src + len == d + 1 (d = 407)
    far_src = list(matches); far_src[2] = (5000, 100)                       # beyond the end of everything
    nomark = cut.replace(M, b"A")
    return {
        "rcMapOff one byte short": (cut, off[:-1], ln),
        "rcMapOff with 4M + 4 bytes": (cut, off + b"\x00\x00\x00\x00", ln),
        "rcMapLen ends inside a value": (cut, off, ln[:-1] + b"\x85"),
        "rcMapLen one value short": (cut, off, ln[:-1]),
        "rcMapLen one value too many": (cut, off, ln + b"\x05"),
        "a varint of 11 bytes": (cut, off, ln[:-1] + b"\x80" * 10 + b"\x00"),
        "src + len == d + 1": (cut,) + build_maps(0, bad_src),
        "src beyond the end": (cut,) + build_maps(0, far_src),
        "rcMapOff without a mark": (nomark, off[:4 * m], b""),
        "lengths beyond 64 bits": (cut, off, ln[:-1] + b"\xff" * 9 + b"\x01"),
    }


REFUSALS = refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_malformed_maps_are_refused_by_the_plan(ssm, name):
    from mbgc_amd import binding
    good_cut, matches = hand_built()
    good = (good_cut,) + build_maps(0, matches)
    with pytest.raises(binding.SwsemError, match=r"copmem error -4: \S") as e:
        ssm.rc_restore_plan(*REFUSALS[name])
    assert "malformed" in str(e.value)
    assert ssm.rc_restore_sequence(*good)[0] == _rcrestore.restore(*good)    # the handle and the process go on


def test_a_destination_too_small_is_refused_by_the_fill(ssm):
    from mbgc_amd import binding
    cut, matches = hand_built()
    map_off, map_len = build_maps(0, matches)
    n, _, _ = ssm.rc_restore_plan(cut, map_off, map_len)
    with pytest.raises(binding.SwsemError, match=r"copmem error -4: \S"):
        ssm.rc_restore_fill(n, cap=n - 1)
    assert ssm.rc_restore_fill(n)[0] == _rcrestore.restore(cut, map_off, map_len)
    assert ssm.rc_restore_sequence(cut, map_off, map_len)[0] == _rcrestore.restore(cut, map_off, map_len)


def test_no_marks_and_empty_streams(ssm):
    s = INPUTS["short"].tobytes().replace(M, b"A")
    assert ssm.rc_restore_sequence(s, b"", b"")[0] == s                       # shorter than the target length: no matcher, empty maps
    assert ssm.rc_restore_sequence(s, b"", _rcrestore.put_byte_frugal(55))[0] == s   # a matcher that found nothing
    assert ssm.rc_restore_sequence(b"", b"", b"")[0] == b""
