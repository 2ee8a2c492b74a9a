"""The `-m3` reverse-complement pass on the device (mbgc_amd/csrc/copmem.hip) against the oracle (oracle/rcmatch_oracle.c) where
its geometry changes with the text's length: one byte either side of every length at which the number of whole 256-sample query
blocks grows (the tail then shrinks from 256 samples to one), matches that run into the text's two ends, that are carried from
the last whole block into the tail or found in the tail alone, texts that are their own reverse complement, periodic texts whose
buckets overflow — for five target lengths (_rcdata.edge_inputs) — and one text long enough for a 25-bit mask."""
import numpy as np
import pytest

import _orc
import _rcdata

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssm():
    from mbgc_amd import copmem
    m = copmem.SimpleSequenceMatcher()
    yield m
    m.close()


def oracle(s, target):
    """-> (rows, params, rc_match_sequence's result). orc_rc_match_sequence is orc_rc_find_matches followed by
    orc_rc_apply_matches and nothing else (test_rcmatch_oracle.py holds the two equal on these inputs): one index, not two."""
    if s.size < target:
        return np.zeros((0, 3), dtype=np.uint64), None, (s.tobytes(), b"", b"", (0, 0, 0))
    rows, params, _ = _orc.rc_find_matches(s, target)
    return rows, params, _orc.rc_apply_matches(s, rows, target)


@pytest.mark.parametrize("target,group,content", _rcdata.EDGE_ITEMS)
def test_edge_lengths_equal_oracle(ssm, target, group, content):
    """rows (shape, order, value) and derived parameters, the rewritten stream with both maps and the three stats, and the way
    back through the device's inverse; the item's lengths ascending and then descending through one handle, whose buffers
    never shrink: nothing may depend on what a longer text left in them"""
    item = _rcdata.edge_item(target, group, content)
    assert item, "no input fits"
    want = {}
    for name, s in item:
        want[name] = oracle(s, target)
        _rcdata.edge_expect(name, s, want[name][0], target)
    for name, s in item + item[::-1]:
        rows, params, seq = want[name]
        if s.size >= target:                                              # (shorter: no matcher is built, no parameters)
            got, gparams = ssm.rc_matches(s, target)
            assert gparams == params, name
            assert got.shape == rows.shape and np.array_equal(got, rows), (name, got[:4].tolist(), rows[:4].tolist())
        cut, map_off, map_len, stats = ssm.rc_match_sequence(s, target)
        assert (cut, map_off, map_len, stats) == seq, name
        if len(map_off):
            back, rstats = ssm.rc_restore_sequence(cut, map_off, map_len)
            assert back == s.tobytes(), name
            assert rstats["marks"] == len(map_off) // 4 and rstats["restored_from_matches"] == stats[1]


def test_mask_of_25_bits(ssm):
    """the smallest text whose index takes a 25-bit mask (hash_size grows while it is below n / k1; target length 25 gives
    K = 20, k1 = 3: n / 3 > 2^24) — the radix sort's bit count and the sizes of the count and offset tables follow the mask —
    with a few hundred planted reverse-complement copies and one of 1 Mbp. The counterpart of test_gpu_rcmatch.py's
    test_literal_stream_sized_input (64 MB, target length 55, 24 bits)."""
    target = 25
    n = 3 * (2 ** 24 + 1)
    rng = np.random.default_rng(25)
    s = _rcdata.ACGT[rng.integers(0, 4, n)].copy()
    s[30_000_000:31_000_000] = _rcdata.revcomp(s[2_000_000:3_000_000])
    for k in range(300):
        a, b, ln = int(rng.integers(0, n - 5000)), int(rng.integers(0, n - 5000)), int(rng.integers(60, 4000))
        s[b:b + ln] = _rcdata.revcomp(s[a:a + ln])
    want, wparams, _ = _orc.rc_find_matches(s, target)
    assert wparams == (20, 3, 2, 25)
    got, params = ssm.rc_matches(s, target)
    assert params == wparams and got.shape == want.shape and np.array_equal(got, want)
    a, b = ssm.rc_match_sequence(s, target), _orc.rc_apply_matches(s, want, target)
    assert a == b and a[3][1] > 950_000 and len(want) > 300
    assert ssm.rc_matches(s[:n - 1], target)[1] == (20, 3, 2, 24)         # one byte less: (n - 1) / 3 == 2^24, the loop stops at 24
