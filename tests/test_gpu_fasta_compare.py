"""mbgc_fasta_compare_dev (k_fa_compare: what `mbgc-hip v` compares with) through the ctypes mirror, on torch buffers, against numpy's
first index where the two arrays differ: piece lengths around the 16-byte lane step and the 4096-byte tile, every combination of the
two sides' offsets modulo 16, pieces that end with their buffers, differences at the step's and the tile's edges, slots shared and
apart, a call of more tiles than one grid slice, and the refusal of a piece that does not lie inside the buffers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5]
MODS = [0, 1, 15]
NONE = 2 ** 64 - 1


def layout(specs, lead=True):
    """specs: [(len, aOff % 16, bOff % 16, slot)] -> (a, b as numpy arrays that end with the last piece, pieces [(aOff, bOff, len, slot)]).
    The pieces are equal; every byte outside them differs between a and b, and one such byte at least stands on each side of a piece
    (lead=False: the first piece may start at byte 0)."""
    rng = np.random.default_rng(len(specs) * 131 + sum(s[0] for s in specs) % 977)
    pieces, ea, eb = [], 0, 0
    for n, am, bm, slot in specs:
        ao = ea + (1 if lead or pieces else 0)
        ao += (am - ao) % 16
        bo = eb + (1 if lead or pieces else 0)
        bo += (bm - bo) % 16
        pieces.append((ao, bo, n, slot))
        ea, eb = ao + n, bo + n
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), max(ea, 1))
    b = rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), max(eb, 1))
    for ao, bo, n, _ in pieces:
        b[bo: bo + n] = a[ao: ao + n]
    return a[:ea].copy(), b[:eb].copy(), pieces


def expected(a, b, pieces, nslots):
    want = np.full(nslots, NONE, dtype=np.uint64)
    for ao, bo, n, slot in pieces:
        d = np.flatnonzero(a[ao: ao + n] != b[bo: bo + n])
        if d.size:
            want[slot] = min(int(want[slot]), int(d[0]))
    return want


def to_device(x):
    """-> (tensor that keeps the bytes alive, a 16-byte aligned device address at which x stands)"""
    import torch
    buf = torch.zeros(x.size + 32, dtype=torch.uint8, device="cuda:0")
    base = (-buf.data_ptr()) % 16
    buf[base: base + x.size] = torch.from_numpy(x).to("cuda:0")
    return buf, buf.data_ptr() + base


def compare(a, b, pieces, nslots, first_diff=None):
    import torch
    from mbgc_amd import fasta
    ka, pa = to_device(a)
    kb, pb = to_device(b)
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        got, _ = p.compare_dev(pa, a.size, pb, b.size, pieces, nslots, first_diff)
    finally:
        p.close()
    del ka, kb
    return got


def check(a, b, pieces, nslots):
    got, want = compare(a, b, pieces, nslots), expected(a, b, pieces, nslots)
    assert got.tolist() == want.tolist(), (pieces, got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("bm", MODS)
@pytest.mark.parametrize("am", MODS)
def test_lengths_alignments_and_planted_positions(am, bm):
    """all the lengths in one call, a slot each, the last piece ending with both buffers; equal first, then one difference per piece at
    byte 0, the last byte, 15, 16, 4095 and 4096 (where the piece holds that byte)"""
    specs = [(n, am, bm, i) for i, n in enumerate(LENGTHS)]
    a, b, pieces = layout(specs)
    assert pieces[-1][0] + pieces[-1][2] == a.size and pieces[-1][1] + pieces[-1][2] == b.size
    assert all(p[0] % 16 == am and p[1] % 16 == bm for p in pieces)
    assert check(a, b, pieces, len(specs)).tolist() == [NONE] * len(specs)
    for at in (0, -1, 15, 16, 4095, 4096):
        b2 = b.copy()
        planted = 0
        for ao, bo, n, slot in pieces:
            if n and -n <= at < n:
                b2[bo + at % n] ^= 0x20
                planted += 1
        got = check(a, b2, pieces, len(specs))
        assert sum(v != NONE for v in got.tolist()) == planted > 0
        # (the shorter pieces, and the empty one, stay equal: their neighbours' differences are not theirs)


def test_ends_with_the_buffers_from_byte_zero():
    """one piece that is the whole of both buffers, and a piece that is the whole of a against the tail of b"""
    a, b, pieces = layout([(4097, 0, 0, 0)], lead=False)
    assert pieces == [(0, 0, 4097, 0)] and a.size == b.size == 4097
    check(a, b, pieces, 1)
    b[4096] ^= 0x20
    assert check(a, b, pieces, 1).tolist() == [4096]
    a, b, pieces = layout([(33, 0, 7, 0)], lead=False)
    assert pieces[0][1] == 7 and b.size == 40
    a[32] ^= 0x20
    assert check(a, b, pieces, 1).tolist() == [32]


def test_two_differences_in_one_piece_report_the_first():
    a, b, pieces = layout([(3 * 4096 + 5, 1, 15, 0)])
    for first, second in ((17, 18), (100, 5000), (4095, 4096), (0, 3 * 4096 + 4), (1023, 1024)):      # (1024: the next wave's first byte at offset 0 mod 16)
        b2 = b.copy()
        b2[pieces[0][1] + first] ^= 0x20
        b2[pieces[0][1] + second] ^= 0x20
        assert check(a, b2, pieces, 1).tolist() == [first]


def test_slots_apart_are_independent_and_a_shared_slot_takes_the_smaller():
    specs = [(5000, 1, 0, 0), (300, 15, 15, 1), (5000, 0, 1, 2), (40, 0, 0, 1)]
    a, b, pieces = layout(specs)
    b2 = b.copy()
    b2[pieces[0][1] + 4500] ^= 0x20
    b2[pieces[2][1] + 7] ^= 0x20
    assert check(a, b2, pieces, 3).tolist() == [4500, NONE, 7]
    b2 = b.copy()                                                     # pieces 1 and 3 share slot 1: offsets within each piece
    b2[pieces[1][1] + 200] ^= 0x20
    b2[pieces[3][1] + 30] ^= 0x20
    assert check(a, b2, pieces, 3).tolist() == [NONE, 30, NONE]
    b2[pieces[1][1] + 29] ^= 0x20
    assert check(a, b2, pieces, 3).tolist() == [NONE, 29, NONE]
    # several pieces inside one wave's 1024 bytes, each with a difference and a slot of its own
    specs = [(20, i % 16, (3 * i) % 16, i) for i in range(12)]
    a, b, pieces = layout(specs)
    for i, (ao, bo, n, slot) in enumerate(pieces):
        b[bo + (i * 5) % n] ^= 0x20
    assert check(a, b, pieces, 12).tolist() == [(i * 5) % 20 for i in range(12)]


@pytest.mark.parametrize("n", [1, 16, 4096, 4097])
def test_a_difference_just_outside_a_piece_is_not_reported(n):
    """the bytes in front of and behind the piece differ on both sides of the comparison; the piece itself is equal"""
    for am, bm in ((0, 0), (1, 15), (15, 1)):
        a, b, pieces = layout([(n, am, bm, 0), (1, 0, 0, 1)])
        ao, bo = pieces[0][0], pieces[0][1]
        assert ao >= 1 and bo >= 1 and a[ao - 1] != b[bo - 1] and a[ao + n] != b[bo + n]
        assert check(a, b, pieces, 2).tolist() == [NONE, NONE]


def test_all_equal_and_no_piece():
    a, b, pieces = layout([(n, 3, 9, i % 2) for i, n in enumerate(LENGTHS)])
    assert check(a, b, pieces, 2).tolist() == [NONE, NONE]
    assert compare(a, b, [], 3).tolist() == [NONE] * 3
    assert compare(a, b, [(5, 5, 0, 2)], 3).tolist() == [NONE] * 3


def test_more_tiles_than_one_launch_slice():
    """70 pieces of 1000 tiles each: 70 000 tiles, past the 65 535 of one launch. They read the same 4 MB of a; the last one's b side is a
    copy of its own with one byte changed, piece 3 shares its slot, piece 0's copy differs early"""
    n = 1000 * 4096
    rng = np.random.default_rng(70)
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
    b = np.concatenate([a, a, a])
    b[n + 4_000_001] ^= 0x20
    b[2 * n + 77] ^= 0x20
    pieces = [(0, 2 * n, n, 0)] + [(0, 0, n, 1 + k % 5) for k in range(1, 69)] + [(0, n, n, 6)]
    assert sum(p[2] for p in pieces) // 4096 == 70_000
    got = check(a, b, pieces, 7)
    assert got.tolist() == [77, NONE, NONE, NONE, NONE, NONE, 4_000_001]


@pytest.mark.parametrize("bad", [(90, 0, 11, 0), (0, 95, 6, 0), (101, 0, 0, 0), (0, 0, 2 ** 63, 0), (0, 0, 4, 2)],
                         ids=["a-side", "b-side", "starts-behind-the-end", "length-overflows", "slot"])
def test_a_piece_out_of_range_is_refused_and_the_result_left_untouched(bad):
    from mbgc_amd import binding
    a, b, _ = layout([(100, 0, 0, 0)], lead=False)
    assert a.size == b.size == 100
    b[50] ^= 0x20
    out = np.array([12345, 67890], dtype=np.uint64)
    with pytest.raises(binding.SwsemError, match="compare: piece 1"):
        compare(a, b, [(0, 0, 100, 0), bad], 2, first_diff=out)
    assert out.tolist() == [12345, 67890]
    assert compare(a, b, [(0, 0, 100, 0)], 2, first_diff=out).tolist() == [50, NONE]      # the same handle kind of call goes through afterwards
