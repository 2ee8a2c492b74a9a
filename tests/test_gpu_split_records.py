"""mbgc_fasta_split_buf_dev2 on the GPU: the split with a rule for what a mark is (MBGC_FASTA_SPLIT_LINE_START: only at offset 0 of
the buffer or right behind a line feed; MBGC_FASTA_SPLIT_AT: '@' beside '>') against the restatement
tests/_singlefasta_lossy.split_records, on the smallest shapes at which the look-behind can go wrong: the 4096-byte tile edge, the
1 KiB load edge, the 16-byte lane edge, the dword edge, the seam of a scan that is resumed; and flags 0 against
mbgc_fasta_split_buf_dev."""
import numpy as np
import pytest

import _singlefasta_lossy as sfl

pytestmark = pytest.mark.gpu
LS, AT, BOTH = sfl.LINE_START, sfl.AT, sfl.LINE_START | sfl.AT
TILE = 4096


class Dev:
    def __init__(self, data, shift=0):
        import torch
        from mbgc_amd import fasta
        self.data = bytes(data)
        self.buf = torch.from_numpy(np.frombuffer(b"\n" * shift + self.data + b"\n>@\n>@\n>@\n>@\n>@\n", dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()                                   # (marks behind the window's end: nothing may read them)
        self.ptr = self.buf.data_ptr() + shift
        self.p = fasta.FastaParser()

    def __call__(self, start, n, scanned, is_end, mins, flags, max_elems=64):
        first_min, next_min = (mins, mins) if isinstance(mins, int) else mins
        return self.p.split_buf_dev2(self.ptr, start, n, scanned, is_end, first_min, next_min, flags, max_elems)

    def close(self):
        self.p.close()


def check(data, mins, start=0, flag_sets=(BOTH, LS, AT, 0), max_elems=64, shift=0):
    d = Dev(data, shift)
    for flags in flag_sets:                                        # (each call changes the rule: the kept tiles are not reused)
        for is_end in (True, False):
            got = d(start, len(data), 0, is_end, mins, flags, max_elems)
            assert got == sfl.split_records(data, start, mins, flags, is_end, max_elems), (flags, is_end, mins, start)
    d.close()


def at(offset, mark, total=3 * TILE, fill=b"A"):
    """a buffer of `total` bytes, "\\n" + mark so that the mark stands at `offset`"""
    b = bytearray(fill * total)
    if offset:
        b[offset - 1] = 0x0A
    b[offset:offset + len(mark)] = mark
    return bytes(b)


@pytest.mark.parametrize("offset", [4095, 4096, 4097, 1023, 1024, 1025, 15, 16, 17, 3, 4, 5, 8191, 8192])
def test_a_mark_behind_a_line_feed_across_every_edge(offset):
    """the line feed is the last byte of the tile (the load, the lane's 16 bytes, the dword) before the mark's, or the mark is"""
    for mark in (b">", b"@"):
        data = at(offset, mark)
        for mins in (1, offset, max(1, offset - 1), (offset + 1, 1)):   # the threshold inside the mark's tile, on the mark, behind it
            check(data, mins)
        miss = bytearray(data)
        miss[offset - 1] = 0x0D                                    # a CR in the line feed's place: not a line start
        check(bytes(miss), 1)


def test_marks_inside_a_line_are_not_taken():
    data = b">h a > b @ c\nAC>GT@AC\n" * 400 + b"\r\n>x\r\n@y\r>z\r\n" + b"AC@>\n" * 900 + b"\n>last\nAC\n"
    assert len(data) > 3 * TILE
    for mins in (1, 7, 100, 5000, (1, 4097)):
        check(data, mins)
        check(data, mins, shift=5)                                 # (a window that starts anywhere in its buffer)
    check(data, 1, max_elems=4096)                                 # every mark of the buffer, one by one
    check(data, 1, max_elems=3)


def test_a_mark_at_buffer_offset_0_and_a_nonzero_start():
    data = b">a\nAC\n@b\nG>\n>c\nA@\n"
    d = Dev(data)
    assert d(0, len(data), 0, True, 1, BOTH) == [6, 12, 18] == sfl.split_records(data, 0, 1, BOTH)
    assert d(0, 6, 0, True, 1, BOTH) == [6] and d(0, 6, 0, False, 1, BOTH) == []
    d.close()
    big = data + b"A" * (2 * TILE) + b"\n" + data                  # the same records behind a tile edge
    for start in (0, 6, 12, 18, len(big) - 18, len(big) - 12):
        for mins in (1, 6, 7, 5000):
            check(big, mins, start=start)
    # offset 0 of the BUFFER is a line start, `start` is not one: with a '>' at 0 and the tile array's first entry read for a
    # threshold in tile 0, the first mark of tile 0 stands before every threshold and the rest of the tile is walked
    check(b">" + b"A" * 99 + b">" + b"A" * 100 + b"\n>" + b"A" * 50, 1)
    check(b">" + b"A" * 99 + b">" + b"A" * 100 + b"\n>" + b"A" * 50, 1, start=100)


def test_no_mark_at_all():
    for data in (b"A" * 9000, b"\n" * 9000, b"A>@\r>" * 2000, b"A"):
        check(data, 1)
        check(data, 5000)
    d = Dev(b"ACGT" * 3000)
    assert d(0, 12000, 0, False, 1, BOTH) == [] and d(0, 12000, 0, True, 1, BOTH) == [12000] and d(12000, 12000, 0, True, 1, BOTH) == []
    d.close()


def test_a_buffer_grown_in_three_appends():
    """scannedBefore: the tiles of the bytes scanned before stand, the scan is resumed at the tile that was not whole — the seams
    fall between a line feed and its mark (the look-behind reads a byte of the part scanned before), on a tile edge and inside
    a tile; the ends must be those of one call over everything"""
    rng = np.random.default_rng(21)
    body = rng.choice(np.frombuffer(b"ACGT\n", dtype=np.uint8), 5 * TILE + 300).tobytes().replace(b"\n", b"\nA")[:5 * TILE + 300]
    b = bytearray(body.replace(b">", b"A").replace(b"@", b"A"))
    seams = [TILE, 3 * TILE + 117, len(b)]
    for s, mark in zip(seams[:2], (b">", b"@")):
        b[s - 1:s + 1] = b"\n" + mark                               # ... | '\n' ][ mark | ...
    b[2 * TILE + 5:2 * TILE + 7] = b"\n>"
    data = bytes(b)
    for flags in (BOTH, LS):
        want = sfl.split_records(data, 0, 100, flags)
        assert (seams[0] in want) and ((seams[1] in want) == bool(flags & AT))
        d = Dev(data, shift=3)
        got, done, scanned = [], 0, 0
        for have in seams:
            ends = d(done, have, scanned, have == len(data), 100, flags, 1000)
            assert ends == sfl.split_records(data[:have], done, 100, flags, have == len(data)), (flags, have)
            got += ends
            done, scanned = (ends[-1] if ends else done), have
        assert got == want
        d.close()


@pytest.mark.parametrize("seed,alphabet,mins,max_elems", [(1, b">@\n\rA", 1, 400_000), (2, b">@\n\rA", (5000, 60_000), 4096),
                                                         (3, b"A" * 60 + b">@\n\r", 777, 8192)])
def test_random_bytes(seed, alphabet, mins, max_elems):
    rng = np.random.default_rng(seed)
    n = 2 * (1 << 20) + int(rng.integers(0, 5000))
    data = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tobytes()
    check(data, mins, flag_sets=(BOTH,), max_elems=max_elems, shift=int(rng.integers(0, 16)))
    d = Dev(data)
    for flags in (LS, AT):
        cut = int(rng.integers(n // 3, n))
        assert d(0, cut, 0, False, mins, flags, max_elems) == sfl.split_records(data[:cut], 0, mins, flags, False, max_elems)
    d.close()


def test_without_flags_the_call_is_split_buf_dev():
    rng = np.random.default_rng(4)
    n = (1 << 20) + 333
    data = rng.choice(np.frombuffer(b"A" * 30 + b">@\n", dtype=np.uint8), n).tobytes()
    d = Dev(data, shift=7)
    for start, have, is_end, mins in ((0, n, True, 5000), (0, n // 2, False, 5000), (4097, n, True, 1), (0, n, False, 70_000)):
        old = d.p.split_buf_dev(d.ptr, start, have, 0, is_end, mins, mins, 100_000)
        assert d(start, have, 0, is_end, mins, 0, 100_000) == old == sfl.split_records(data[:have], start, mins, 0, is_end, 100_000)
    d.close()
    from mbgc_amd import binding
    d = Dev(b">a\n")
    with pytest.raises(binding.SwsemError):
        d(0, 3, 0, True, 1, 4)                                      # a flag the call does not know
    d.close()
