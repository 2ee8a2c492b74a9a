"""mbgc_fasta_crc_dev through the ctypes mirror (FastaParser.crc_dev), on torch buffers, against zlib.crc32. The kernel's thresholds
are powers of two — 256 bytes (a lane's share and the one-lane class), 1024, 4096 and 16384 (the groups of 4, 16 and 64 lanes; 16384
is also the piece a longer range is cut into) — so the lengths 2^j - 1, 2^j, 2^j + 1 for j = 0..17 straddle every one of them. The
buffers are allocated exactly (the last range ends on the buffer's last byte) unless a test says otherwise."""
import zlib

import numpy as np
import pytest
import torch

from mbgc_amd import binding, fasta

pytestmark = pytest.mark.gpu

LENGTHS = sorted({0} | {(1 << j) + d for j in range(18) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def parser():
    p = fasta.FastaParser()
    yield p
    p.close()


def content(kind, n, seed=3):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return np.full(n, 0x00 if kind == "zeros" else 0xFF, dtype=np.uint8)


def run(parser, data, ranges):
    """data: the whole buffer (numpy uint8), allocated on the device exactly as long as it is"""
    buf = torch.from_numpy(data.copy() if data.size else np.zeros(1, dtype=np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    got, _ = parser.crc_dev(buf.data_ptr(), data.size, ranges)
    host = data.tobytes()
    want = [zlib.crc32(host[o:o + n]) for o, n in ranges]
    bad = [(k, ranges[k], hex(int(got[k])), hex(want[k])) for k in range(len(ranges)) if int(got[k]) != want[k]]
    assert not bad, bad[:8]


def packed(lengths, lead=0):
    off, out = lead, []
    for n in lengths:
        out.append((off, n))
        off += n
    return out, off


@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_lengths_around_every_threshold(parser, kind, order):
    lengths = list(LENGTHS)
    if order == "descending":
        lengths.reverse()
    elif order == "shuffled":
        np.random.default_rng(9).shuffle(lengths)
    ranges, total = packed(lengths)
    run(parser, content(kind, total), ranges)


@pytest.mark.parametrize("lead", range(16))
def test_every_alignment(parser, lead):
    """the same records `lead` bytes behind a 16-byte boundary (torch's allocations start on one), the last one at the buffer's end"""
    lengths = [n for n in LENGTHS if n <= 4097] + [16385, 40_001]
    ranges, total = packed(lengths, lead)
    run(parser, content("random", total, seed=lead), ranges)


@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
def test_one_long_record(parser, kind):
    data = content(kind, 300_001)
    run(parser, data, [(0, 300_001)])                                # alone: 19 pieces over several workgroups
    tiny, total = packed([3, 0, 17, 300_001, 1, 40, 255], lead=5)
    run(parser, content(kind, total), tiny)                          # between tiny ones, ending with the buffer


def test_five_thousand_tiny_records(parser):
    lengths = np.random.default_rng(4).integers(0, 41, 5000).tolist()
    ranges, total = packed(lengths)
    run(parser, content("random", total), ranges)


def test_overlapping_and_repeated_ranges(parser):
    data = content("random", 70_000)
    ranges = [(0, 70_000), (0, 70_000), (1, 69_999), (100, 300), (100, 300), (150, 20_000), (69_999, 1), (70_000, 0), (35_000, 35_000), (5, 0)]
    run(parser, data, ranges)


def test_last_record_ends_on_the_last_byte(parser):
    for n in (1, 255, 257, 4097, 16_385, 33_333):
        data = content("random", n + 7, seed=n)
        run(parser, data, [(7, n)])


def test_no_records_and_refusals(parser):
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    got, ms = parser.crc_dev(buf.data_ptr(), 64, np.zeros((0, 2), dtype=np.uint64))
    assert got.size == 0 and ms == 0                                 # nothing launched: no kernel time
    got, ms = parser.crc_dev(buf.data_ptr(), 64, [(3, 0), (64, 0)])
    assert got.tolist() == [0, 0] and ms == 0
    with pytest.raises(binding.SwsemError, match="outside the buffer"):
        parser.crc_dev(buf.data_ptr(), 64, [(0, 64), (60, 5)])
