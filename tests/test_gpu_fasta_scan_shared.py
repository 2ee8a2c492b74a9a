"""What stats_dev, find_dev, sketch_dev, dups_dev and crc_dev share on one FastaParser: the device copies of the records and of their
tiles' prefix sum, the pair of events, the check of the ranges and the empty answers. One text of two tiles and a byte, seen from a
base address that is 5 modulo 16, and a handful of records at the grid's edges; the five calls one after the other on one parser, then
in the reverse order, each answer held against the same call on a parser of its own; the refusal of a record that ends one byte behind
the buffer, with its message, and the next call's answer; no record, and records without a byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TILE = 4096
N = 2 * TILE + 1
SHIFT = 5
CALLS = ("stats", "find", "sketch", "dups", "crc")


def text():
    rng = np.random.default_rng(20)
    t = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, N)].copy()
    grid = TILE - SHIFT                                              # the text offset of the first tile boundary of a record that starts at 0
    t[grid - 21:grid + 31] = ord("A")
    t[grid - 20:grid + 30] = ord("N")                                # one run of N across it, of 50 bytes
    t[5000:5064] = t[100:164]                                        # two records of the same bytes
    return t


RECORDS = [(50, 0),                  # empty
           (77, 1),                  # one byte
           (N - 300, 300),           # ends on the buffer's last byte
           (10, 2 * TILE - 20),      # spans both tile boundaries
           (100, 64), (100, 64),     # the same record listed twice
           (5000, 64)]               # ... and its bytes once more, elsewhere
OUTSIDE = (N - 9, 10)                # off + len = seq_bytes + 1
REFUSAL = {"stats": "stats: record 2 lies outside the buffer", "find": "find: record 2 lies outside the buffer",
           "sketch": "sketch: record 2 lies outside the buffer", "dups": "dups: record 2 lies outside the buffer",
           "crc": "crc: range 2 lies outside the buffer"}


@pytest.fixture(scope="module")
def device():
    import torch
    host = text()
    whole = torch.from_numpy(np.concatenate([np.zeros(SHIFT, dtype=np.uint8), host])).to("cuda:0")
    view = whole[SHIFT:]
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == SHIFT and view.numel() == N
    return view, host


def call(p, name, ptr, host, records):
    """one of the five calls -> its answer without the kernel's ms, as a tuple of arrays and numbers"""
    n = len(records)
    if name == "stats":
        return p.stats_dev(ptr, N, records)[:2]
    if name == "find":
        return p.find_dev(ptr, N, records, [host[120:128].tobytes()], max_mismatches=0)[:1]
    if name == "sketch":
        return p.sketch_dev(ptr, N, records, np.arange(n, dtype=np.uint32) % 3, 3, k=5, max_hash=2 ** 64 - 1)[:3]
    if name == "dups":
        return p.dups_dev(ptr, N, records)[:2]
    return p.crc_dev(ptr, N, records)[:1]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


@pytest.fixture(scope="module")
def fresh(device):
    """every call's answer on a parser of its own: computed once, compared against and never changed"""
    from mbgc_amd import fasta
    view, host = device
    out = {}
    for name in CALLS:
        p = fasta.FastaParser()
        try:
            out[name] = call(p, name, view.data_ptr(), host, RECORDS)
        finally:
            p.close()
    return out


def test_the_fresh_answers_are_not_trivial(fresh):
    counts, runs = fresh["stats"]
    assert [int(c[:6].sum()) for c in counts] == [ln for _, ln in RECORDS]
    assert any(int(r["rec"]) == 3 and int(r["cls"]) == 0 and int(r["start"]) == TILE - SHIFT - 20 - 10 and int(r["len"]) == 50 for r in runs)
    hits = fresh["find"][0]
    assert {int(h["rec"]) for h in hits} >= {3, 4, 5, 6}
    hashes, start, kmers = fresh["sketch"]
    assert hashes.size and int(start[-1]) == hashes.size and int(kmers.sum()) > 0
    dups, classes = fresh["dups"]
    assert [int(d["rep"]) for d in dups][4:] == [4, 4, 4] and 1 < classes < len(RECORDS)
    crc = fresh["crc"][0]
    assert crc[0] == 0 and crc[4] == crc[5] == crc[6] != 0


def test_one_parser_forwards_then_backwards(device, fresh):
    from mbgc_amd import fasta
    view, host = device
    p = fasta.FastaParser()
    try:
        for name in CALLS + CALLS[::-1]:
            got = call(p, name, view.data_ptr(), host, RECORDS)
            assert same(got, fresh[name]), name
    finally:
        p.close()


@pytest.mark.parametrize("name", CALLS)
def test_a_record_one_byte_past_the_buffer_is_refused_and_the_next_call_is_right(device, fresh, name):
    from mbgc_amd import binding, fasta
    view, host = device
    assert OUTSIDE[0] + OUTSIDE[1] == N + 1
    p = fasta.FastaParser()
    try:
        with pytest.raises(binding.SwsemError) as e:
            call(p, name, view.data_ptr(), host, RECORDS[:2] + [OUTSIDE] + RECORDS[2:])
        assert str(e.value) == REFUSAL[name]
        assert same(call(p, name, view.data_ptr(), host, RECORDS), fresh[name])
    finally:
        p.close()


@pytest.mark.parametrize("name", CALLS)
def test_no_record_and_records_without_a_byte(device, name):
    from mbgc_amd import fasta
    view, host = device
    p = fasta.FastaParser()
    try:
        none = call(p, name, view.data_ptr(), host, [])
        hollow = call(p, name, view.data_ptr(), host, [(0, 0), (N, 0), (77, 0)])
    finally:
        p.close()
    if name == "stats":
        assert none[0].shape == (0, 8) and none[1].size == 0
        assert hollow[0].shape == (3, 8) and not hollow[0].any() and hollow[1].size == 0
    elif name == "find":
        assert none[0].size == 0 and hollow[0].size == 0
    elif name == "sketch":
        for hashes, start, kmers in (none, hollow):
            assert hashes.size == 0 and start.tolist() == [0, 0, 0, 0] and kmers.tolist() == [0, 0, 0]
    elif name == "dups":
        assert none[0].size == 0 and none[1] == 0
        assert [(int(d["rep"]), int(d["strand"])) for d in hollow[0]] == [(0, 0)] * 3 and hollow[1] == 1
    else:
        assert none[0].size == 0 and hollow[0].tolist() == [0, 0, 0]
