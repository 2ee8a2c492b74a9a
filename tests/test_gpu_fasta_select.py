"""mbgc_fasta_match_headers_dev (k_fa_match_headers: what `mbgc-hip d --select-seq` chooses records with) through the ctypes mirror,
on torch buffers, against `pattern in header` over the same bytes: patterns at a header's first and last byte, equal to it, one
byte longer than it, split over two headers; headers of no bytes and shorter than the table's gram; patterns of one byte, with a
shared 8-byte prefix, prefixes of each other, given twice, 300 bytes long; a match that straddles the 64-position tile and the
256- and 4096-byte marks of a long header; the edge of a bit word; a list of thousands."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def blob_of(headers, last_ends_blob=False):
    """headers (bytes) -> (the blob as .headers holds them: '\\n' behind each — not behind the last one when last_ends_blob —, offsets, lengths)"""
    off, at = [], 0
    for h in headers:
        off.append(at)
        at += len(h) + 1
    blob = b"".join(h + b"\n" for h in headers)
    if last_ends_blob:
        blob = blob[:-1]
    return blob, off, [len(h) for h in headers]


def match(headers, patterns, last_ends_blob=False):
    """-> the chosen bits, after holding them to the oracle"""
    import torch
    from mbgc_amd import fasta
    blob, off, ln = blob_of(headers, last_ends_blob)
    # the buffer ends with the blob: what stands behind it is another allocation's
    buf = torch.from_numpy(np.frombuffer(blob if blob else b"\0", dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        got, ms = p.match_headers_dev(buf.data_ptr(), len(blob), off, ln, patterns)
    finally:
        p.close()
    want = np.array([any(q in h for q in patterns) for h in headers], dtype=bool)
    assert got.tolist() == want.tolist(), [(i, h[:60]) for i, h in enumerate(headers) if got[i] != want[i]][:10]
    return got


def test_edges_of_a_header():
    headers = [b"NC_000913.3 Escherichia coli K-12", b"plasmid pA", b"", b"abc", b"xyzK-12", b"NC_0009"]
    assert match(headers, [b"NC_000913"]).tolist() == [True, False, False, False, False, False]          # at byte 0
    assert match(headers, [b"coli K-12"]).tolist() == [True, False, False, False, False, False]          # ends on the last byte
    assert match(headers, [b"plasmid pA"]).tolist() == [False, True, False, False, False, False]         # the whole header
    assert not match(headers, [b"plasmid pA "]).any() and not match(headers, [b"plasmid pAN"]).any()     # one byte longer than it
    assert not match(headers, [b"abcd", b"abcx"]).any()                                                  # (a header shorter than the gram, m = 4)
    assert match(headers, [b"abc", b"longer than that"]).tolist() == [False, False, False, True, False, False]
    # bytes that occur only split over the end of header r and the start of header r + 1 (a header of no bytes between them too)
    assert not match(headers, [b"K-12plasmid"]).any() and not match(headers, [b"2p"]).any()
    assert not match(headers, [b"pAabc"]).any() and not match(headers, [b"abcxyzK"]).any()
    # the last header ends on the blob's last byte
    assert match(headers, [b"C_0009"], last_ends_blob=True).tolist() == [True, False, False, False, False, True]
    assert match(headers, [b"NC_0009"], last_ends_blob=True).tolist() == [True, False, False, False, False, True]
    assert not match(headers, [b"NC_00091"], last_ends_blob=True)[5]


def test_a_header_of_no_bytes_and_no_pattern_at_all():
    assert not match([b""], [b"a"]).any()
    assert not match([b"", b""], [b"\t", b"ab"]).any()
    assert not match([b"abc"], []).any()


def test_pattern_shapes():
    headers = [b"contig_0001 len=5", b"contig_0002 len=7", b"contig_00 short", b"scaffold|12|x", b"q"]
    assert match(headers, [b"7"]).tolist() == [False, True, False, False, False]                         # one byte: m = 1
    assert match(headers, [b"q", b"|"]).tolist() == [False, False, False, True, True]
    assert match(headers, [b"contig_0001", b"contig_0002 len=7"]).tolist() == [True, True, False, False, False]     # a shared 8-byte prefix
    assert match(headers, [b"contig_0002 len=8", b"contig_0002 len=7"]).tolist() == [False, True, False, False, False]
    assert match(headers, [b"contig_00", b"contig_0001"]).tolist() == [True, True, True, False, False]   # a prefix of another
    assert match(headers, [b"contig_0001 len=5 and more", b"contig_0001"]).tolist() == [True, False, False, False, False]
    assert match(headers, [b"scaffold|12", b"scaffold|12", b"len=5", b"len=5"]).tolist() == [True, False, False, True, False]   # the same twice


@pytest.mark.parametrize("at", [60, 250, 4090])
def test_a_match_across_the_marks_of_a_long_header(at):
    rng = np.random.default_rng(at)
    h = bytearray(rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), 5000).tobytes())
    needle = b"NEEDLE_0123"                                                          # bytes [at, at + 11): over byte 64, 256 or 4096
    h[at: at + len(needle)] = needle
    assert at < (64, 256, 4096)[(60, 250, 4090).index(at)] < at + len(needle)
    others = [bytes(rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), 5000).tobytes()), b"NEEDLE_012"]
    assert match([others[0], bytes(h), others[1]], [needle]).tolist() == [False, True, False]
    assert match([others[0], bytes(h), others[1]], [needle + b"4"]).tolist() == [False, False, False]


def test_a_pattern_of_300_bytes():
    rng = np.random.default_rng(300)
    h = rng.choice(np.frombuffer(b"acgtn ", dtype=np.uint8), 900).tobytes()
    pat = h[417: 717]
    assert match([h, h[:716], h[418:], h[417: 717]], [pat]).tolist() == [True, False, False, True]
    wrong_end = pat[:-1] + (b"A" if pat[-1:] != b"A" else b"C")
    assert not match([h], [wrong_end]).any()


def test_the_edge_of_a_bit_word():
    assert match([b"only one"], [b"one"]).tolist() == [True]
    headers = [b"record %d" % r for r in range(32)] + [b"record 32 x"]
    got = match(headers, [b"32 x"])
    assert got.tolist() == [False] * 32 + [True]


def test_thousands_of_patterns():
    """3000 distinct 10-byte patterns against 2000 headers, a known 50 of which hold one"""
    rng = np.random.default_rng(3000)
    headers = [b"seq%06d|sample %d|len=%d" % (r, r % 97, 1000 + r) for r in range(2000)]
    pats = [b"ACC_%06d" % (7 * k) for k in range(3000)]                                # none of them in a header
    assert len(set(pats)) == 3000 and all(len(q) == 10 for q in pats)
    hit = sorted(rng.choice(2000, 50, replace=False).tolist())
    for i, r in enumerate(hit):
        q = pats[59 * i]
        at = (0, len(headers[r]) - 3, 9)[i % 3]
        headers[r] = headers[r][:at] + q + headers[r][at:]
    got = match(headers, pats)
    assert np.flatnonzero(got).tolist() == hit
