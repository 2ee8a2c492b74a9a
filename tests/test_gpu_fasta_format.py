"""mbgc_fasta_format_dev (the inverse of the input stage, k_fa_format) against tests/_fastaout.py's restatement of the
reference's writeDNA: line lengths around the 16-byte lane step and the 4096-byte tile, empty sequences, long headers, every
alignment of the text, more tiles and records than one grid slice, the too-small buffer, and the way round through the parser."""
import numpy as np
import pytest

from _fastaout import format_fasta

pytestmark = pytest.mark.gpu
LINES = [0, 1, 7, 60, 80, 4095, 4096, 4097, 2 ** 32 + 5]
HEADERS = [0, 1, 15, 16, 17, 5000]
GUARD = 0xA5


def seq_lengths(line):
    L = line if 0 < line < 2 ** 32 else 61
    return sorted({0, 1, L - 1, L, L + 1, 3 * L, 3 * L + 1})


def make_records(rng, lens, hdrs):
    return [(bytes(rng.integers(32, 127, h).astype(np.uint8)), bytes(rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), n)))
            for n, h in zip(lens, hdrs)]


def run_format(units, shift=0, cap=None, tail=64):
    """units: [(records, line_len)] -> (text bytes as written, offsets, the whole buffer with its guard bytes)"""
    import torch
    from mbgc_amd import fasta
    seqs, heads, rows = bytearray(), bytearray(), []
    for records, line in units:
        for h, s in records:
            rows.append((len(seqs), len(s), len(heads), len(h), line))
            seqs += s
            heads += h
    want = len(b"".join(format_fasta(r, l) for r, l in units))
    cap = want if cap is None else cap
    dseq = torch.from_numpy(np.frombuffer(bytes(seqs) + b"\0", dtype=np.uint8).copy()).to("cuda:0")
    dhdr = torch.from_numpy(np.frombuffer(bytes(heads) + b"\0", dtype=np.uint8).copy()).to("cuda:0")
    buf = torch.full((shift + cap + tail + 16,), GUARD, dtype=torch.uint8, device="cuda:0")
    base = (-buf.data_ptr()) % 16 + shift                           # the text starts `shift` bytes behind a 16-byte boundary
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        offs, _ = p.format_dev(dseq.data_ptr(), len(seqs), dhdr.data_ptr(), len(heads), np.array(rows, dtype=np.uint64).reshape(-1, 5),
                               buf.data_ptr() + base, cap)
    finally:
        p.close()
    whole = buf.cpu().numpy()
    assert (whole[:base] == GUARD).all() and (whole[base + cap:] == GUARD).all()      # nothing outside the buffer
    return whole[base: base + int(offs[-1])].tobytes(), offs, whole


def check(units, shift=0):
    text, offs, _ = run_format(units, shift)
    want = b"".join(format_fasta(r, l) for r, l in units)
    assert len(text) == len(want) and text == want
    at, k = 0, 0
    for records, line in units:
        for rec in records:
            assert int(offs[k]) == at
            at += len(format_fasta([rec], line))
            k += 1
    assert int(offs[k]) == at == len(want)


@pytest.mark.parametrize("line", LINES)
def test_line_lengths(line):
    rng = np.random.default_rng(line % 1000 + 3)
    lens = seq_lengths(line) + [20_000]                              # the last spans more than four tiles
    hdrs = [HEADERS[i % len(HEADERS)] for i in range(len(lens))]
    check([(make_records(rng, lens, hdrs), line)])
    check([(make_records(rng, lens[::-1], hdrs), line), (make_records(rng, [5, 0, 300], [3, 0, 17]), 60)])     # two units, two line lengths


@pytest.mark.parametrize("hdr", HEADERS)
def test_header_lengths(hdr):
    rng = np.random.default_rng(hdr + 11)
    check([(make_records(rng, [0, 1, 79, 80, 81, 0, 4096], [hdr] * 7), 80)])
    check([(make_records(rng, [0, 0, 0], [hdr] * 3), 0)])           # headers only: no blank lines


def test_every_start_residue_and_buffer_alignment():
    rng = np.random.default_rng(5)
    for shift in range(16):                                          # the buffer's head and tail are stored byte by byte
        first = make_records(rng, [shift], [shift])                  # moves the start of the second record through every residue
        check([(first + make_records(rng, [500, 0, 33], [9, 2, 40]), 70)], shift)


def test_more_records_and_tiles_than_a_grid_slice():
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 4, 70_000)
    recs = make_records(rng, lens.tolist(), (lens % 3).tolist())
    check([(recs, 2)])
    # more than 65 535 tiles of text: one record of 3.4 M lines. The expectation of that size is laid out with numpy (the
    # restatement's loop takes seconds there) and held to the restatement on its first lines.
    lines, width = 65_536 * 4096 // 81 + 100, 80
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), lines * width + 17)
    body = np.concatenate([seq[:lines * width].reshape(lines, width), np.full((lines, 1), 10, dtype=np.uint8)], axis=1).ravel()
    want = b">long\n" + body.tobytes() + seq[lines * width:].tobytes() + b"\n"
    assert want[:6 + 81 * 50] == format_fasta([(b"long", seq[:50 * width].tobytes())], width)
    assert len(want) > 65_536 * 4096
    import torch
    from mbgc_amd import fasta
    dseq = torch.from_numpy(seq).to("cuda:0")
    dhdr = torch.from_numpy(np.frombuffer(b"long", dtype=np.uint8).copy()).to("cuda:0")
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    offs, _ = p.format_dev(dseq.data_ptr(), seq.size, dhdr.data_ptr(), 4, np.array([(0, seq.size, 0, 4, width)], dtype=np.uint64),
                           buf.data_ptr(), len(want))
    p.close()
    assert int(offs[1]) == len(want)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:len(want)], np.frombuffer(want, dtype=np.uint8)) and (got[len(want):] == GUARD).all()


def test_text_buffer_too_small():
    from mbgc_amd import fasta
    rng = np.random.default_rng(7)
    units = [(make_records(rng, [100, 0, 9000], [5, 6, 7]), 60)]
    want = b"".join(format_fasta(r, l) for r, l in units)
    for cap in (0, 1, len(want) - 1):
        with pytest.raises(fasta.TextTooSmall) as e:
            run_format(units, cap=cap)
        assert e.value.needed == len(want)
    import torch
    # the call that fails writes nothing at all: the buffer keeps its pattern (run_format checks the guard bytes around it only
    # after a success, so look here)
    seqs = b"".join(s for _, s in units[0][0])
    heads = b"".join(h for h, _ in units[0][0])
    rows, a, b = [], 0, 0
    for h, s in units[0][0]:
        rows.append((a, len(s), b, len(h), 60)); a += len(s); b += len(h)
    dseq = torch.from_numpy(np.frombuffer(seqs, dtype=np.uint8).copy()).to("cuda:0")
    dhdr = torch.from_numpy(np.frombuffer(heads, dtype=np.uint8).copy()).to("cuda:0")
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    p = fasta.FastaParser()
    with pytest.raises(fasta.TextTooSmall):
        p.format_dev(dseq.data_ptr(), len(seqs), dhdr.data_ptr(), len(heads), np.array(rows, dtype=np.uint64), buf.data_ptr(), len(want) - 1)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()
    offs, _ = p.format_dev(dseq.data_ptr(), len(seqs), dhdr.data_ptr(), len(heads), np.array(rows, dtype=np.uint64), buf.data_ptr(), len(want))
    p.close()
    whole = buf.cpu().numpy()
    assert whole[:len(want)].tobytes() == want and (whole[len(want):] == GUARD).all()


def test_records_outside_their_buffers_are_refused():
    import torch
    from mbgc_amd import binding, fasta
    d = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    p = fasta.FastaParser()
    for row in ((60, 5, 0, 1, 80), (0, 5, 64, 1, 80), (2 ** 64 - 1, 2, 0, 0, 0)):
        with pytest.raises(binding.SwsemError):
            p.format_dev(d.data_ptr(), 64, d.data_ptr(), 64, np.array([row], dtype=np.uint64), d.data_ptr(), 64)
    p.close()


def test_device_round_trip():
    """parse(format(x)) == x on the device: contigs, records, dnaLineLen, status 0"""
    import torch
    from mbgc_amd import fasta
    rng = np.random.default_rng(8)
    for line, lens in ((80, [400, 81, 80, 1, 0, 7000]), (0, [50, 0, 3]), (7, [7, 14, 6, 22]), (4097, [3 * 4097 + 1, 4097, 12])):
        recs = make_records(rng, lens, [int(x) for x in rng.integers(0, 40, len(lens))])
        recs = [(h.replace(b">", b"-"), s) for h, s in recs]
        text, _, _ = run_format([(recs, line)])
        dev = torch.from_numpy(np.frombuffer(text + b"\0", dtype=np.uint8).copy()).to("cuda:0")
        out = torch.zeros(len(text), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        p = fasta.FastaParser()
        r = p.parse_batch_dev(dev.data_ptr(), np.array([0, len(text)], dtype=np.uint64), out.data_ptr(), out.numel())
        p.close()
        assert int(r["status"][0]) == 0
        seq = out.cpu().numpy().tobytes()
        got = [(text[int(x["headerOff"]): int(x["headerOff"] + x["headerLen"])], seq[int(x["seqOff"]): int(x["seqOff"] + x["seqLen"])])
               for x in r["records"]]
        assert got == recs
        assert seq[: int(r["seq_base"][1])] == b"".join(s for _, s in recs)
        has_full_line = any(len(s) > line for _, s in recs) if line else False
        assert int(r["dna_line_len"][0]) == (line if has_full_line else 0)


def test_gather_packs_pieces_with_their_separator():
    """mbgc_fasta_gather_dev (the header lines of a `c -i` batch): empty pieces, pieces longer than a workgroup's stride, more
    pieces than one grid slice, and a piece outside the buffer"""
    import torch
    from mbgc_amd import binding, fasta
    rng = np.random.default_rng(12)
    src = rng.integers(0, 256, 200_000).astype(np.uint8)
    dev = torch.from_numpy(src).to("cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    lens = np.concatenate([[0, 1, 255, 256, 257, 5000], rng.integers(0, 4, 70_000)]).astype(np.uint64)
    offs = rng.integers(0, src.size - 5000, lens.size).astype(np.uint64)
    got = p.gather_dev(dev.data_ptr(), src.size, offs, lens)
    want = b"".join(src[int(o): int(o + n)].tobytes() + b"\n" for o, n in zip(offs, lens))
    assert got == want
    assert p.gather_dev(dev.data_ptr(), src.size, [], []) == b""
    with pytest.raises(binding.SwsemError):
        p.gather_dev(dev.data_ptr(), src.size, [src.size - 3], [4])
    p.close()
