"""The lossy FASTA rule (`mbgc c -L`, `mbgc-hip c --lossy`) restated byte by byte from the reference's kseq_read_lossy
(utils/kseq.h:282-333) and ks_getuntil2 (:100-150, the `loosy` strip at :147) — not from the kernels. One kseq_t per file:
maxLastDnaLineLen runs over all records of the file. The FASTQ branch (:320-332) is not restated: a '+' where a sequence line
could start ends the file with EFASTQ. Test infrastructure only."""
from _fastaout import format_fasta

EFASTQ = -16
MARKERS = (0x3E, 0x40)                                               # '>' '@'


def _line(data, pos):
    """ks_getuntil2(KS_SEP_LINE) from pos: (the bytes up to the next newline, the position behind it)"""
    e = data.find(b"\n", pos)
    return (data[pos:], len(data)) if e < 0 else (data[pos:e], e + 1)


def lossy_parse(data, upper=False):
    """-> dict(status, records=[(header bytes, sequence bytes)], dna_line_len, seq=all sequences back to back)"""
    data = bytes(data)
    n, pos = len(data), 0
    records, longest, status = [], 0, 0
    while pos < n and data[pos] not in MARKERS:                      # :288, anywhere in the file
        pos += 1
    pos += 1                                                         # last_char = the marker
    while pos < n:                                                   # (a marker on the last byte: ks_getuntil returns -1, :293)
        name, pos = _line(data, pos)
        if len(name) > 1 and name.endswith(b"\r"):                   # :147
            name = name[:-1]
        seq, b, c = bytearray(), 0, -1
        while pos < n:                                               # :299
            c = data[pos]
            pos += 1
            if c in (0x3E, 0x2B, 0x40):
                break
            if c == 0x0A:
                c = -1
                continue
            if len(seq) > b:
                longest = max(longest, len(seq) - b)
            b = len(seq)
            seq.append(c)
            if pos < n:                                              # (nothing behind the byte: -1 at :143, before the strip)
                rest, pos = _line(data, pos)
                seq += rest
                if len(seq) > 1 and seq[-1] == 0x0D:
                    seq.pop()
            c = -1
        if len(seq) > b:
            longest = max(longest, len(seq) - b)
        records.append((name, bytes(seq).upper() if upper else bytes(seq)))
        if c == 0x2B:
            status = EFASTQ
            break
        if c not in MARKERS:
            break
    return dict(status=status, records=records, dna_line_len=longest if status == 0 else 0, seq=b"".join(s for _, s in records))


def normalise(data, upper=False):
    """the FASTA text the reference's `mbgc d` writes for this file of a -L archive"""
    p = lossy_parse(data, upper)
    assert p["status"] == 0
    return format_fasta(p["records"], p["dna_line_len"])


def _g(n, seed=7):
    x, out = seed, bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(b"ACGT"[(x >> 16) & 3])
    return bytes(out)


G = _g(3000)
FILE_A = b">a one\r\n" + G[0:70] + b"\r\n" + G[70:100] + b"\r\n\r\n" + G[100:3000] + b"\r\n>b\n\r\nAC\n"
FILE_B = (b"junk line\nxx>b1 hdr\n" + G[:500] + b"\n" + G[500:560] + b"\n\n" + G[560:2000] + b"\n@q1\n" + G[2000:2100] +
          b"\n>e\n>f\r\n\rA\n")

# the EDGE list of tests/test_fasta_input.py (kept in step by test_fasta_lossy.py)
EDGE_LOSSLESS = [
    b"", b">", b">h", b">h\n", b">h\nACGT", b">h\nACGT\n", b">h\nACGT\nAC\n", b">h\nAC\nACGT\n",
    b">h\nACGT\nACGT\n>g\nACGT\nA\n>k\nAC\n", b">h\nACGT\nACG\nACGT\n", b">h\nACGT\n\nACGT\n", b">h\nACGT\n\n", b">h\n\n>g\nAC\n",
    b"ACGT\n>h\nAC\n", b"\n>h\nAC\n", b">h\nAC>GT\nACTT\n", b">h\nACGT\n>g\n>k\nACGT\n", b">a b c\tdef\r\nACGT\r\nAC\r\n",
    b">h\nacgtnACGT\nry\n", b">h\nA\nC\nG\n>g\nTT\n", b">h\nAAAA\n>g\nCC\nCC\n",
    bytes([62, 104, 10, 200, 65, 255, 10, 65, 66, 10]),
]

EDGE_LOSSY = [FILE_A, FILE_B] + EDGE_LOSSLESS + [
    b">x y\r\nACGT\r\nACGT\r\nAC\r\n>z\r\nTT\r\n",                  # CRLF throughout
    b">x y\r\nACGT\r\nACGT\r\nAC\r\n>z\r\nTT",                      # ... without the last line end
    b">\r\n",                                                        # a header that is one CR keeps it
    b">\r\nAC\r\n",
    b">h\r",                                                         # header, CR, end of file
    b">\r",
    b">h\n\r\nACGT\n",                                               # a CR-only line first in a record: its byte stays
    b">h\n\n\n\r\n\nACGT\n",                                         # ... behind empty lines too
    b">h\nACGT\n\r\nAC\n",                                           # later in a record: nothing
    b">h\n\r\n\r\nAC\n>g\nA\n\n\r\n",                               # the second one goes, in both records
    b">h\n\r\r\nAC\n",                                               # CR CR first in a record: one stays
    b">h\nAC\r\r\nGT\n",                                             # one CR of two goes
    b">h\nA\r\n",                                                    # X CR always loses the CR
    b">h\nACGT\n\r",                                                 # a lone CR as the file's last byte stays, in a long record too
    b">h\n\r",
    b">h\nACGT\nA\r",                                                # ... but not behind another byte of its line
    b">h\nACGT\r",
    b">h\nACGT\n>",                                                  # a marker as the last byte starts no record
    b">h\nACGT\n@",
    b"@",
    b"no marker in here\nat all\n",                                  # junk only: no records, status 0
    b"\n\n\r\n",
    b"junk > h\nACGT\n",                                             # the marker in the middle of a line
    b"\r\n\r\n>h\nACGT\n",
    b"xx@h\nAC\n",
    b"@r1\nACGT\nAC\n@r2\nTT\n",                                     # '@' records
    b">h\nAC@GT\n@g\nA>C\n",                                         # markers inside a line are sequence
    b"@r1\nACGT\n+\nIIII\n",                                         # FASTQ
    b">h\nACGT\n+x\n",
    b">h\n+\n",
    b">h\n\n+\n",
    b">+h\nAC+GT\nA+\n",                                             # '+' elsewhere is a byte like any other
    b"+ junk\n>h\nAC\n",
    bytes([200, 201, 62, 104, 200, 13, 10, 200, 65, 255, 13, 10, 13, 10, 65, 66, 10]),     # bytes >= 0x80
    b">h\nacgt\r\nnnRY\r\n",                                         # -U composes
    b">h\nA\n>g\nACGTACGT\n>k\nAC\n",                               # the longest line wins wherever it stands
]
