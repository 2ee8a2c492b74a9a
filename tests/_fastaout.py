"""What `mbgc-hip d --fasta` must write, restated: the header line, then the reference's writeDNA (MBGC_Decoder.cpp:76-92). The
single expectation of the format tests. Test infrastructure only."""


def format_fasta(records, line_len):
    """records: [(header bytes, sequence bytes)]; line_len: bytes per line, 0 = every sequence on one line"""
    out = bytearray()
    for header, seq in records:
        out += b">" + header + b"\n"
        width = line_len if line_len else max(len(seq), 1)
        for i in range(0, len(seq), width):        # full lines, then the remainder; nothing for an empty sequence
            out += seq[i:i + width] + b"\n"
    return bytes(out)
