"""The referee of mbgc_fasta_find_dev and `mbgc-hip f`: a brute-force search in numpy, written from the contract alone. A hit is (rec,
pos, pattern, mismatches): the pattern lies inside the record at pos, and at most K of its positions differ after letters are folded
to upper case (fold(b) = b & 0xDF for an ASCII letter, b otherwise). No table, no seed, no tile: per (record, pattern) the mismatches
of every start are counted, a column of the pattern at a time."""
import numpy as np


def fold(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    letter = ((a | 0x20) >= ord("a")) & ((a | 0x20) <= ord("z"))
    a[letter] &= 0xDF
    return a


def hits_in(text, pattern, k):
    """folded arrays -> [(pos, mismatches)] of every start of `pattern` in `text` with at most k mismatches"""
    n, m = text.size, pattern.size
    if m > n:
        return []
    starts = n - m + 1
    if k == 0:
        # (exact search: bytes.find over the folded bytes, restarted one byte behind every hit so that overlapping ones count)
        tb, pb, out, at = text.tobytes(), pattern.tobytes(), [], 0
        while (at := tb.find(pb, at)) >= 0:
            out.append((at, 0))
            at += 1
        return out
    d = np.zeros(starts, dtype=np.int32)
    for j in range(m):
        d += text[j:j + starts] != pattern[j]
    return [(int(p), int(d[p])) for p in np.flatnonzero(d <= k)]


def brute_force(buf, ranges, patterns, k=0):
    """buf: the buffer's bytes; ranges: (off, len) per record; patterns: bytes objects -> sorted [(rec, pos, pattern, mismatches)]"""
    folded = fold(buf)
    pats = [fold(p) for p in patterns]
    out = []
    for r, (off, ln) in enumerate(ranges):
        text = folded[int(off):int(off) + int(ln)]
        for q, p in enumerate(pats):
            out += [(r, pos, q, d) for pos, d in hits_in(text, p, k)]
    return sorted(out)


COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def reverse_complement(seq):
    """upper-case A, C, G, T, N only: what the queries of the tests are made of"""
    return bytes(seq).translate(COMPLEMENT)[::-1]


def cli_lines(files, queries, k=0, forward_only=False):
    """files: [(name, [(header line, sequence bytes)])] in collection order; queries: [(name, bases)] -> the TSV lines of `mbgc-hip f`:
    query, file, record, start, end, strand, mismatches; by file, record, start, query, + before -"""
    rows = []
    for f, (name, records) in enumerate(files):
        for r, (header, seq) in enumerate(records):
            text = fold(seq)
            for q, (qname, bases) in enumerate(queries):
                bases = bytes(bases).upper()
                strands = [(0, "+", bases)]
                if not forward_only and reverse_complement(bases) != bases:
                    strands.append((1, "-", reverse_complement(bases)))
                for order, strand, pat in strands:
                    for pos, d in hits_in(text, fold(pat), k):
                        rows.append((f, r, pos + 1, q, order, "\t".join([qname, name, header.split()[0], str(pos + 1), str(pos + len(pat)), strand, str(d)])))
    return [row[-1] for row in sorted(rows)]
