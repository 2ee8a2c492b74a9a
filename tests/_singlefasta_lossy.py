"""Single fasta file mode under the lossy rule (`mbgc c -L -i`, `mbgc-hip c --lossy-file`), restated from the reference and not from
the kernels. The byte stream is cut by mgmpInSplit_next exactly as without -L (MultipleGenomeMatchingProcessor.cpp:73-76,489-506:
the split never looks at allowLossyParsing), and KSEQ_READ (:9-10) reads every element with kseq_read_lossy as if it were a file
of its own; under the sequential schedule the whole file is ONE target read by one kseq_read_lossy (mgmpInReset(firstFp), :247).
split_records restates what mbgc_fasta_split_buf_dev2 has to return. Test infrastructure only."""
import numpy as np

import _singlefasta as sfa
from _fasta_lossy import lossy_parse
from _fastaout import format_fasta

LINE_START, AT = 1, 2                                                # MBGC_FASTA_SPLIT_LINE_START, MBGC_FASTA_SPLIT_AT


def rounds(data, upper=False):
    """the parallel schedule: [lossy_parse of element 0 (the initial reference), of element 1 (the first target), ...]"""
    return [lossy_parse(e, upper) for e in sfa.elements(data)]


def sequential(data, upper=False):
    """the sequential schedule: the file is one target"""
    return lossy_parse(data, upper)


def rounds_text(data):
    """what comes back from a parallel-schedule archive: every element's records at that element's own line length"""
    return b"".join(format_fasta(p["records"], p["dna_line_len"]) for p in rounds(data))


def sequential_text(data):
    p = sequential(data)
    return format_fasta(p["records"], p["dna_line_len"])


def split_records(data, start, mins, flags, is_file_end=True, max_elems=None):
    """sfa.split_window over a buffer, from `start`, with a rule for what a mark is: the ends (offsets in the buffer) of the
    elements; an element ends at the first mark at or behind its start + minimum (mins: one number, or (first, next)).
    LINE_START: a mark counts only at offset 0 of the buffer or right behind a line feed; AT: '@' is a mark beside '>'."""
    first_min, next_min = (mins, mins) if isinstance(mins, int) else mins
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    mark = a == 0x3E
    if flags & AT:
        mark = mark | (a == 0x40)
    if flags & LINE_START and a.size:
        mark = mark & np.concatenate(([True], a[:-1] == 0x0A))
    at = np.flatnonzero(mark)
    ends, s, n = [], start, len(data)
    while s != n and (max_elems is None or len(ends) < max_elems):
        thr = s + (next_min if ends else first_min)
        k = int(np.searchsorted(at, thr)) if thr < n else at.size
        if k == at.size:
            if not is_file_end:
                break
            e = n
        else:
            e = int(at[k])
        ends.append(e)
        s = e
    return ends


# ---- damaged single files: a `cat` of assemblies written by different tools
def styled(contigs, first_id, widths, eol=b"\n", marker=b">", tag=b""):
    """contigs (uint8 arrays of bases) as FASTA text: lines of widths[0], widths[1], ... bases in turn"""
    out = bytearray()
    for j, c in enumerate(contigs):
        out += marker + ("seq%05d %s" % (first_id + j, "part")).encode() + tag + eol
        s, at, k = c.tobytes(), 0, 0
        while at < len(s):
            w = widths[k % len(widths)]
            out += s[at:at + w] + eol
            at += w
            k += 1
    return bytes(out)


STYLES = 6


def damaged_part(contigs, first_id, style):
    """one assembly, damaged in the way `style` names; no '+' at a line start, no CR that stays in a sequence (a CR-only line
    stands behind a record's first line only), headers of at least one byte"""
    if style == 0:                                                   # the widest lines of the file, LF
        return styled(contigs, first_id, [100])
    if style == 1:                                                   # CRLF throughout
        return styled(contigs, first_id, [80], b"\r\n")
    if style == 2:                                                   # ragged, with empty lines
        return styled(contigs, first_id, [70, 61, 70, 33]).replace(b"AC\nG", b"AC\n\n\nG")
    if style == 3:                                                   # '@' headers, CRLF
        return styled(contigs, first_id, [60], b"\r\n", b"@")
    if style == 4:                                                   # a '>' and an '@' inside the header lines; some lines end CRLF
        return styled(contigs, first_id, [90], tag=b" a -> b, c@d >x").replace(b"GT\nA", b"GT\r\nA")
    t = styled(contigs, first_id, [50, 50, 49])                      # CR-only and empty lines behind a record's first line
    return t.replace(b"TTA\n", b"TTA\n\r\n\n")


JUNK = b"# assembled by hand\r\n\r\nno marker in these lines\n   "  # in front of the file's first '>', which stands inside a line


def damaged_single(parts, junk=JUNK):
    """parts: lists of contigs, one per assembly -> the file. Part 0 is written in style 0 and no other part is, so the first
    record holds the file's longest line and the elements behind part 0 have a shorter longest line than the file."""
    out, first_id = bytearray(junk), 0
    for p, contigs in enumerate(parts):
        out += damaged_part(contigs, first_id, 1 + (p - 1) % (STYLES - 1) if p else 0)
        first_id += len(contigs)
    return bytes(out)


def damaged_listeria(texts):
    """the golden fixture's input (tests/golden/make_single_fasta_lossy_golden.py): the bundled genomes' FASTA texts, each parsed
    and written again in another style, concatenated behind JUNK"""
    out, first_id = bytearray(JUNK), 0
    for p, t in enumerate(texts):
        recs = lossy_parse(t)["records"]
        contigs = [np.frombuffer(s, dtype=np.uint8) for _, s in recs]
        part = damaged_part(contigs, first_id, (1, 2, 3)[p % 3])
        if p == 0:                                                   # the first record keeps lines of 100: the longest of the file
            part = styled(contigs[:1], first_id, [100]) + damaged_part(contigs[1:], first_id + 1, 1)
        out += part
        first_id += len(contigs)
    return bytes(out)


def synth_single(total, nparts, seed, junk=JUNK):
    """a damaged single file of about `total` bytes: nparts related assemblies of three contigs each"""
    from mbgc_amd import synth
    base = synth.base_codes(total // nparts, seed)
    parts = []
    for p in range(nparts):
        g = synth.genome(base, p, 0.01)
        cuts = [0, g.size // 5 + 13 * p, g.size // 2 + 7 * p, g.size]
        parts.append([g[a:b] for a, b in zip(cuts, cuts[1:])])
    return damaged_single(parts, junk)
