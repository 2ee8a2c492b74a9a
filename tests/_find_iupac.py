"""The referee of mbgc_fasta_find_iupac_dev, `mbgc-hip f --iupac` and `f --primers`: a brute-force search in numpy, written from the
contract alone. The set of a pattern letter, either case: A, C, G, T (U as T); R = AG, Y = CT, S = CG, W = AT, K = GT, M = AC; B = CGT,
D = AGT, H = ACT, V = ACG; N = ACGT. A text byte has a base only if it is one of acgtuACGTU; position j matches iff the text byte has a
base and that base is in the pattern letter's set — a text N matches nothing. A hit is (rec, pos, pattern, mismatches): the pattern
lies inside the record at pos and at most K positions do not match. No table, no seed, no window, no tile: per (record, pattern) the
mismatches of every start are counted, a column of the pattern at a time."""
import numpy as np

SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
        "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
              "S": "S", "W": "W", "N": "N"}

# byte -> the bit of its base (A 1, C 2, G 4, T 8), 0 for a byte without one
BASE = np.zeros(256, dtype=np.uint8)
for _i, _b in enumerate("ACGT"):
    BASE[ord(_b)] = BASE[ord(_b.lower())] = 1 << _i
BASE[ord("U")] = BASE[ord("u")] = 8


def letter_set(letter):
    """the pattern letter (a byte) -> the bits of the bases in its set"""
    return sum(1 << i for i, b in enumerate("ACGT") if b in SETS[chr(letter).upper()])


def hits_in(text, pattern, k):
    """text: uint8 array, pattern: bytes -> [(pos, mismatches)] of every start with at most k positions that do not match"""
    n, m = text.size, len(pattern)
    if m > n:
        return []
    starts = n - m + 1
    has = BASE[text]
    d = np.zeros(starts, dtype=np.uint8 if m < 256 else np.int32)
    for j, letter in enumerate(pattern):
        d += (has[j:j + starts] & np.uint8(letter_set(letter))) == 0
    return [(int(p), int(d[p])) for p in np.flatnonzero(d <= k)]


_NEAR = {}


def hits_of_record(seq, pattern, k):
    """hits_in for a record of `files` (a bytes object that lives as long as the test module): the starts with at most 3 mismatches —
    the most any call allows — are counted once per (record, pattern) and kept; a smaller k takes its part of them"""
    key = (id(seq), len(seq), bytes(pattern))
    if key not in _NEAR:
        _NEAR[key] = hits_in(np.frombuffer(bytes(seq), dtype=np.uint8), bytes(pattern), 3)
    return [(p, d) for p, d in _NEAR[key] if d <= k]


def brute_force(buf, ranges, patterns, k=0):
    """buf: the buffer's bytes; ranges: (off, len) per record; patterns: bytes objects -> sorted [(rec, pos, pattern, mismatches)]"""
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    out = []
    for r, (off, ln) in enumerate(ranges):
        text = a[int(off):int(off) + int(ln)]
        for q, p in enumerate(patterns):
            out += [(r, pos, q, d) for pos, d in hits_in(text, bytes(p), k)]
    return sorted(out)


def expansion(window):
    """the concrete sequences a run of pattern letters stands for"""
    n = 1
    for letter in bytes(window):
        n *= len(SETS[chr(letter).upper()])
    return n


def table_rows(patterns, k):
    """the rows of the seed table by the contract: per pattern and per segment j of len // (k + 1) letters at j * (len // (k + 1)), the
    expansion of the segment's cheapest window of 8 letters"""
    rows = 0
    for p in patterns:
        step = len(p) // (k + 1)
        for j in range(k + 1):
            rows += min(expansion(p[j * step + w:j * step + w + 8]) for w in range(step - 7))
    return rows


def window_grams(window):
    """every concrete gram a window of 8 letters stands for, base i in bits [2 i, 2 i + 2) (A 0, C 1, G 2, T 3)"""
    grams = [0]
    for i, letter in enumerate(bytes(window)):
        grams = [g | "ACGT".index(b) << (2 * i) for g in grams for b in SETS[chr(letter).upper()]]
    return grams


def rows_walked(buf, ranges, patterns, k):
    """the rows the scan walks, by the contract: a segment's seed is its cheapest window of 8 letters, the leftmost on a tie, expanded
    into its grams; every position t of a record — one at least as long as the shortest pattern — with t + 8 <= the record's length
    whose 8 bytes all have a base walks the rows of that gram"""
    chain = np.zeros(65536, dtype=np.int64)
    for p in patterns:
        step = len(p) // (k + 1)
        for j in range(k + 1):
            w = min(range(step - 7), key=lambda w: (expansion(p[j * step + w:j * step + w + 8]), w))
            for g in window_grams(p[j * step + w:j * step + w + 8]):
                chain[g] += 1
    has = BASE[np.frombuffer(bytes(buf), dtype=np.uint8)]
    code = np.select([has == 1, has == 2, has == 4, has == 8], [0, 1, 2, 3], 0).astype(np.int64)
    shortest = min(len(p) for p in patterns)
    total = 0
    for off, ln in ranges:
        off, ln = int(off), int(ln)
        if ln < max(shortest, 8):
            continue
        n = ln - 7
        gram = np.zeros(n, dtype=np.int64)
        ok = np.ones(n, dtype=bool)
        for i in range(8):
            gram |= code[off + i:off + i + n] << (2 * i)
            ok &= has[off + i:off + i + n] != 0
        total += int(chain[gram[ok]].sum())
    return total


def reverse_complement(seq):
    """the IUPAC reverse complement of upper-case letters of the table (U is read as T)"""
    return "".join(COMPLEMENT[c] for c in reversed(bytes(seq).decode().upper())).encode()


def widen(rng, seq, at, keep=True):
    """seq (bases) with the letters at the positions `at` replaced: keep — by degenerate codes that contain the base there; not keep —
    by letters of the table whose set excludes it"""
    out = bytearray(seq)
    for j in at:
        base = chr(out[j]).upper().replace("U", "T")
        codes = [c for c, s in SETS.items() if c != "U" and (len(s) > 1 and base in s if keep else base not in s)]
        out[j] = ord(codes[int(rng.integers(0, len(codes)))])
    return bytes(out)


def strands_of(bases, forward_only=False):
    bases = bytes(bases).upper().replace(b"U", b"T")
    out = [(0, "+", bases)]
    if not forward_only and reverse_complement(bases) != bases:
        out.append((1, "-", reverse_complement(bases)))
    return out


def cli_lines(files, queries, k=0, forward_only=False):
    """files: [(name, [(header line, sequence bytes)])] in collection order; queries: [(name, letters)] -> the TSV lines of `mbgc-hip f
    --iupac`: query, file, record, start, end, strand, mismatches; by file, record, start, query, + before -"""
    rows = []
    for f, (name, records) in enumerate(files):
        for r, (header, seq) in enumerate(records):
            for q, (qname, bases) in enumerate(queries):
                for order, strand, pat in strands_of(bases, forward_only):
                    for pos, d in hits_of_record(seq, pat, k):
                        rows.append((f, r, pos + 1, q, order, "\t".join([qname, name, header.split()[0], str(pos + 1), str(pos + len(pat)), strand, str(d)])))
    return [row[-1] for row in sorted(rows)]


def amplicon_lines(files, pairs, k=0, lo=0, hi=5000):
    """pairs: [(name, fwd, rev)], both 5'->3' -> (the product lines of `mbgc-hip f --primers`, the summary line). A + product: FWD + at
    [s1, e1], REV - at [s2, e2], s1 <= s2, e1 <= e2, lo <= e2 - s1 + 1 <= hi; a - product: REV + on the left, FWD - on the right. Lines:
    pair, file, record, start, end, strand, length, left mismatches, right mismatches; by file, record, start, end, pair, + before -"""
    rows, bases_searched = [], 0
    for f, (name, records) in enumerate(files):
        for r, (header, seq) in enumerate(records):
            bases_searched += len(seq)
            for p, (pname, fwd, rev) in enumerate(pairs):
                fwd, rev = bytes(fwd).upper(), bytes(rev).upper()
                for left, right, order, strand in ((fwd, reverse_complement(rev), 0, "+"), (rev, reverse_complement(fwd), 1, "-")):
                    rights = hits_of_record(seq, right, k)
                    for s1, d1 in hits_of_record(seq, left, k):
                        for s2, d2 in rights:
                            e1, e2 = s1 + len(left) - 1, s2 + len(right) - 1
                            if s1 <= s2 and e1 <= e2 and lo <= e2 - s1 + 1 <= hi:
                                rows.append((f, r, s1 + 1, e2 + 1, p, order, d1, d2,
                                             "\t".join([pname, name, header.split()[0], str(s1 + 1), str(e2 + 1), strand, str(e2 - s1 + 1), str(d1), str(d2)])))
    rows.sort()
    records = {(f, r) for f, r, *_ in rows}
    summary = "amplicons: %d of %d primer pairs in %d records of %d files; %d bases searched" % (len(rows), len(pairs), len(records), len({f for f, _ in records}), bases_searched)
    return [row[-1] for row in rows], summary
