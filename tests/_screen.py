"""The referee of mbgc_fasta_screen_dev, mbgc_screen_loci.h and `mbgc-hip m`, written from the contract alone, in Python and numpy: no
project code, no tile, no packed word, no filter, no table. canons(text, k): k vectorised shifts over a uint64 code array build fw and
rc of every position at once, a validity mask drops the k-mers with a byte that is no A/C/G/T/U, np.minimum picks the canonical word —
that word, no hash, is a k-mer's key. A record is all a function is given, so a byte outside it cannot touch a result.
  key_set(queries, k)       -> (the strictly ascending union of the queries' distinct keys, [each query's own sorted distinct keys])
  screen(records, groups..) -> ([per group the ascending indices of the keys that occur in it], the hits (rec, pos, key index) by (rec, pos))
  loci(hits, ...)           -> the chains of one query's hit positions per record
  cli_lines(files, ...)     -> the lines of the command out of the FASTA files' records"""
import numpy as np

CODE = np.full(256, 4, dtype=np.uint8)
for _letters, _code in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _letters:
        CODE[ord(_ch)] = _code


def canons(text, k):
    """bytes -> (the canonical words of its valid k-mers in position order, their positions)"""
    c = CODE[np.frombuffer(bytes(text), dtype=np.uint8)]
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    fw, rc, valid = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.ones(n, bool)
    for j in range(k):
        cj = c[j:j + n]
        valid &= cj < 4
        v = (cj & 3).astype(np.uint64)
        fw |= v << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - v) << np.uint64(2 * j)
    return np.minimum(fw, rc)[valid], np.flatnonzero(valid)


def reverse_complement(seq):
    return bytes(seq).translate(bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa"))[::-1]


def key_set(queries, k):
    own = [np.unique(canons(q, k)[0]) for q in queries]
    return (np.unique(np.concatenate(own)) if own else np.zeros(0, np.uint64)), own


def screen(records, groups, ngroups, keys, k):
    """records: bytes each; groups: a group id each; keys: strictly ascending uint64"""
    keys = np.asarray(keys, dtype=np.uint64)
    found, hits = [[] for _ in range(ngroups)], []
    for r, (text, g) in enumerate(zip(records, groups)):
        c, pos = canons(text, k)
        at = np.searchsorted(keys, c)
        is_key = (at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == c) if keys.size else np.zeros(c.size, bool)
        found[g].append(at[is_key])
        hits += [(r, int(p), int(i)) for p, i in zip(pos[is_key], at[is_key])]
    return [np.unique(np.concatenate(x)).astype(np.uint32) if x else np.zeros(0, np.uint32) for x in found], hits


def loci(hits, keys, own, k, max_gap=500, min_hits=3):
    """hits: (rec, pos, key index) sorted by (rec, pos); own: each query's keys -> [(query, rec, start, end, hits, distinct)], 0-based
    inclusive, sorted by (query, rec, start). Cut where two neighbours are MORE than max_gap apart; a piece needs min_hits positions"""
    keys = np.asarray(keys, dtype=np.uint64)
    out = []
    for q, mine in enumerate(own):
        member = set(int(i) for i in np.searchsorted(keys, mine))
        by_rec = {}
        for rec, pos, key in hits:
            if key in member:
                by_rec.setdefault(rec, []).append((pos, key))
        for rec in sorted(by_rec):
            rows = sorted(set(by_rec[rec]))
            piece = [rows[0]]
            for row in rows[1:] + [None]:
                if row is not None and row[0] - piece[-1][0] <= max_gap:
                    piece.append(row)
                    continue
                if len(piece) >= min_hits:
                    out.append((q, rec, piece[0][0], piece[-1][0] + k - 1, len(piece), len(set(key for _, key in piece))))
                piece = [row]
    return out


def region_line(record, start, end, flank):
    """a locus [start, end] (0-based) as a line of --regions-out"""
    return "%s:%d-%d" % (record, max(1, start + 1 - flank), end + 1 + flank)


def cli_lines(files, queries, k=21, by_record=False, min_shared=1, min_containment=0.0, max_gap=500, min_hits=3, flank=0):
    """files: [(name, [(header line, sequence bytes)])] in collection order; queries: [(name, bases)] -> a dict of the lines of `mbgc-hip
    m`: "pairs" (stdout), "loci" (--loci-out), "regions" (--regions-out), "summary"; and, for the tests' own assertions, "shared" {(query
    name, group name): n}, "keys" (per query), "hits" and "loci_rows" (query, file, record, start, end, hits, distinct; 1-based)"""
    names, records, groups, where = [], [], [], []
    for name, recs in files:
        if not by_record:
            names.append(name)
        for header, seq in recs:
            if by_record:
                names.append(header.split()[0])
            records.append(seq)
            groups.append(len(names) - 1)
            where.append((name, header.split()[0]))
    keys, own = key_set([s for _, s in queries], k)
    found, hits = screen(records, groups, len(names), keys, k)
    out = {"pairs": [], "loci": [], "regions": [], "shared": {}, "keys": [int(o.size) for o in own], "hits": len(hits), "loci_rows": []}
    for (qname, _), mine in zip(queries, own):
        idx = np.searchsorted(keys, mine)
        for g, gname in enumerate(names):
            s = int(np.intersect1d(idx, found[g]).size)
            out["shared"][(qname, gname)] = s
            c = s / mine.size if mine.size else 0.0
            if s >= min_shared and c >= min_containment:
                out["pairs"].append("%s\t%s\t%d\t%d\t%.6f" % (qname, gname, mine.size, s, c))
    for q, rec, start, end, n, distinct in loci(hits, keys, own, k, max_gap, min_hits):
        row = (queries[q][0], where[rec][0], where[rec][1], start + 1, end + 1, n, distinct)
        out["loci_rows"].append(row)
        out["loci"].append("%s\t%s\t%s\t%d\t%d\t%d\t%d" % row)
        line = region_line(where[rec][1], start, end, flank)
        if line not in out["regions"]:
            out["regions"].append(line)
    out["summary"] = "screen: %d queries, %d distinct k-mers, k %d; %d groups, %d records, %d bases; %d hits, %d pairs reported" % (
        len(queries), keys.size, k, len(names), len(records), sum(len(s) for s in records), len(hits), len(out["pairs"]))
    return out
