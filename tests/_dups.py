"""The referee of `mbgc-hip u` and mbgc_fasta_dups_dev, written from the definition in include/mbgc_fasta.h and from nothing else: fold, the
comp table, the canonical key min(fold(s), revcomp(fold(s))) as bytes, rep = the first index with that key, the strand by comparing with
rep itself; and the command's lines over FASTA records. Plain Python over bytes: no fingerprint, no GPU."""

PAIRS = (b"AT", b"CG", b"RY", b"KM", b"BV", b"DH")


def comp_table():
    """comp over 0..255: the six pairs on upper case, the same on lower case (keeping the case), every other byte itself"""
    t = list(range(256))
    for a, b in PAIRS:
        for x, y in ((a, b), (b, a)):
            t[x] = y
            t[x | 0x20] = y | 0x20
    return bytes(t)


COMP = comp_table()
FOLD = bytes(b & 0xDF if ord("a") <= b <= ord("z") else b for b in range(256))
assert all(COMP[COMP[b]] == b for b in range(256))                   # an involution


def fold(s, exact_case=False):
    return bytes(s) if exact_case else bytes(s).translate(FOLD)


def revcomp(s):
    return bytes(s)[::-1].translate(COMP)


def classes(records, forward_only=False, exact_case=False):
    """records: bytes objects -> ([(rep, strand)] per record, the number of classes)"""
    folded = [fold(s, exact_case) for s in records]
    first, out = {}, []
    for r, f in enumerate(folded):
        key = f if forward_only else min(f, revcomp(f))
        rep = first.setdefault(key, r)
        if f == folded[rep]:
            out.append((rep, 0))
        else:
            assert not forward_only and f == revcomp(folded[rep])
            out.append((rep, 1))
    return out, len(first)


def cli_lines(files, forward_only=False, exact_case=False, min_len=1):
    """files: [(name, [(header, sequence)])] in collection order -> dict(dups: stdout's lines, clusters: --clusters-out, unique:
    --unique-files-out, summary: the summary line)"""
    recs = [(h.split()[0] if h.split() else "", name, s) for name, rs in files for h, s in rs]
    cls, n = classes([s for _, _, s in recs], forward_only, exact_case)
    least = max(min_len, 1)

    def columns(r):
        rep, strand = cls[r]
        return "\t".join([recs[r][0], recs[r][1], str(len(recs[r][2])), "-" if strand else "+", recs[rep][0], recs[rep][1]])
    kept = [r for r in range(len(recs)) if len(recs[r][2]) >= least]
    dups = [r for r in kept if cls[r][0] != r]
    members = {}
    for r in kept:
        members.setdefault(cls[r][0], []).append(r)
    clusters, number = [], 0
    for rep in sorted(members):
        if len(members[rep]) > 1:
            number += 1
            clusters += [columns(r) + "\t%d" % number for r in members[rep]]
    seen, unique, at = set(), [], 0
    for name, rs in files:
        key = tuple(sorted(cls[r][0] for r in range(at, at + len(rs))))
        at += len(rs)
        if key not in seen:
            seen.add(key)
            unique.append(name)
    summary = "dups: %d records, %d bases; %d distinct sequences; %d duplicate records, %d bases (%d as reverse complements); %d of %d files duplicate" % (
        len(recs), sum(len(s) for _, _, s in recs), n, len(dups), sum(len(recs[r][2]) for r in dups), sum(cls[r][1] for r in dups), len(files) - len(unique), len(files))
    return {"dups": [columns(r) for r in dups], "clusters": clusters, "unique": unique, "summary": summary, "classes": cls}
