"""The referee of mbgc_fasta_sketch_dev, mbgc_fasta_sketch_pairs_dev and `mbgc-hip k`, written from the contract alone, in numpy: no
project code, no tile, no packed word. hashes(text, k): k vectorised shifts over a uint64 code array build fw and rc of every
position at once, a validity mask drops the k-mers with a byte that is no A/C/G/T/U, np.minimum picks the canonical word and fmix64
is five array operations. The record is all the function is given, so a byte outside it cannot touch a hash. cli_lines: the lines of
the command out of the FASTA files' records."""
import math

import numpy as np

SEED = np.uint64(0x9E3779B97F4A7C15)
CODE = np.full(256, 4, dtype=np.uint8)
for _letters, _code in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _letters:
        CODE[ord(_ch)] = _code


def max_hash(scale):
    return (2 ** 64 - 1) // int(scale)


def fmix64(x):
    x = x.astype(np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def words(text, k):
    """bytes -> (fw, rc, valid) per position 0 .. len - k"""
    c = CODE[np.frombuffer(bytes(text), dtype=np.uint8)]
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, bool)
    fw, rc, valid = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.ones(n, bool)
    for j in range(k):
        cj = c[j:j + n]
        valid &= cj < 4
        v = (cj & 3).astype(np.uint64)
        fw |= v << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - v) << np.uint64(2 * j)
    return fw, rc, valid


def hashes(text, k):
    """bytes -> the hashes of its valid k-mers, one per valid position, in position order"""
    fw, rc, valid = words(text, k)
    return fmix64(np.minimum(fw, rc)[valid] ^ SEED)


def sketch(records, groups, k, max_hash, ngroups=None):
    """records: bytes each; groups: a group id each -> ([the strictly ascending distinct kept hashes per group], [kmers per group])"""
    ngroups = (max(groups) + 1 if len(groups) else 0) if ngroups is None else ngroups
    kept, kmers = [[] for _ in range(ngroups)], [0] * ngroups
    for text, g in zip(records, groups):
        h = hashes(text, k)
        kmers[g] += int(h.size)
        kept[g].append(h[h <= np.uint64(max_hash)])
    return [np.unique(np.concatenate(x)) if x else np.zeros(0, np.uint64) for x in kept], kmers


def shared(a, b):
    return int(np.intersect1d(a, b).size)


def reverse_complement(seq):
    return bytes(seq).translate(bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa"))[::-1]


def derived(s, a, b, k):
    """-> (jaccard, containment A, containment B, distance) as the host derives them in double"""
    j = s / (a + b - s) if a + b - s else 0.0
    d = 1.0 if j == 0 else max(0.0, -math.log(2 * j / (1 + j)) / k)
    return j, (s / a if a else 0.0), (s / b if b else 0.0), d + 0.0


def cli_lines(files, k=21, scale=1000, by_record=False, min_shared=0, no_pairs=False):
    """files: [(name, [(header line, sequence bytes)])] in collection order -> a dict of the lines of `mbgc-hip k`: "groups" (stdout, one
    per group), "pairs" (stdout or --pairs-out), "sketches" (--sketches-out), "order" (--order-out; file groups with pairs only),
    "summary" (one line); and, for the tests' own assertions, "sizes", "kmers" and "shared" {(i, j): n}"""
    names, records, groups, n_rec, bases = [], [], [], [], []
    for name, recs in files:
        if not by_record:
            names.append(name); n_rec.append(0); bases.append(0)
        for header, seq in recs:
            if by_record:
                names.append(header.split()[0]); n_rec.append(0); bases.append(0)
            records.append(seq)
            groups.append(len(names) - 1)
            n_rec[-1] += 1
            bases[-1] += len(seq)
    lists, kmers = sketch(records, groups, k, max_hash(scale), len(names))
    out = {"groups": [], "pairs": [], "sketches": [], "order": [], "sizes": [int(x.size) for x in lists], "kmers": kmers, "shared": {}}
    for g, name in enumerate(names):
        out["groups"].append("%s\t%d\t%d\t%d\t%d\t%d" % (name, n_rec[g], bases[g], kmers[g], lists[g].size, lists[g].size * scale))
        out["sketches"].append("%s\t%d\t%d\t%d\t%s" % (name, k, scale, lists[g].size, ",".join("%016x" % int(h) for h in lists[g])))
    total = [0] * len(names)
    if not no_pairs:
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                s = out["shared"][(i, j)] = shared(lists[i], lists[j])
                total[i] += s
                total[j] += s
                if s >= min_shared:
                    out["pairs"].append("%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f" % ((names[i], names[j], lists[i].size, lists[j].size, s) + derived(s, lists[i].size, lists[j].size, k)))
        if names and not by_record:
            first = max(range(len(names)), key=lambda g: (total[g], -g))
            with_first = lambda g: out["shared"][(min(g, first), max(g, first))]
            out["order"] = [names[first]] + [names[g] for g in sorted((g for g in range(len(names)) if g != first), key=lambda g: (-with_first(g), g))]
    out["summary"] = "sketch: %d groups, %d records, %d bases; k %d, scale %d; %d hashes of %d k-mers, %d pairs, %d share a hash" % (
        len(names), len(records), sum(bases), k, scale, sum(out["sizes"]), sum(kmers), len(out["shared"]), sum(1 for s in out["shared"].values() if s > 0))
    return out
