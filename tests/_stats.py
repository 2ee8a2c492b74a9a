"""The referee of mbgc_fasta_stats_dev and `mbgc-hip s`, written from the contract alone, in numpy: no project code, no tile, no edge
buffer. counts(text): the eight counters of a record out of one np.bincount over its bytes. runs(text, cls): the maximal runs of a
class out of np.diff of the class mask padded with a 0 on both sides — the record is all the function is given, so a byte outside it
cannot touch a run. cli_lines: the lines of the command out of the FASTA files' records."""
import numpy as np

COLUMNS = ("a", "c", "g", "t", "n", "other", "lower", "reserved")


def counts(text):
    """bytes -> [a, c, g, t, n, other, lower, reserved]: a, c, g, t (with u) and n without case, other = every other byte, lower = the
    bytes in 'a'..'z' whatever the letter"""
    b = np.bincount(np.frombuffer(bytes(text), dtype=np.uint8), minlength=256)
    both = lambda ch: int(b[ord(ch)]) + int(b[ord(ch.lower())])
    a, c, g, t, n = both("A"), both("C"), both("G"), both("T") + both("U"), both("N")
    return [a, c, g, t, n, int(b.sum()) - a - c - g - t - n, int(b[ord("a"):ord("z") + 1].sum()), 0]


def class_mask(text, cls):
    x = np.frombuffer(bytes(text), dtype=np.uint8)
    return (x == ord("N")) | (x == ord("n")) if cls == 0 else (x >= ord("a")) & (x <= ord("z"))


def runs(text, cls, least=1):
    """bytes -> [(start, len)] of the maximal runs of class cls (0: N / n, 1: 'a'..'z') of at least `least` bytes (0 is read as 1)"""
    d = np.diff(np.concatenate([[0], class_mask(text, cls).astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return [(int(s), int(e - s)) for s, e in zip(starts, ends) if e - s >= max(int(least), 1)]


def table(buf, ranges, flags=7, min_n=1, min_lower=1):
    """buf: the buffer's bytes; ranges: (off, len) per record -> (counts as an (n, 8) uint64 array, [(rec, cls, start, len)] sorted)"""
    buf = bytes(buf)
    cnt = np.array([counts(buf[o:o + n]) for o, n in ranges], dtype=np.uint64).reshape(-1, 8)
    rows = []
    for r, (o, n) in enumerate(ranges):
        for cls, flag, least in ((0, 2, min_n), (1, 4, min_lower)):
            if flags & flag:
                rows += [(r, cls, s, ln) for s, ln in runs(buf[o:o + n], cls, least)]
    return cnt, sorted(rows)


def gc(c):
    acgt = c[0] + c[1] + c[2] + c[3]
    return "%.6f" % ((c[2] + c[1]) / acgt if acgt else 0.0)


def n50(lengths):
    """-> (N50, L50) over the lengths in descending order: L50 = the smallest count whose cumulative length x 2 >= the sum"""
    total, run = sum(lengths), 0
    for i, ln in enumerate(sorted(lengths, reverse=True)):
        run += ln
        if total and 2 * run >= total:
            return ln, i + 1
    return 0, 0


def cli_lines(files, min_gap=1, min_masked=1):
    """files: [(name, [(header line, sequence bytes)])] in collection order -> a dict of the lines of `mbgc-hip s`: "files" (stdout, one
    per file), "records" (--records), "gaps" / "masked" (--gaps-out / --masked-out: BED) and "summary" (one line)"""
    out = {"files": [], "records": [], "gaps": [], "masked": []}
    total, n_runs, n_records = [0] * 8, 0, 0
    for name, records in files:
        per, lens = [0] * 8, []
        for header, seq in records:
            c, word = counts(seq), header.split()[0]
            per = [x + y for x, y in zip(per, c)]
            lens.append(len(seq))
            out["records"].append("\t".join([name, word, str(len(seq))] + [str(v) for v in c[:7]] + [gc(c)]))
            n_runs += len(runs(seq, 0))
            out["gaps"] += ["%s\t%d\t%d" % (word, s, s + ln) for s, ln in runs(seq, 0, min_gap)]
            out["masked"] += ["%s\t%d\t%d" % (word, s, s + ln) for s, ln in runs(seq, 1, min_masked)]
        half, count = n50(lens)
        out["files"].append("\t".join([name, str(len(lens)), str(sum(lens)), str(min(lens, default=0)), str(max(lens, default=0)), str(half), str(count)] +
                                      [str(v) for v in per[:7]] + [gc(per)]))
        total = [x + y for x, y in zip(total, per)]
        n_records += len(lens)
    out["summary"] = "stats: %d files, %d records, %d bases; GC %s, N %d in %d runs, lower-case %d, other %d" % (
        len(files), n_records, sum(total[:6]), gc(total), total[4], n_runs, total[6], total[5])
    return out
