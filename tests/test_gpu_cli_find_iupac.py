"""`mbgc-hip f --iupac` and `f --primers` on a stream set, on the device. The three Listeria genomes of tests/golden/listeria are unpacked
and compressed with `mbgc-hip c`, as tests/test_gpu_cli_find.py does; the lines are held one by one against tests/_find_iupac.py's
brute force over the records of the unpacked FASTA files. The queries are cut from the genomes here: some letters widened to codes
that contain the original base (still a match), others replaced by codes that exclude it (a mismatch), one query that is its own
IUPAC reverse complement; the primers are cut 300 and 1800 bases apart, one pair on each strand. For every class the referee's own
lines are held non-empty before the comparison."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _find_iupac as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")


def tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def tsv(stdout, tabs=6):
    return [l for l in stdout.split("\n") if l.count("\t") == tabs]


def records_of(text):
    out = []
    for block in text.split(b">")[1:]:
        header, _, body = block.partition(b"\n")
        out.append((header.decode(), body.replace(b"\n", b"")))
    return out


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the unpacked files, the stream set, the queries, the primers and — computed once — the referee's lines"""
    tmp = str(tmp_path_factory.mktemp("find_iupac"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    files = []
    for f in names:
        data = lzma.open(os.path.join(LIST, f + ".xz")).read()
        open(os.path.join(tmp, f), "wb").write(data)
        files.append((f, records_of(data)))
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")
    r = tool(["c", "list.txt", "set"], tmp)
    assert r.returncode == 0, r.stderr
    longest = [max(range(len(recs)), key=lambda r: len(recs[r][1])) for _, recs in files]
    rng = np.random.default_rng(2)

    def cut(f, at, n):
        q = files[f][1][longest[f]][1][at:at + n].upper()
        assert len(q) == n and set(q) <= set(b"ACGT")
        return q

    L = type("Listeria", (), {})()
    L.tmp, L.files = tmp, files
    wide = ref.widen(rng, cut(0, 100_000, 30), [2, 9, 10, 17, 29])                       # still a match
    wide_rc = ref.reverse_complement(ref.widen(rng, cut(1, 200_000, 30), [0, 5, 14, 22]))       # found on the - strand
    two = ref.widen(rng, ref.widen(rng, cut(0, 300_000, 30), [1, 8, 25]), [4, 21], keep=False)   # two letters that exclude the base
    lower = ref.widen(rng, cut(2, 5_000, 24), [3, 12]).lower().replace(b"t", b"u")
    absent = ref.widen(rng, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30)].tobytes(), [7], keep=True)
    big = files[0][1][longest[0]][1].upper()
    own_at = next(p for p in range(len(big) - 10) if big[p:p + 10] == ref.reverse_complement(big[p:p + 10]))
    own = bytearray(big[own_at:own_at + 10])
    own[2], own[7] = ord("N"), ord("N")                                                 # N is its own complement: still its own reverse complement
    assert bytes(own) == ref.reverse_complement(bytes(own))
    L.queries = [("wide", wide), ("wide_rc", wide_rc), ("two", two), ("lower", lower), ("absent", absent), ("own", bytes(own))]
    open(os.path.join(tmp, "q.fa"), "w").write("".join(">%s words\n%s\n%s\n" % (n, q[:13].decode(), q[13:].decode()) for n, q in L.queries))
    L.want = {(k, fo): ref.cli_lines(files, L.queries if k == 0 else L.queries[:5], k, forward_only=fo) for k in (0, 2) for fo in (False, True)}
    by = lambda lines, n: [l.split("\t") for l in lines if l.startswith(n + "\t")]
    w0, w2 = L.want[0, False], L.want[2, False]
    assert any(l[5] == "+" and l[6] == "0" for l in by(w0, "wide")) and any(l[5] == "-" for l in by(w0, "wide_rc")) and by(w0, "lower") and not by(w0, "two")
    assert not by(w0, "absent") and by(w0, "own") and all(l[5] == "+" for l in by(w0, "own"))
    assert any(l[6] == "2" for l in by(w2, "two")) and len(L.want[0, True]) < len(w0)
    # the primers: pair `near` on the + strand, 300 bases from the first base of FWD to the last of REV's site, pair `far` on the - strand,
    # 1800 bases; 24-mers, so that K = 2 is allowed; widened
    g = files[1][1][longest[1]][1].upper()
    assert len(g) > 40_000
    at = next(p for p in range(len(g) // 3, len(g) // 2) if set(g[p:p + 2000]) <= set(b"ACGT"))
    near = ("near", ref.widen(rng, g[at:at + 24], [3, 11, 19]), ref.widen(rng, ref.reverse_complement(g[at + 300 - 24:at + 300]), [5, 16]))
    at2 = at + 5_000
    assert set(g[at2:at2 + 2000]) <= set(b"ACGT")
    far = ("far", ref.widen(rng, ref.reverse_complement(g[at2 + 1800 - 24:at2 + 1800]), [2, 20]), ref.widen(rng, g[at2:at2 + 24], [7, 13]))
    L.pairs, L.genome, L.near_at, L.far_at = [near, far], g, at, at2
    L.record = files[1][1][longest[1]][0].split()[0]
    return L


def run_f(L, args):
    return tool(["f"] + args + ["set"], L.tmp)


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("forward_only", [False, True])
def test_the_lines_equal_the_referee(listeria, k, forward_only):
    qfile = "q.fa"
    if k:                                                            # (the own-reverse-complement query has 10 letters: K = 0 only)
        qfile = "q2.fa"
        open(os.path.join(listeria.tmp, qfile), "w").write("".join(">%s\n%s\n" % (n, q.decode()) for n, q in listeria.queries[:5]))
    r = run_f(listeria, ["--iupac", "--seq-file", qfile, "--mismatches", str(k)] + (["--forward-only"] if forward_only else []))
    want = listeria.want[k, forward_only]
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == want
    nq = 6 if k == 0 else 5
    records = {tuple(l.split("\t")[1:3]) for l in want}
    bases = sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert "hits: %d in %d records of %d files; %d bases searched, %d patterns\n" % (len(want), len(records), len({f for f, _ in records}), bases,
                                                                                      nq if forward_only else 2 * nq - (k == 0)) in r.stdout


def test_without_iupac_a_degenerate_query_is_compared_literally(listeria):
    """the behaviour of before: an R matches only an R"""
    r = run_f(listeria, ["--seq", listeria.queries[0][1].decode()])
    assert r.returncode == 3 and tsv(r.stdout) == [], r.stderr


def test_the_hosts_loop_and_a_hit_buffer_of_one_row(listeria):
    want = listeria.want[0, False]
    r = run_f(listeria, ["--iupac", "--seq-file", "q.fa", "--find-host", "--bench"])
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == want
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    assert line["find_host_ms"] > 0 and line["hits"] == len(want) and line["rows"] == ref.table_rows([p for q in listeria.queries for _, _, p in ref.strands_of(q[1])], 0)
    assert line["rows_walked"] >= len(want) and set(line) >= {"find_kernel_ms", "bases_searched", "patterns", "hits", "retries", "decode_ms", "find_gb_per_s"}
    r = run_f(listeria, ["--iupac", "--seq-file", "q.fa", "--hit-capacity", "1", "--bench", "--hits", "hits.tsv", "--regions-out", "regions.txt"])
    assert r.returncode == 0 and tsv(r.stdout) == [], r.stderr
    assert open(os.path.join(listeria.tmp, "hits.tsv")).read().split("\n")[:-1] == want
    assert json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])["retries"] == 1
    assert open(os.path.join(listeria.tmp, "regions.txt")).read().split("\n")[:-1] == list(dict.fromkeys("%s:%s-%s" % tuple(l.split("\t")[2:5]) for l in want))


def test_a_query_without_a_usable_window_is_refused_by_name(listeria):
    r = run_f(listeria, ["--iupac", "--seq", "ACGTACGTACGT", "--seq", "ACNNNNNTG"])
    assert r.returncode == 1 and tsv(r.stdout) == [] and "pattern 1, segment 0" in r.stderr, r.stderr


def primer_args(pairs):
    return [a for n, f, v in pairs for a in ("--primers", "%s:%s:%s" % (n, f.decode(), v.decode()))]


def test_two_primer_pairs_one_on_each_strand(listeria):
    want, summary = ref.amplicon_lines(listeria.files, listeria.pairs, 0)
    rows = [l.split("\t") for l in want]
    assert ["near", listeria.record, str(listeria.near_at + 1), str(listeria.near_at + 300), "+", "300", "0", "0"] in [l[:1] + l[2:] for l in rows]
    assert ["far", listeria.record, str(listeria.far_at + 1), str(listeria.far_at + 1800), "-", "1800", "0", "0"] in [l[:1] + l[2:] for l in rows]
    r = run_f(listeria, primer_args(listeria.pairs) + ["--hits", "primer_hits.tsv"])
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout, 8) == want and tsv(r.stdout) == [] and summary + "\n" in r.stdout and "hits: " not in r.stdout
    hits = ref.cli_lines(listeria.files, [(n + e, p) for n, f, v in listeria.pairs for e, p in ((".fwd", f), (".rev", v))], 0)
    assert open(os.path.join(listeria.tmp, "primer_hits.tsv")).read().split("\n")[:-1] == hits and len(hits) >= 4
    # the same from a primer file, with two mismatches allowed: the referee again
    open(os.path.join(listeria.tmp, "primers.tsv"), "w").write("".join("%s\t%s\t%s\n" % (n, f.decode(), v.decode()) for n, f, v in listeria.pairs))
    want2, summary2 = ref.amplicon_lines(listeria.files, listeria.pairs, 2)
    r = run_f(listeria, ["--primer-file", "primers.tsv", "--mismatches", "2"])
    assert r.returncode == 0 and tsv(r.stdout, 8) == want2 and summary2 + "\n" in r.stdout and len(want2) >= len(want), r.stderr


def test_max_amplicon_drops_the_longer_product(listeria):
    want, summary = ref.amplicon_lines(listeria.files, listeria.pairs, 0, hi=1000)
    assert want and all(l.split("\t")[0] == "near" for l in want) and len(want) < len(ref.amplicon_lines(listeria.files, listeria.pairs, 0)[0])
    r = run_f(listeria, primer_args(listeria.pairs) + ["--max-amplicon", "1000"])
    assert r.returncode == 0 and tsv(r.stdout, 8) == want and summary + "\n" in r.stdout, r.stderr
    none, _ = ref.amplicon_lines(listeria.files, listeria.pairs, 0, lo=301, hi=1799)
    assert none == []
    r = run_f(listeria, primer_args(listeria.pairs) + ["--min-amplicon", "301", "--max-amplicon", "1799"])
    assert r.returncode == 3 and tsv(r.stdout, 8) == [] and "amplicons: 0 of 2 primer pairs in 0 records of 0 files" in r.stdout, r.stderr


def test_amplicons_out_feeds_d_region_list(listeria):
    want, _ = ref.amplicon_lines(listeria.files, listeria.pairs, 0)
    r = run_f(listeria, primer_args(listeria.pairs) + ["--amplicons-out", "amplicons.txt"])
    assert r.returncode == 0, r.stderr
    regions = open(os.path.join(listeria.tmp, "amplicons.txt")).read().split("\n")[:-1]
    assert regions == list(dict.fromkeys("%s:%s-%s" % tuple(l.split("\t")[2:5]) for l in want)) and len(regions) >= 2
    r = tool(["d", "--region-list", "amplicons.txt", "--fasta", "back", "set", "pieces"], listeria.tmp)
    assert r.returncode == 0, r.stderr
    got = [s.upper() for d, _, fs in os.walk(os.path.join(listeria.tmp, "back")) for f in sorted(fs) for _, s in records_of(open(os.path.join(d, f), "rb").read())]
    by_record = {h.split()[0]: s for _, recs in listeria.files for h, s in recs}
    cut = []
    for line in regions:
        name, _, span = line.rpartition(":")
        a, b = span.split("-")
        cut.append(by_record[name][int(a) - 1:int(b)].upper())
    assert sorted(got) == sorted(cut) and listeria.genome[listeria.near_at:listeria.near_at + 300] in got


def test_a_pair_that_amplifies_nothing_exits_with_3(listeria):
    rng = np.random.default_rng(9)
    a, b = (np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 24)].tobytes() for _ in range(2))
    assert ref.amplicon_lines(listeria.files, [("none", a, b)], 0)[0] == []
    r = run_f(listeria, ["--primers", "none:%s:%s" % (a.decode(), b.decode())])
    assert r.returncode == 3 and tsv(r.stdout, 8) == [] and "amplicons: 0 of 1 primer pairs" in r.stdout, r.stderr
