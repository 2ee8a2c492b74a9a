"""`mbgc-hip s`: composition, N50 and the runs of N / lower case of a stream set, taken on the device. The three Listeria genomes of
tests/golden/listeria are unpacked and, before `mbgc-hip c`, letters of their sequence lines are rewritten (the line structure stays):
in genome 0 two stretches of the longest record become N — 100 bytes, and 5 000 bytes that end on the record's last base —, in genome 1
three stretches become lower case, one of them from the record's first base on; genome 2 is left alone. The sets (default rounds, -t1,
and -m 3 read back with --restore-rc) are described and every line is held against tests/_stats.py's lines over the rewritten FASTA
text; the referee's own gap and mask tables are held non-empty, and of the planted sizes, before they are compared."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
SETS = {"default": ([], []), "t1": (["-t1"], []), "m3": (["-m", "3"], ["--restore-rc"]), "upper": (["-U"], [])}
KEYS = {"stats_kernel_ms", "bases", "records", "edges", "edge_reruns", "decode_ms", "stats_gb_per_s"}


def tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def lines_of(stdout, tabs):
    return [l for l in stdout.split("\n") if l.count("\t") == tabs]


def records_of(text):
    out = []
    for block in text.split(b">")[1:]:
        header, _, body = block.partition(b"\n")
        out.append((header.decode(), body.replace(b"\n", b"")))
    return out


def rewrite(data, edits):
    """data: a FASTA file's bytes; edits: [(from, to, function of bytes)] over the bases of its longest record -> the file with those
    bases rewritten, every line as long as it was"""
    a = np.frombuffer(data, dtype=np.uint8).copy()
    starts = np.flatnonzero(a == ord(">"))
    spans = []
    for s, e in zip(starts, list(starts[1:]) + [a.size]):
        body = s + int(np.flatnonzero(a[s:e] == 10)[0]) + 1
        where = body + np.flatnonzero(a[body:e] != 10)
        spans.append(where)
    where = max(spans, key=len)
    for lo, hi, f in edits:
        lo, hi = (lo + where.size if lo < 0 else lo), (hi + where.size if hi <= 0 else hi)
        a[where[lo:hi]] = np.frombuffer(f(a[where[lo:hi]].tobytes()), dtype=np.uint8)
    return a.tobytes()


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the rewritten files, their records and — computed once — the referee's lines"""
    tmp = str(tmp_path_factory.mktemp("stats"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    to_n, to_lower = (lambda b: b"N" * len(b)), (lambda b: b.lower())
    edits = [[(70_000, 70_100, to_n), (-5_000, 0, to_n)], [(0, 777, to_lower), (123_456, 125_000, to_lower), (300_001, 300_002, to_lower)], []]
    files = []
    for f, e in zip(names, edits):
        data = rewrite(lzma.open(os.path.join(LIST, f + ".xz")).read(), e)
        open(os.path.join(tmp, f), "wb").write(data)
        files.append((f, records_of(data)))
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")
    L = type("Listeria", (), {})()
    L.tmp, L.files, L.names = tmp, files, names
    L.want = _stats.cli_lines(files)
    L.want_11, L.want_101 = _stats.cli_lines(files, min_gap=11), _stats.cli_lines(files, min_gap=101)
    # the planted stretches stand in the referee's tables: the two gaps with their sizes, the second one ending its record, and the three masks
    longest = [max(recs, key=lambda r: len(r[1])) for _, recs in files]
    word0, word1 = longest[0][0].split()[0], longest[1][0].split()[0]
    n0 = len(longest[0][1])
    assert "%s\t70000\t70100" % word0 in L.want["gaps"] and "%s\t%d\t%d" % (word0, n0 - 5000, n0) in L.want["gaps"]
    # (the genomes hold gaps of their own, two of them of 10 bytes: between --min-gap 11 and --min-gap 101 lies the planted gap alone)
    assert set(L.want["gaps"]) > set(L.want_11["gaps"]) > set(L.want_101["gaps"]) and set(L.want_11["gaps"]) - set(L.want_101["gaps"]) == {"%s\t70000\t70100" % word0}
    assert "%s\t%d\t%d" % (word0, n0 - 5000, n0) in L.want_101["gaps"]
    assert {"%s\t0\t777" % word1, "%s\t123456\t125000" % word1, "%s\t300001\t300002" % word1} <= set(L.want["masked"])
    assert len(L.want["files"]) == 3 and len(L.want["records"]) == sum(len(r) for _, r in files) > 3
    return L


@pytest.fixture(scope="module")
def sets(listeria):
    """the stream sets, made when first asked for: c runs where the files lie (the list holds bare names), each set under its mode's name"""
    made = {}

    def get(mode):
        if mode not in made:
            r = tool(["c"] + SETS[mode][0] + ["list.txt", mode], listeria.tmp)
            assert r.returncode == 0, r.stderr
            made[mode] = mode
        return made[mode]
    return get


@pytest.mark.parametrize("mode", ["default", "t1", "m3"])
def test_every_line_equals_the_referees(listeria, sets, mode):
    r = tool(["s", "--records", "rec.tsv", "--gaps-out", "gaps.bed", "--min-gap", "1", "--masked-out", "masked.bed"] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 14) == listeria.want["files"]
    assert listeria.want["summary"] in r.stdout.split("\n")
    read = lambda f: open(os.path.join(listeria.tmp, f)).read().split("\n")[:-1]
    assert read("rec.tsv") == listeria.want["records"]
    assert read("gaps.bed") == listeria.want["gaps"] and read("masked.bed") == listeria.want["masked"]


def test_min_gap_drops_exactly_the_short_gap_and_records_go_to_stdout(listeria, sets):
    r = tool(["s", "--gaps-out", "gaps11.bed", "--min-gap", "11", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(listeria.tmp, "gaps11.bed")).read().split("\n")[:-1] == listeria.want_11["gaps"]
    r = tool(["s", "--gaps-out", "gaps101.bed", "--min-gap", "101", "--records", "-", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(listeria.tmp, "gaps101.bed")).read().split("\n")[:-1] == listeria.want_101["gaps"]
    out = r.stdout.split("\n")
    first = out.index(listeria.want["records"][0])
    assert out[first:first + len(listeria.want["records"])] == listeria.want["records"]            # the records' lines, then the files'
    assert lines_of("\n".join(out[first + len(listeria.want["records"]):]), 14) == listeria.want["files"]
    assert listeria.want["summary"] in out                                                          # (the summary counts every run of N, whatever --min-gap is)


def test_select_describes_the_chosen_file_only(listeria, sets):
    """the second file's contigs depend on the first file's: those are decoded, and not counted"""
    want = _stats.cli_lines(listeria.files[1:2])
    r = tool(["s", "--select", listeria.names[1], "--masked-out", "m1.bed", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 14) == want["files"] == listeria.want["files"][1:2] and want["summary"] in r.stdout.split("\n")
    assert open(os.path.join(listeria.tmp, "m1.bed")).read().split("\n")[:-1] == want["masked"] != []


def test_select_seq_of_one_header_is_one_record(listeria, sets):
    name, records = listeria.files[0]
    header, seq = max(records, key=lambda r: len(r[1]))
    want = _stats.cli_lines([(name, [(header, seq)])])
    r = tool(["s", "--select-seq", header.split()[0], "--records", "one.tsv", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    line = lines_of(r.stdout, 14)
    assert line == want["files"] and line[0].split("\t")[1:7] == ["1", str(len(seq)), str(len(seq)), str(len(seq)), str(len(seq)), "1"]
    assert open(os.path.join(listeria.tmp, "one.tsv")).read().split("\n")[:-1] == want["records"] and want["summary"] in r.stdout.split("\n")


def test_the_hosts_loop_agrees_and_bench_prints_its_line(listeria, sets):
    r = tool(["s", "--stats-host", "--masked-out", "mh.bed", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 14) == listeria.want["files"]
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    assert set(line) >= KEYS and line["records"] == len(listeria.want["records"]) and line["bases"] == sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert line["edges"] == 2 * (len(listeria.want["gaps"]) + len(listeria.want["masked"])) and line["stats_kernel_ms"] > 0


def test_refusals(listeria, sets):
    for args, word in ((["--region", "KK073979.1:1-10", sets("default")], "--region"), (["--check", sets("default")], "--check"),
                       (["--fasta", "dir", sets("default")], "--fasta")):
        r = tool(["s"] + args, listeria.tmp)
        assert r.returncode == 1 and "mbgc-hip s: " in r.stderr and word in r.stderr and r.stderr.count("\n") == 1 and lines_of(r.stdout, 14) == [], (args, r.stderr)
    r = tool(["s", sets("m3")], listeria.tmp)                                                     # (an -m 3 set read back without --restore-rc: d's refusal)
    assert r.returncode == 1 and "mbgc-hip s: " in r.stderr and "--restore-rc" in r.stderr and lines_of(r.stdout, 14) == [], r.stderr
    r = tool(["s", "--gaps-out", os.path.join(listeria.tmp, "no", "such", "dir", "g.bed"), sets("default")], listeria.tmp)
    assert r.returncode == 1 and "cannot write" in r.stderr


def test_an_upper_case_set_has_no_lower_case(listeria, sets):
    upper = [(name, [(h, s.upper()) for h, s in recs]) for name, recs in listeria.files]
    want = _stats.cli_lines(upper)
    assert want["masked"] == [] and want["gaps"] == listeria.want["gaps"]
    r = tool(["s", "--masked-out", "mu.bed", "--gaps-out", "gu.bed", sets("upper")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 14) == want["files"] and all(l.split("\t")[13] == "0" for l in lines_of(r.stdout, 14)) and want["summary"] in r.stdout.split("\n")
    assert open(os.path.join(listeria.tmp, "mu.bed")).read() == "" and open(os.path.join(listeria.tmp, "gu.bed")).read().split("\n")[:-1] == want["gaps"]
