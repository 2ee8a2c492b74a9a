"""`mbgc-hip m`: a stream set screened on the device for the k-mers of query sequences. The three Listeria genomes of
tests/golden/listeria are unpacked and packed into sets (default rounds, -t1, and -m 3 read back with --restore-rc). The queries: a
1 500-base slice of the first genome with every 25th base substituted (60 substitutions: `f --mismatches 3` finds nothing, `m` does), its
reverse complement (the same numbers), the 1 500 bases of the first genome that share the most 21-mers with both others, and a random
1 500-mer (no line; alone: exit status 3). Every line is held against tests/_screen.py's lines over the FASTA text: the integer columns
as text, the %.6f column within 1e-6 — one unit of its last printed digit."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _screen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
SETS = {"default": ([], []), "t1": (["-t1"], []), "m3": (["-m", "3"], ["--restore-rc"])}
KEYS = {"screen_kernel_ms", "sort_ms", "bases", "keys", "table_slots", "filter_passes", "hits", "hit_reruns", "decode_ms", "screen_gb_per_s"}
K = 21


def tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def tsv(stdout):
    return [l for l in stdout.split("\n") if l.count("\t") == 4]


def records_of(text):
    out = []
    for block in text.split(b">")[1:]:
        header, _, body = block.partition(b"\n")
        out.append((header.decode(), body.replace(b"\n", b"")))
    return out


def same_lines(got, want):
    """pair lines: the names and the integer columns as text, the %.6f column within one unit of its last printed digit"""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        g, w = g.split("\t"), w.split("\t")
        assert g[:4] == w[:4], (g, w)
        assert len(g[4].split(".")[1]) == 6 and abs(float(g[4]) - float(w[4])) <= 1e-6 + 1e-12, (g, w)


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the three files, their records, the four queries and — computed once — the referee's lines at the defaults"""
    tmp = str(tmp_path_factory.mktemp("screen"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    raw = [lzma.open(os.path.join(LIST, f + ".xz")).read() for f in names]
    files = [(n, records_of(data)) for n, data in zip(names, raw)]
    for name, data in zip(names, raw):
        open(os.path.join(tmp, name), "wb").write(data)
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")
    rng = np.random.default_rng(83)
    longest = max(files[0][1], key=lambda r: len(r[1]))[1].upper()
    # the slice: 1 500 letters of A, C, G, T; every 25th base substituted by another one
    at = next(p for p in range(200_000, len(longest), 1500) if set(longest[p:p + 1500]) <= set(b"ACGT"))
    original = longest[at:at + 1500]
    mutated = bytearray(original)
    for i in range(24, 1500, 25):
        mutated[i] = b"ACGT"[(b"ACGT".index(mutated[i]) + 1 + int(rng.integers(0, 3))) % 4]
    mutated = bytes(mutated)
    assert sum(a != b for a, b in zip(original, mutated)) == 60
    # the window of the first genome's longest record that shares the most 21-mers with both other genomes
    c0, pos0 = _screen.canons(longest, K)
    in_both = np.ones(c0.size, bool)
    for _, recs in files[1:]:
        in_both &= np.isin(c0, np.unique(np.concatenate([_screen.canons(s, K)[0] for _, s in recs])))
    flags = np.zeros(len(longest) + 1, np.int64)
    flags[pos0[in_both] + 1] = 1
    sums = np.cumsum(flags)
    window = sums[1500 - K + 1:] - sums[:-(1500 - K + 1)]
    common = longest[int(np.argmax(window)):int(np.argmax(window)) + 1500]
    noise = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1500)].tobytes()
    L = type("Listeria", (), {})()
    L.tmp, L.files, L.names, L.original, L.noise = tmp, files, names, original, noise
    L.queries = [("mutated", mutated), ("flipped", _screen.reverse_complement(mutated)), ("common", common), ("noise", noise)]
    open(os.path.join(tmp, "queries.fa"), "wb").write(b"".join(b">" + n.encode() + b" a query\n" + s[:700] + b"\n" + s[700:] + b"\n" for n, s in L.queries))
    L.want = _screen.cli_lines(files, L.queries, k=K, flank=30)
    shared = L.want["shared"]
    assert shared[("mutated", names[0])] >= 200 and all(shared[("common", n)] >= 1000 for n in names) and all(shared[("noise", n)] == 0 for n in names)
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


def read(listeria, f):
    return open(os.path.join(listeria.tmp, f)).read().split("\n")[:-1]


@pytest.mark.parametrize("mode", ["default", "t1", "m3"])
def test_every_line_equals_the_referees(listeria, sets, mode):
    r = tool(["m", "--seq-file", "queries.fa", "--loci-out", "loci.tsv", "--regions-out", "regions.txt", "--flank", "30"] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    want = listeria.want
    same_lines(tsv(r.stdout), want["pairs"])
    assert r.stdout.split("\n")[-2] == want["summary"] and len(r.stdout.split("\n")) == len(want["pairs"]) + 2      # nothing else is written
    assert read(listeria, "loci.tsv") == want["loci"] and read(listeria, "regions.txt") == want["regions"] and len(want["loci"]) >= 5
    # the reverse complement: the same numbers, line by line; the random 1 500-mer: no line
    got = [l.split("\t") for l in tsv(r.stdout)]
    assert [l[1:] for l in got if l[0] == "mutated"] == [l[1:] for l in got if l[0] == "flipped"] != []
    assert not any(l[0] == "noise" for l in got) and sum(1 for l in got if l[0] == "common") == 3


def test_f_finds_nothing_where_m_reports_the_allele(listeria, sets):
    name, mutated = listeria.queries[0]
    r = tool(["f", "--seq", mutated.decode(), "--mismatches", "3", sets("default")], listeria.tmp)
    assert r.returncode == 3 and r.stdout.startswith("hits: 0 in 0 records"), (r.stdout, r.stderr)
    r = tool(["m", "--seq", mutated.decode(), sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    want = _screen.cli_lines(listeria.files, [("q1", mutated)], k=K)
    same_lines(tsv(r.stdout), want["pairs"])
    first = tsv(r.stdout)[0].split("\t")
    assert first[:3] == ["q1", listeria.names[0], str(1500 - K + 1)] and int(first[3]) >= 200 and want["summary"] in r.stdout
    # alone, the random 1 500-mer reports nothing: exit status 3, the summary all the same
    r = tool(["m", "--seq", listeria.noise.decode(), sets("default")], listeria.tmp)
    assert r.returncode == 3 and tsv(r.stdout) == [], (r.stdout, r.stderr)
    assert r.stdout == _screen.cli_lines(listeria.files, [("q1", listeria.noise)], k=K)["summary"] + "\n" and "0 hits, 0 pairs reported" in r.stdout


def test_by_record_select_other_k_and_thresholds(listeria, sets):
    chosen = [listeria.files[1]]
    want = _screen.cli_lines(chosen, listeria.queries, k=16, by_record=True, min_shared=3, min_containment=0.01, max_gap=100, min_hits=5)
    r = tool(["m", "--seq-file", "queries.fa", "-k", "16", "--by-record", "--select", listeria.names[1], "--min-shared", "3", "--min-containment", "0.01", "--loci-out", "loci2.tsv",
              "--max-gap", "100", "--min-locus-hits", "5", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    same_lines(tsv(r.stdout), want["pairs"])
    assert want["summary"] in r.stdout and read(listeria, "loci2.tsv") == want["loci"] and len(want["pairs"]) >= 2 and "%d groups" % len(chosen[0][1]) in want["summary"]


def test_the_hosts_loops_agree_and_bench_prints_its_line(listeria, sets):
    r = tool(["m", "--seq-file", "queries.fa", "--screen-host", "--loci-out", "loci3.tsv", "--select", listeria.names[0], sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    r = tool(["m", "--seq-file", "queries.fa", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    same_lines(tsv(r.stdout), listeria.want["pairs"])
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    keys = int(_screen.key_set([s for _, s in listeria.queries], K)[0].size)
    assert set(line) == KEYS and line["keys"] == keys and line["hits"] == listeria.want["hits"] and line["bases"] == sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert line["table_slots"] >= 2 * keys and line["table_slots"] & (line["table_slots"] - 1) == 0 and line["filter_passes"] >= line["hits"] and line["screen_kernel_ms"] > 0


def test_regions_out_feeds_d_region_list(listeria, sets):
    """the mutated slice's locus in the genome it was cut from, widened by 30 bases, fetched by d: the piece holds the original slice"""
    name, mutated = listeria.queries[0]
    r = tool(["m", "--seq", mutated.decode(), "--regions-out", "r.txt", "--flank", "30", "--select", listeria.names[0], sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    want = _screen.cli_lines([listeria.files[0]], [("q1", mutated)], k=K, flank=30)
    regions = read(listeria, "r.txt")
    assert regions == want["regions"] and len(regions) >= 1
    r = tool(["d", "--region-list", "r.txt", sets("default"), "back"], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert listeria.original in open(os.path.join(listeria.tmp, "back.seq"), "rb").read().upper()
    # a --hit-capacity below the hits is a refusal that says how many there are
    r = tool(["m", "--seq", mutated.decode(), "--regions-out", "r2.txt", "--hit-capacity", "5", sets("default")], listeria.tmp)
    assert r.returncode == 1 and "--hit-capacity" in r.stderr and "%d hits" % _screen.cli_lines(listeria.files, [("q1", mutated)], k=K)["hits"] in r.stderr, r.stderr


def test_refusals_on_a_real_set(listeria, sets):
    s = sets("default")
    q = ["--seq", listeria.noise.decode()]
    for args, word in ((q + ["--region", "KK073979.1:1-10", s], "--region"), (q + ["--check", s], "--check"), (q + ["--fasta", "dir", s], "--fasta"), (q + ["-k", "33", s], "-k 33")):
        r = tool(["m"] + args, listeria.tmp)
        assert r.returncode == 1 and "mbgc-hip m: " in r.stderr and word in r.stderr and r.stderr.count("\n") == 1 and r.stdout == "", (args, r.stderr)
    r = tool(["m"] + q + [sets("m3")], listeria.tmp)                                               # (an -m 3 set read back without --restore-rc: d's refusal)
    assert r.returncode == 1 and "mbgc-hip m: " in r.stderr and "--restore-rc" in r.stderr and r.stdout == "", r.stderr
    r = tool(["m", "--seq", listeria.queries[0][1].decode(), "--loci-out", os.path.join(listeria.tmp, "no", "such", "dir", "l.tsv"), s], listeria.tmp)
    assert r.returncode == 1 and "cannot write" in r.stderr
