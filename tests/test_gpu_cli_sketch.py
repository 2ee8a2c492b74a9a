"""`mbgc-hip k`: k-mer sketches of a stream set's files (or records) and what every two of them share, taken on the device. The three
Listeria genomes of tests/golden/listeria are unpacked, and two more files are made: a copy of genome 2 under another name with every
record reverse-complemented (the same canonical k-mers: the same sketch), and genome 0 with 5 000 bases of its longest record turned
to N (fewer k-mers, a sketch that differs). The sets (default rounds, -t1, and -m 3 read back with --restore-rc) are sketched and
every line is held against tests/_sketch.py's lines over the FASTA text: the integer columns as text, the four %.6f columns within
1e-6 — one unit of the last printed digit, the two sides may round a libm log differently."""
import json
import lzma
import os
import subprocess

import pytest

import _sketch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
SETS = {"default": ([], []), "t1": (["-t1"], []), "m3": (["-m", "3"], ["--restore-rc"])}
KEYS = {"sketch_kernel_ms", "pairs_kernel_ms", "sort_ms", "bases", "rows", "row_reruns", "hashes", "pairs", "decode_ms", "sketch_gb_per_s"}


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


def fasta_of(records):
    return b"".join(b">" + h.encode() + b"\n" + b"".join(s[i:i + 70] + b"\n" for i in range(0, len(s), 70)) for h, s in records)


def same_pairs(got, want):
    """pair lines: the names and the integer columns as text, the four %.6f columns within one unit of the last printed digit"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        g, w = g.split("\t"), w.split("\t")
        assert g[:5] == w[:5], (g, w)
        for x, y in zip(g[5:], w[5:]):
            assert len(x.split(".")[1]) == 6 and not x.startswith("-") and abs(float(x) - float(y)) <= 1e-6 + 1e-12, (g, w)


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the five files, their records and — computed once — the referee's lines at the defaults"""
    tmp = str(tmp_path_factory.mktemp("sketch"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    raw = [lzma.open(os.path.join(LIST, f + ".xz")).read() for f in names]
    genomes = [records_of(data) for data in raw]
    flipped = [(h, _sketch.reverse_complement(s)) for h, s in genomes[2]]
    longest = max(range(len(genomes[0])), key=lambda r: len(genomes[0][r][1]))
    planted = list(genomes[0])
    h, s = planted[longest]
    planted[longest] = (h, s[:100_000] + b"N" * 5_000 + s[105_000:])
    files = list(zip(names, genomes)) + [("flipped.fa", flipped), ("planted.fa", planted)]
    for name, data in list(zip(names, raw)) + [(name, fasta_of(recs)) for name, recs in files[3:]]:
        open(os.path.join(tmp, name), "wb").write(data)
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(n for n, _ in files) + "\n")
    L = type("Listeria", (), {})()
    L.tmp, L.files, L.names = tmp, files, [n for n, _ in files]
    L.want = _sketch.cli_lines(files)
    assert len(L.want["groups"]) == 5 and len(L.want["pairs"]) == 10 and len(L.want["order"]) == 5 and min(L.want["sizes"]) > 1000
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
    r = tool(["k", "--pairs-out", "pairs.tsv", "--sketches-out", "sk.tsv", "--order-out", "order.txt"] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 5) == listeria.want["groups"] and lines_of(r.stdout, 8) == []
    assert listeria.want["summary"] in r.stdout.split("\n")
    same_pairs(read(listeria, "pairs.tsv"), listeria.want["pairs"])
    assert read(listeria, "sk.tsv") == listeria.want["sketches"] and read(listeria, "order.txt") == listeria.want["order"]


def test_the_two_made_files(listeria, sets):
    """the reverse-complemented copy has its original's sketch; the planted N cost k-mers and hashes"""
    want, k = listeria.want, 21
    r = tool(["k", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    same_pairs(lines_of(r.stdout, 8), want["pairs"])                 # (without --pairs-out the pair lines are on stdout)
    groups = [l.split("\t") for l in lines_of(r.stdout, 5)]
    pairs = {(l.split("\t")[0], l.split("\t")[1]): l.split("\t") for l in lines_of(r.stdout, 8)}
    line = pairs[(listeria.names[2], "flipped.fa")]
    assert line[2] == line[3] == line[4] == str(want["sizes"][2]) and line[5] == "1.000000" and line[8] == "0.000000"
    line = pairs[(listeria.names[0], "planted.fa")]
    assert int(line[4]) == want["shared"][(0, 4)] < want["sizes"][0] == int(line[2])
    lost = want["kmers"][0] - want["kmers"][4]
    assert 5_000 <= lost <= 5_000 + k - 1 and int(groups[0][3]) - int(groups[4][3]) == lost


@pytest.mark.parametrize("args", [["-k", "32", "--scale", "50"], ["-k", "21", "--scale", "1000"]])
def test_other_k_and_scale(listeria, sets, args):
    want = _sketch.cli_lines(listeria.files, k=int(args[1]), scale=int(args[3]))
    r = tool(["k"] + args + ["--sketches-out", "sk2.tsv", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 5) == want["groups"] and want["summary"] in r.stdout.split("\n")
    same_pairs(lines_of(r.stdout, 8), want["pairs"])
    assert read(listeria, "sk2.tsv") == want["sketches"]


def test_by_record_select_min_shared_and_no_pairs(listeria, sets):
    chosen = [listeria.files[1], listeria.files[3]]
    want = _sketch.cli_lines(chosen, by_record=True, scale=100)
    r = tool(["k", "--by-record", "--scale", "100", "--select", listeria.names[1], "--select", "flipped.fa", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 5) == want["groups"] and len(want["groups"]) == sum(len(r) for _, r in chosen) > 2 and want["summary"] in r.stdout.split("\n")
    same_pairs(lines_of(r.stdout, 8), want["pairs"])
    least = sorted(listeria.want["shared"].values())[5]              # half of the ten pairs share at least this much
    want = _sketch.cli_lines(listeria.files, min_shared=least)
    assert 0 < len(want["pairs"]) < 10
    r = tool(["k", "--min-shared", str(least), sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    same_pairs(lines_of(r.stdout, 8), want["pairs"])
    assert want["summary"] == listeria.want["summary"] and want["summary"] in r.stdout.split("\n")     # (the summary counts every pair)
    want = _sketch.cli_lines(listeria.files, no_pairs=True)
    r = tool(["k", "--no-pairs", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 5) == want["groups"] and lines_of(r.stdout, 8) == [] and want["summary"] in r.stdout.split("\n") and ", 0 pairs, 0 share" in want["summary"]


def test_the_hosts_loops_agree_and_bench_prints_its_line(listeria, sets):
    r = tool(["k", "--sketch-host", "--select", listeria.names[2], "--select", "flipped.fa", "--scale", "200", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    r = tool(["k", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout, 5) == listeria.want["groups"]
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    assert set(line) == KEYS and line["pairs"] == 10 and line["hashes"] == sum(listeria.want["sizes"]) and line["bases"] == sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert line["rows"] >= line["hashes"] and line["sketch_kernel_ms"] > 0 and line["pairs_kernel_ms"] > 0 and line["sort_ms"] > 0


def test_refusals(listeria, sets):
    s = sets("default")
    for args, word in ((["--region", "KK073979.1:1-10", s], "--region"), (["--check", s], "--check"), (["--fasta", "dir", s], "--fasta"), (["-k", "0", s], "-k 0"),
                       (["-k", "33", s], "-k 33"), (["--scale", "0", s], "--scale 0"), (["--order-out", "o.txt", "--by-record", s], "--order-out"),
                       (["--order-out", "o.txt", "--no-pairs", s], "--order-out")):
        r = tool(["k"] + args, listeria.tmp)
        assert r.returncode == 1 and "mbgc-hip k: " in r.stderr and word in r.stderr and r.stderr.count("\n") == 1 and lines_of(r.stdout, 5) == [], (args, r.stderr)
    r = tool(["k", sets("m3")], listeria.tmp)                                                     # (an -m 3 set read back without --restore-rc: d's refusal)
    assert r.returncode == 1 and "mbgc-hip k: " in r.stderr and "--restore-rc" in r.stderr and lines_of(r.stdout, 5) == [], r.stderr
    r = tool(["k", "--sketches-out", os.path.join(listeria.tmp, "no", "such", "dir", "s.tsv"), s], listeria.tmp)
    assert r.returncode == 1 and "cannot write" in r.stderr
