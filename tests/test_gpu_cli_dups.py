"""`mbgc-hip u`: which records of a stream set are the same sequence, forward or as the reverse complement, classed on the device. Five
files are made from the three Listeria genomes of tests/golden/listeria: genome 0; genome 1; genome 1's records reverse-complemented
and in reverse order; genome 0 with its longest record's last base changed; genome 2 with one record lower-cased. The sets (default
rounds, -t1, and -m 3 read back with --restore-rc) are classed and stdout, --clusters-out and --unique-files-out are held against
tests/_dups.py's lines over the FASTA text, as text. Then --unique-files-out feeds `r --select-list`, and no file of the new set is a
duplicate."""
import json
import lzma
import os
import subprocess

import pytest

import _dups

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
SETS = {"default": ([], []), "t1": (["-t1"], []), "m3": (["-m", "3"], ["--restore-rc"])}
KEYS = {"dups_kernel_ms", "verify_ms", "bases", "records", "buckets", "verified", "refuted", "decode_ms", "dups_gb_per_s"}


def tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def lines_of(stdout, tabs=5):
    return [l for l in stdout.split("\n") if l.count("\t") == tabs]


def records_of(text):
    out = []
    for block in text.split(b">")[1:]:
        header, _, body = block.partition(b"\n")
        out.append((header.decode(), body.replace(b"\n", b"")))
    return out


def fasta_of(records):
    return b"".join(b">" + h.encode() + b"\n" + b"".join(s[i:i + 70] + b"\n" for i in range(0, len(s), 70)) for h, s in records)


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the five files, their records and — computed once — the referee's lines at the defaults"""
    tmp = str(tmp_path_factory.mktemp("dups"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    raw = [lzma.open(os.path.join(LIST, f + ".xz")).read() for f in names]
    genomes = [records_of(data) for data in raw]
    flipped = [(h, _dups.revcomp(s)) for h, s in reversed(genomes[1])]
    longest = max(range(len(genomes[0])), key=lambda r: len(genomes[0][r][1]))
    changed = list(genomes[0])
    h, s = changed[longest]
    changed[longest] = (h, s[:-1] + (b"A" if s[-1:] != b"A" else b"C"))
    lowered = list(genomes[2])
    lowered[1] = (lowered[1][0], lowered[1][1].lower())
    files = [(names[0], genomes[0]), (names[1], genomes[1]), ("flipped.fa", flipped), ("changed.fa", changed), ("lowered.fa", lowered)]
    for name, data in list(zip(names[:2], raw[:2])) + [(name, fasta_of(recs)) for name, recs in files[2:]]:
        open(os.path.join(tmp, name), "wb").write(data)
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(n for n, _ in files) + "\n")
    L = type("Listeria", (), {})()
    L.tmp, L.files, L.names, L.longest = tmp, files, [n for n, _ in files], longest
    L.want = _dups.cli_lines(files)
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


def test_the_referee_sees_what_the_files_were_made_for(listeria):
    want, n = listeria.want, [len(r) for _, r in listeria.files]
    assert want["unique"] == [listeria.names[0], listeria.names[1], "changed.fa", "lowered.fa"]
    assert len(want["dups"]) == n[1] + n[3] - 1                      # all of flipped.fa (as reverse complements), all of changed.fa but its longest record
    assert sum(l.split("\t")[3] == "-" for l in want["dups"]) >= n[1] - 2 and "; 1 of 5 files duplicate" in want["summary"]
    assert len(want["clusters"]) == 2 * n[1] + 2 * (n[3] - 1) and want["clusters"][0].split("\t")[3] == "+" and want["clusters"][0].endswith("\t1")
    changed = [r[0].split()[0] for r in listeria.files[3][1]][listeria.longest]
    assert not any(l.split("\t")[0] == changed and l.split("\t")[1] == "changed.fa" for l in want["dups"])     # one base in 3 Mb: not the same sequence


@pytest.mark.parametrize("mode", ["default", "t1", "m3"])
def test_every_line_equals_the_referees(listeria, sets, mode):
    r = tool(["u", "--clusters-out", "clusters.tsv", "--unique-files-out", "unique.txt"] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == listeria.want["dups"] and listeria.want["summary"] in r.stdout.split("\n")
    assert read(listeria, "clusters.tsv") == listeria.want["clusters"] and read(listeria, "unique.txt") == listeria.want["unique"]


def test_forward_only_exact_case_and_min_len(listeria, sets):
    s = sets("default")
    want = _dups.cli_lines(listeria.files, forward_only=True)
    assert "flipped.fa" in want["unique"] and len(want["dups"]) < len(listeria.want["dups"])      # (the third file stops being a duplicate)
    r = tool(["u", "--forward-only", "--unique-files-out", "unique_fw.txt", s], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == want["dups"] and want["summary"] in r.stdout.split("\n") and read(listeria, "unique_fw.txt") == want["unique"]
    want = _dups.cli_lines(listeria.files, exact_case=True)
    r = tool(["u", "--exact-case", "--clusters-out", "clusters_ec.tsv", s], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == want["dups"] and want["summary"] in r.stdout.split("\n") and read(listeria, "clusters_ec.tsv") == want["clusters"]
    lens = sorted(int(l.split("\t")[2]) for l in listeria.want["dups"])
    least = lens[len(lens) // 2] + 1
    want = _dups.cli_lines(listeria.files, min_len=least)
    assert 0 < len(want["dups"]) < len(listeria.want["dups"])
    r = tool(["u", "--min-len", str(least), "--clusters-out", "clusters_ml.tsv", s], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == want["dups"] and want["summary"] in r.stdout.split("\n") and read(listeria, "clusters_ml.tsv") == want["clusters"]


def test_case_only_difference_is_a_duplicate_unless_exact_case(listeria, sets):
    """genome 2 beside its copy with one record lower-cased: a duplicate file without --exact-case, none with it"""
    tmp = listeria.tmp
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    open(os.path.join(tmp, names[2]), "wb").write(lzma.open(os.path.join(LIST, names[2] + ".xz")).read())
    open(os.path.join(tmp, "list2.txt"), "w").write(names[2] + "\nlowered.fa\n")
    r = tool(["c", "list2.txt", "pair"], tmp)
    assert r.returncode == 0, r.stderr
    files = [(names[2], records_of(open(os.path.join(tmp, names[2]), "rb").read())), listeria.files[4]]
    for args, kw, uniq in (([], {}, 1), (["--exact-case"], {"exact_case": True}, 2)):
        want = _dups.cli_lines(files, **kw)
        assert len(want["unique"]) == uniq
        r = tool(["u"] + args + ["--unique-files-out", "unique2.txt", "pair"], tmp)
        assert r.returncode == 0, r.stderr
        assert lines_of(r.stdout) == want["dups"] and want["summary"] in r.stdout.split("\n") and read(listeria, "unique2.txt") == want["unique"]


def test_select_composes_and_the_hosts_map_agrees(listeria, sets):
    chosen = [listeria.files[1], listeria.files[2]]
    want = _dups.cli_lines(chosen)
    assert len(want["dups"]) == len(chosen[0][1]) and want["unique"] == [listeria.names[1]]
    r = tool(["u", "--select", listeria.names[1], "--select", "flipped.fa", "--dups-host", "--unique-files-out", "unique_sel.txt", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == want["dups"] and want["summary"] in r.stdout.split("\n") and read(listeria, "unique_sel.txt") == want["unique"]
    r = tool(["u", "--dups-host", "--restore-rc", sets("m3")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == listeria.want["dups"]


def test_bench_prints_its_line(listeria, sets):
    r = tool(["u", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert lines_of(r.stdout) == listeria.want["dups"]
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    assert set(line) == KEYS and line["records"] == sum(len(r) for _, r in listeria.files) and line["bases"] == sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert line["verified"] >= len(listeria.want["dups"]) and line["dups_kernel_ms"] > 0 and line["verify_ms"] > 0 and line["buckets"] <= line["records"]


def test_refusals(listeria, sets):
    s = sets("default")
    for args, word in ((["--region", "KK073979.1:1-10", s], "--region"), (["--check", s], "--check"), (["--fasta", "dir", s], "--fasta"), (["--min-len", "x", s], "--min-len")):
        r = tool(["u"] + args, listeria.tmp)
        assert r.returncode == 1 and "mbgc-hip u: " in r.stderr and word in r.stderr and r.stderr.count("\n") == 1 and lines_of(r.stdout) == [], (args, r.stderr)
    r = tool(["u", sets("m3")], listeria.tmp)                                                     # (an -m 3 set read back without --restore-rc: d's refusal)
    assert r.returncode == 1 and "mbgc-hip u: " in r.stderr and "--restore-rc" in r.stderr and lines_of(r.stdout) == [], r.stderr
    r = tool(["u", "--clusters-out", os.path.join(listeria.tmp, "no", "such", "dir", "c.tsv"), s], listeria.tmp)
    assert r.returncode == 1 and "cannot write" in r.stderr


def test_unique_files_feed_a_repack_without_duplicates(listeria, sets):
    r = tool(["u", "--unique-files-out", "keep.txt", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    r = tool(["r", "--select-list", "keep.txt", sets("default"), "kept"], listeria.tmp)
    assert r.returncode == 0, r.stderr
    keep = read(listeria, "keep.txt")
    want = _dups.cli_lines([f for f in listeria.files if f[0] in keep])
    r = tool(["u", "--unique-files-out", "keep2.txt", "kept"], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert "; 0 of %d files duplicate" % len(keep) in r.stdout and want["summary"] in r.stdout.split("\n") and lines_of(r.stdout) == want["dups"]
    assert read(listeria, "keep2.txt") == keep == listeria.want["unique"]
