"""`mbgc-hip f`: query sequences found in a stream set on the device. The three Listeria genomes of tests/golden/listeria are unpacked,
compressed with `mbgc-hip c` (default rounds, -t1, and -m 3 — read back with --restore-rc) and searched; the TSV is held line for line
against tests/_find.py's brute force over the records of the unpacked FASTA files. The queries are cut from the genomes here: forward
30-mers, the reverse complement of others, one with two substitutions (--mismatches 2), a 30-mer that stands nowhere, and a query that
is its own reverse complement. For every class the referee's own lines are held non-empty before the comparison."""
import json
import lzma
import os
import subprocess

import numpy as np
import pytest

import _find

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
SETS = {"default": ([], []), "t1": (["-t1"], []), "m3": (["-m", "3"], ["--restore-rc"])}


def tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def tsv(stdout):
    return [l for l in stdout.split("\n") if l.count("\t") == 6]


def records_of(text):
    out = []
    for block in text.split(b">")[1:]:
        header, _, body = block.partition(b"\n")
        out.append((header.decode(), body.replace(b"\n", b"")))
    return out


@pytest.fixture(scope="module")
def listeria(tmp_path_factory):
    """the unpacked files, their records, the queries and — computed once — the referee's lines"""
    tmp = str(tmp_path_factory.mktemp("find"))
    names = sorted(f[:-3] for f in os.listdir(LIST) if f.endswith(".xz"))
    files = []
    for f in names:
        data = lzma.open(os.path.join(LIST, f + ".xz")).read()
        open(os.path.join(tmp, f), "wb").write(data)
        files.append((f, records_of(data)))
    open(os.path.join(tmp, "list.txt"), "w").write("\n".join(names) + "\n")

    longest = [max(range(len(recs)), key=lambda r: len(recs[r][1])) for _, recs in files]

    def cut(f, at, n=30):
        q = files[f][1][longest[f]][1][at:at + n].upper()
        assert len(q) == n and set(q) <= set(b"ACGT")
        return q

    rng = np.random.default_rng(1)
    two = bytearray(cut(0, 300_000))
    for j in (4, 21):
        two[j] = {65: 67, 67: 71, 71: 84, 84: 65}[two[j]]
    big = files[0][1][longest[0]][1].upper()
    own = next(big[p:p + 10] for p in range(len(big) - 10) if big[p:p + 10] == _find.reverse_complement(big[p:p + 10]))
    L = type("Listeria", (), {})()
    L.tmp, L.files, L.names = tmp, files, names
    L.forward = [("fwd_a", cut(0, 100_000)), ("fwd_b", cut(2, 5_000).lower())]
    L.reverse = [("rev_a", _find.reverse_complement(cut(1, 200_000))), ("rev_b", _find.reverse_complement(cut(2, 50_000)))]
    L.two = [("two_subs", bytes(two))]
    L.absent = [("absent", np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30)].tobytes())]
    L.own = [("own_rc", own)]
    L.exact = L.forward + L.reverse + L.absent + L.own
    open(os.path.join(tmp, "exact.fa"), "w").write("".join(">%s some words\n%s\n%s\n" % (n, q[:17].decode(), q[17:].decode()) for n, q in L.exact))
    L.want = _find.cli_lines(files, L.exact, 0)
    by_query = {n: [l for l in L.want if l.split("\t")[0] == n] for n, _ in L.exact}
    # every class of query has lines of its own in the referee's table, and of the right kind
    assert all(any(l.split("\t")[5] == "+" for l in by_query[n]) for n, _ in L.forward), by_query
    assert all(any(l.split("\t")[5] == "-" for l in by_query[n]) for n, _ in L.reverse), by_query
    assert by_query["own_rc"] and all(l.split("\t")[5] == "+" for l in by_query["own_rc"]) and not by_query["absent"]
    L.want_two = _find.cli_lines(files, L.two + L.forward[:1], 2)
    assert any(l.startswith("two_subs\t") and l.endswith("\t2") for l in L.want_two) and any(l.startswith("fwd_a\t") and l.endswith("\t0") for l in L.want_two)
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


@pytest.mark.parametrize("mode", list(SETS))
def test_the_lines_equal_the_brute_force(listeria, sets, mode):
    r = tool(["f", "--seq-file", "exact.fa"] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == listeria.want
    records = {tuple(l.split("\t")[1:3]) for l in listeria.want}
    bases = sum(len(s) for _, recs in listeria.files for _, s in recs)
    assert "hits: %d in %d records of %d files; %d bases searched, %d patterns\n" % (len(listeria.want), len(records), len({f for f, _ in records}), bases,
                                                                                      2 * len(listeria.exact) - 1) in r.stdout


@pytest.mark.parametrize("mode", list(SETS))
def test_two_substitutions(listeria, sets, mode):
    r = tool(["f", "--mismatches", "2", "--seq", listeria.two[0][1].decode(), "--seq", listeria.forward[0][1].decode()] + SETS[mode][1] + [sets(mode)], listeria.tmp)
    assert r.returncode == 0, r.stderr
    renamed = [l.replace("two_subs\t", "q1\t", 1).replace("fwd_a\t", "q2\t", 1) for l in listeria.want_two]     # (--seq names them by their place)
    assert tsv(r.stdout) == renamed


def test_forward_only_and_a_hits_file(listeria, sets):
    want = _find.cli_lines(listeria.files, listeria.exact, 0, forward_only=True)
    assert want and len(want) < len(listeria.want)
    r = tool(["f", "--seq-file", "exact.fa", "--forward-only", "--hits", "hits.tsv", sets("default")], listeria.tmp)
    assert r.returncode == 0 and tsv(r.stdout) == [], r.stderr
    assert open(os.path.join(listeria.tmp, "hits.tsv")).read().split("\n")[:-1] == want


def test_select_searches_the_chosen_file_only(listeria, sets):
    """the second file's contigs depend on the first file's: those are decoded, and not searched"""
    name = listeria.names[1]
    want = [l for l in listeria.want if l.split("\t")[1] == name]
    assert want and len(want) < len(listeria.want)
    r = tool(["f", "--seq-file", "exact.fa", "--select", name, sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == want


def test_a_hit_buffer_of_one_row_and_the_hosts_loop_agree(listeria, sets):
    r = tool(["f", "--seq-file", "exact.fa", "--hit-capacity", "1", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == listeria.want
    line = json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])
    assert line["retries"] == 1 and line["hits"] == len(listeria.want) and line["patterns"] == 2 * len(listeria.exact) - 1
    assert set(line) >= {"find_kernel_ms", "bases_searched", "patterns", "hits", "retries", "decode_ms", "find_gb_per_s"}
    r = tool(["f", "--seq-file", "exact.fa", "--find-host", "--bench", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert tsv(r.stdout) == listeria.want
    assert json.loads([l for l in r.stdout.split("\n") if l.startswith("{")][-1])["find_host_ms"] > 0


def test_no_hit_is_exit_status_3(listeria, sets):
    r = tool(["f", "--seq", listeria.absent[0][1].decode(), sets("default")], listeria.tmp)
    assert r.returncode == 3 and tsv(r.stdout) == [] and "hits: 0 in 0 records of 0 files" in r.stdout, r.stderr


def test_refusals(listeria, sets):
    q = listeria.forward[0][1].decode()
    for args, word in ((["--seq", q, "--region", "KK073979.1:1-10", sets("default")], "--region"),
                       (["--seq", "ACGTACG", sets("default")], "query q1 has 7 bases"),
                       (["--seq", q, "--seq", "ACGTNNNN-ACGT", sets("default")], "query q2 holds a byte that is no letter"),
                       (["--seq", q * 2, "--mismatches", "3", "--seq", (q * 2)[:31], sets("default")], "query q2 has 31 bases"),
                       (["--seq", q, "--check", sets("default")], "--check"),
                       (["--seq", q, sets("m3")], "--restore-rc")):
        r = tool(["f"] + args, listeria.tmp)
        assert r.returncode == 1 and "mbgc-hip f: " in r.stderr and word in r.stderr and tsv(r.stdout) == [], (args, r.stderr)
    for letter, rest in (("d", ["out_d"]), ("t", []), ("v", [])):                                   # the other commands do not take f's options
        r = tool([letter, "--seq", q, sets("default")] + rest, listeria.tmp)
        assert r.returncode == 1 and "usage" in r.stderr, (letter, r.stderr)


def test_regions_out_feeds_d_region_list(listeria, sets):
    name, q = listeria.forward[0]
    want = [l for l in _find.cli_lines(listeria.files, [("q1", q)], 0, forward_only=True)]
    assert want
    r = tool(["f", "--seq", q.decode(), "--forward-only", "--regions-out", "r.txt", sets("default")], listeria.tmp)
    assert r.returncode == 0 and tsv(r.stdout) == want, r.stderr
    regions = open(os.path.join(listeria.tmp, "r.txt")).read().split("\n")[:-1]
    assert regions == list(dict.fromkeys("%s:%s-%s" % tuple(l.split("\t")[2:5]) for l in want))
    r = tool(["d", "--region-list", "r.txt", sets("default"), "back"], listeria.tmp)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(listeria.tmp, "back.seq"), "rb").read().upper() == q.upper() * len(regions)
    # --flank: the piece grows on both sides and stops at the record's first base
    r = tool(["f", "--seq", q.decode(), "--forward-only", "--regions-out", "flank.txt", "--flank", "1000000000", sets("default")], listeria.tmp)
    assert r.returncode == 0, r.stderr
    flank = open(os.path.join(listeria.tmp, "flank.txt")).read().split("\n")[:-1]
    assert flank == list(dict.fromkeys("%s:1-%d" % (l.split("\t")[2], int(l.split("\t")[4]) + 10 ** 9) for l in want))
