"""What `mbgc-hip m` refuses before anything is decoded: exit status 1, nothing on stdout, and one line on stderr that names what is
wrong (or the usage text). No stream set is read and no device is opened — the prefix `x` does not exist, and a command line that passes
every refusal fails on exactly that, the missing x.meta, which is read in front of the device: the refusals stand in front of the
decode, as those of tests/test_cli_scan_refusals.py do."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
GENE = "ACGTTGCAAGGCTTAACCGGATCCATGCAAGT"                               # 32 letters
SEQ = ["--seq", GENE]

CASES = {
    "--region": (SEQ + ["--region", "x:1-2", "x"], ["--region / --region-list select parts of records", "a screen looks at whole records"]),
    "--region-list": (SEQ + ["--region-list", "regions.txt", "x"], ["--region / --region-list select parts of records"]),
    "--check": (SEQ + ["--check", "x"], ["--check is an option of mbgc-hip d"]),
    "--fasta": (SEQ + ["--fasta", "dir", "x"], ["--fasta is an option of mbgc-hip d", "m writes no sequence"]),
    "a query shorter than k": (["--seq", GENE[:20], "x"], ["query q1 has 20 bases, fewer than k = 21"]),
    "the second query shorter than -k": (SEQ + ["--seq", GENE[:30], "-k", "31", "x"], ["query q2 has 30 bases, fewer than k = 31"]),
    "a query without a valid k-mer": (["--seq", GENE[:15] + "N" + GENE[:15], "x"], ["query q1 has no k-mer of 21 letters"]),
    "a query of a file without a valid k-mer": (["--seq-file", "genes.fa", "x"], ["query gapped has no k-mer of 21 letters"]),
    "a query file that is not there": (["--seq-file", "none.fa", "x"], ["cannot open the query file none.fa"]),
    "-k 0": (SEQ + ["-k", "0", "x"], ["-k 0: a k-mer has 1 to 32 bases"]),
    "-k 33": (SEQ + ["-k", "33", "x"], ["-k 33: a k-mer has 1 to 32 bases"]),
    "-k that is no number": (SEQ + ["-k", "2a", "x"], ["-k takes a number"]),
    "--min-shared that is no number": (SEQ + ["--min-shared", "x1", "x"], ["--min-shared takes a number"]),
    "--min-containment above 1": (SEQ + ["--min-containment", "1.5", "x"], ["--min-containment takes a fraction from 0 to 1"]),
    "--min-containment that is no number": (SEQ + ["--min-containment", "half", "x"], ["--min-containment takes a fraction from 0 to 1"]),
    "--max-gap that is no number": (SEQ + ["--loci-out", "l.tsv", "--max-gap", "-5", "x"], ["--max-gap takes a number of bases"]),
    "--min-locus-hits 0": (SEQ + ["--loci-out", "l.tsv", "--min-locus-hits", "0", "x"], ["--min-locus-hits 0"]),
    "--hit-capacity 0": (SEQ + ["--loci-out", "l.tsv", "--hit-capacity", "0", "x"], ["--hit-capacity takes a positive number of hits"]),
    "--flank without a list to write": (SEQ + ["--flank", "100", "x"], ["--flank", "go with --loci-out or --regions-out"]),
    "--max-gap without a list to write": (SEQ + ["--max-gap", "100", "x"], ["--max-gap", "go with --loci-out or --regions-out"]),
    "an empty --select": (SEQ + ["--select", "", "x"], ["--select"]),
}
USAGE = {"no query": ["x"], "no prefix": SEQ, "two prefixes": SEQ + ["x", "y"], "an unknown option": SEQ + ["--strand", "x"]}


@pytest.mark.parametrize("case", list(CASES))
def test_refusal(case, tmp_path):
    args, words = CASES[case]
    open(str(tmp_path / "genes.fa"), "w").write(">whole a gene\n%s\n>gapped\n%sN\n%s\n" % (GENE, GENE[:18], GENE[:20]))
    open(str(tmp_path / "regions.txt"), "w").write("x:1-2\n")
    r = subprocess.run([TOOL, "m"] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert r.stderr.startswith("mbgc-hip m: ") and r.stderr.count("\n") == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "HIP" not in r.stderr and "device" not in r.stderr and ".meta" not in r.stderr      # (refused in front of the decode)


@pytest.mark.parametrize("case", list(USAGE))
def test_usage(case, tmp_path):
    r = subprocess.run([TOOL, "m"] + USAGE[case], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: mbgc-hip m [--seq"), r.stderr
    for w in ("--seq-file", "--by-record", "--min-containment", "--loci-out", "--regions-out", "--max-gap", "--min-locus-hits", "--hit-capacity", "--screen-host", "NO STRAND",
              "a canonical k-mer has none", "2^24"):
        assert w in r.stderr, w


def test_more_than_2_to_the_24_distinct_keys(tmp_path):
    """a query of 2^24 + 30 random bases at k = 31 has more than 2^24 distinct k-mers (a repeat among them is as good as impossible)"""
    import numpy as np
    rng = np.random.default_rng(71)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (1 << 24) + 30 + 1000)].tobytes().decode()
    open(str(tmp_path / "big.fa"), "w").write(">big\n" + "\n".join(seq[i:i + 10000] for i in range(0, len(seq), 10000)) + "\n")
    r = subprocess.run([TOOL, "m", "--seq-file", "big.fa", "-k", "31", "x"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("mbgc-hip m: the queries have ") and "more than 2^24" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_a_command_line_that_passes_fails_on_the_missing_set_and_opens_no_device(tmp_path):
    """every refusal above stands in front of this one: the streams are read in front of the device"""
    r = subprocess.run([TOOL, "m"] + SEQ + ["--loci-out", "l.tsv", "--max-gap", "100", "--min-containment", "0.5", "x"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("mbgc-hip m: cannot open x.meta"), r.stderr
    assert not os.path.exists(str(tmp_path / "l.tsv"))
