"""What `mbgc-hip f --iupac` and `f --primers` refuse before anything is decoded: exit status 1, nothing on stdout, and a line on
stderr that names what is wrong. No stream set is read and no device is opened (the prefix `x` does not exist): the refusals stand in
front of the decode, as those of tests/test_cli_scan_refusals.py do."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
FWD, REV = "GTGYCAGCMGCCGCGGTAA", "GGACTACNVGGGTWTCTAAT"                # 19 and 20 letters

CASES = {
    "a letter outside the table under --iupac": (["--iupac", "--seq", "ACGTRYACGTEACGT", "x"], ["query q1 holds 'E'", "no IUPAC letter"]),
    "a byte that is no letter under --iupac": (["--iupac", "--seq", "ACGTRYAC-GTACGT", "x"], ["query q1 holds '-'", "no IUPAC letter"]),
    "a letter outside the table in a primer": (["--primers", "v4:%s:%s" % (FWD, REV.replace("W", "X")), "x"], ["primer v4.rev holds 'X'", "no IUPAC letter"]),
    "a query too short for K under --iupac": (["--iupac", "--mismatches", "1", "--seq", "ACGTRYACGTACGTN", "x"], ["query q1 has 15 letters", "8 (1 + 1) = 16"]),
    "a primer too short for K": (["--primers", "v4:%s:%s" % (FWD, REV), "--mismatches", "2", "x"], ["primer v4.fwd has 19 letters", "--mismatches 2", "8 (2 + 1) = 24"]),
    "a 20-mer allows one mismatch, not two": (["--primers", "p:%s:%s" % (REV, REV), "--mismatches", "2", "x"], ["primer p.fwd has 20 letters", "8 (2 + 1) = 24"]),
    "--primers with --seq": (["--primers", "v4:%s:%s" % (FWD, REV), "--seq", "ACGTACGTAC", "x"], ["--primers", "--seq"]),
    "--primers with --seq-file": (["--primers", "v4:%s:%s" % (FWD, REV), "--seq-file", "queries.fa", "x"], ["--primers", "--seq-file"]),
    "NAME:FWD:REV with two parts": (["--primers", "v4:%s" % FWD, "x"], ["--primers takes NAME:FWD:REV", "v4:" + FWD]),
    "NAME:FWD:REV with four parts": (["--primers", "v4:%s:%s:%s" % (FWD, REV, REV), "x"], ["--primers takes NAME:FWD:REV"]),
    "NAME:FWD:REV with an empty part": (["--primers", "v4::%s" % REV, "x"], ["--primers takes NAME:FWD:REV"]),
    "--max-amplicon below --min-amplicon": (["--primers", "v4:%s:%s" % (FWD, REV), "--min-amplicon", "500", "--max-amplicon", "499", "x"],
                                            ["--max-amplicon 499 is below --min-amplicon 500"]),
    "--max-amplicon below the default of --min-amplicon is fine, a count that is none is not": (["--primers", "v4:%s:%s" % (FWD, REV), "--max-amplicon", "12a", "x"],
                                                                                               ["--max-amplicon takes a number of bases"]),
    "--amplicons-out without --primers": (["--iupac", "--seq", "ACGTRYACGT", "--amplicons-out", "a.txt", "x"], ["--amplicons-out", "--primers"]),
    "--primers with --forward-only": (["--primers", "v4:%s:%s" % (FWD, REV), "--forward-only", "x"], ["--forward-only"]),
    "a malformed line of a primer file": (["--primer-file", "primers.tsv", "x"], ["primers.tsv, line 2", "name<TAB>fwd<TAB>rev"]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_refusal(case, tmp_path):
    args, words = CASES[case]
    open(str(tmp_path / "queries.fa"), "w").write(">a\nACGTACGTACGT\n")
    open(str(tmp_path / "primers.tsv"), "w").write("v4\t%s\t%s\nv5\t%s\n" % (FWD, REV, FWD))
    r = subprocess.run([TOOL, "f"] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert r.stderr.startswith("mbgc-hip f: ") and r.stderr.count("\n") == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)


def test_the_usage_text_names_the_new_options_when_one_of_them_is_given(tmp_path):
    """... and is the text of before when none is: tests/test_cli_scan_refusals.py holds that one byte for byte"""
    r = subprocess.run([TOOL, "f", "--iupac", "x"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: mbgc-hip f [--seq")
    for w in ("--iupac", "--primers NAME:FWD:REV", "--primer-file", "--min-amplicon", "--max-amplicon", "--amplicons-out", "R = AG", "N = ACGT",
              "IN THE TEXT is a\n  mismatch against everything", "circular"):
        assert w in r.stderr, w
    plain = subprocess.run([TOOL, "f", "x"], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert plain.returncode == 1 and r.stderr.startswith(plain.stderr) and "--primers" not in plain.stderr
