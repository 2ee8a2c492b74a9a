"""What `mbgc-hip f`, `s`, `k` and `u` refuse before anything is decoded: the exit status and every byte of stderr, held against
tests/golden/scan_cli_refusals.json — this project's own output, recorded once. No stream set is read and no device is opened: the
refusals stand in front of the decode."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_cli_refusals.json")
LONG = "1234567890123456789"                                         # 19 digits: one more than a number may have
SEQ = ["--seq", "ACGTACGTAC"]


def cases():
    out = []
    for tool in "fsku":
        query = SEQ if tool == "f" else []
        out += [[tool, "--check", "x"], [tool] + query + ["--fasta", "dir", "x"], [tool] + query + ["--region", "x:1-2", "x"],
                [tool] + query, [tool] + query + ["x", "y"]]
    for tool, option in (("s", "--min-gap"), ("s", "--min-masked"), ("k", "-k"), ("k", "--scale"), ("k", "--min-shared"), ("u", "--min-len")):
        out += [[tool, option, "12a", "x"], [tool, option, LONG, "x"], [tool, option, "", "x"]]
    out += [["k", "-k", "0", "x"], ["k", "-k", "33", "x"], ["k", "--scale", "0", "x"],
            ["k", "--order-out", "order.txt", "--by-record", "x"], ["k", "--order-out", "order.txt", "--no-pairs", "x"]]
    out += [["f"] + SEQ + ["--mismatches", "4", "x"], ["f"] + SEQ + ["--mismatches", "10", "x"], ["f"] + SEQ + ["--hit-capacity", "0", "x"],
            ["f", "x"], ["f", "--seq", "ACGT", "x"], ["f", "--seq", "ACGTACG-ACGT", "x"], ["f"] + SEQ + ["-x"]]
    return out


def run(args, cwd):
    r = subprocess.run([TOOL] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)
    return {"args": args, "status": r.returncode, "stdout": r.stdout, "stderr": r.stderr}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {" ".join(row["args"]): row for row in json.load(f)}


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    assert sorted(golden) == sorted(" ".join(c) for c in cases())
    assert all(row["status"] == 1 and row["stderr"] and row["stdout"] == "" for row in golden.values())


@pytest.mark.parametrize("args", cases(), ids=lambda c: " ".join(c) or "none")
def test_refusal(args, golden, tmp_path):
    assert run(args, tmp_path) == golden[" ".join(args)]
