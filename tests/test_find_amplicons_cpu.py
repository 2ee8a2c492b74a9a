"""The pairing of `mbgc-hip f --primers` without a GPU: mbgc_amd/host/mbgc_find_amplicons.h pulls in no decoder type, so
tests/find_amplicons_main.cpp compiles it alone, with AddressSanitizer and UBSan, and this file holds its products against a double
loop written from the rule: a `+` product is a FWD `+` hit at [s1, e1] and a REV `-` hit at [s2, e2] of one record and one pair with
s1 <= s2, e1 <= e2 and min <= e2 - s1 + 1 <= max; a `-` product the same with REV `+` on the left and FWD `-` on the right; every such
pair of hits is a product; sorted by record, start, end, pair, + before -."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FWD_PLUS, FWD_MINUS, REV_PLUS, REV_MINUS = 0, 1, 2, 3


def double_loop(hits, lo, hi):
    out = []
    for left_role, right_role, strand in ((FWD_PLUS, REV_MINUS, "+"), (REV_PLUS, FWD_MINUS, "-")):
        for rec, s1, n1, pair1, role1, d1 in hits:
            for rec2, s2, n2, pair2, role2, d2 in hits:
                if (role1, role2) != (left_role, right_role) or rec != rec2 or pair1 != pair2 or n1 == 0 or n2 == 0:
                    continue
                e1, e2 = s1 + n1 - 1, s2 + n2 - 1
                if s1 <= s2 and e1 <= e2 and lo <= e2 - s1 + 1 <= hi:
                    out.append((rec, s1, e2, pair1, strand == "-", d1, d2, strand))
    return ["%d %d %d %d %s %d %d" % (rec, pair, s, e, strand, d1, d2) for rec, s, e, pair, _, d1, d2, strand in sorted(out)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("amplicons") / "pair")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path,
                    os.path.join(HERE, "find_amplicons_main.cpp")], check=True, capture_output=True, text=True, timeout=300)
    return path


def run(exe, cases):
    """cases: [(hits, min, max)] -> the program's products per case"""
    text = "".join("%d %d %d\n%s" % (lo, hi, len(hits), "".join("%d %d %d %d %d %d\n" % h for h in hits)) for hits, lo, hi in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = [], []
    for line in r.stdout.split("\n")[:-1]:
        if line.startswith("end "):
            assert int(line.split()[1]) == len(cur)
            out.append(cur)
            cur = []
        else:
            cur.append(line)
    assert len(out) == len(cases)
    return out


def test_the_named_cases(exe):
    F, f, R, r = FWD_PLUS, FWD_MINUS, REV_PLUS, REV_MINUS
    cases = [
        # a + product and a - product of one pair in one record; the same hits in another record and under another pair give nothing across
        ([(0, 100, 20, 0, F, 0), (0, 380, 20, 0, r, 1), (0, 1000, 20, 0, R, 2), (0, 1280, 20, 0, f, 0), (1, 100, 20, 0, F, 0), (2, 380, 20, 0, r, 0), (0, 100, 20, 1, F, 0)], 0, 5000),
        # FWD-FWD and REV-REV are no products
        ([(0, 100, 20, 0, F, 0), (0, 380, 20, 0, f, 0), (0, 100, 20, 0, R, 0), (0, 380, 20, 0, r, 0)], 0, 250),
        # exactly min and max, and one beyond each: products of 300, 301 (kept at min 300 .. max 301), 299 and 302 (dropped)
        ([(0, 0, 20, 0, F, 0), (0, 279, 20, 0, r, 0), (0, 280, 20, 0, r, 1), (0, 281, 20, 0, r, 2), (0, 282, 20, 0, r, 3)], 300, 301),
        # s1 = s2: the primers overlap wholly (e1 <= e2 holds for the longer right one, not for the shorter)
        ([(0, 50, 20, 0, F, 0), (0, 50, 25, 0, r, 0), (0, 50, 20, 0, r, 1), (0, 50, 18, 0, r, 2)], 0, 5000),
        # overlapping primers: the right one starts inside the left one; one that starts in front of it is no product
        ([(0, 50, 20, 0, F, 0), (0, 60, 20, 0, r, 0), (0, 45, 30, 0, r, 0)], 0, 5000),
        # several products share a left hit, several a right hit: every pair is a product, not only the nearest
        ([(0, 10, 20, 0, F, 0), (0, 40, 20, 0, F, 1), (0, 300, 20, 0, r, 0), (0, 700, 20, 0, r, 0), (0, 1500, 20, 0, r, 2)], 0, 1000),
        # the right primer in front of the left one: nothing
        ([(0, 500, 20, 0, F, 0), (0, 100, 20, 0, r, 0)], 0, 5000),
        ([], 0, 5000),
        # the whole range of the numbers
        ([(4294967294, 2 ** 62, 4000000000, 4294967294, F, 3), (4294967294, 2 ** 62 + 5, 4000000000, 4294967294, r, 3)], 0, 2 ** 64 - 1),
    ]
    got = run(exe, cases)
    want = [double_loop(h, lo, hi) for h, lo, hi in cases]
    assert got == want
    assert [len(w) for w in want] == [2, 0, 2, 2, 1, 4, 0, 0, 1]     # (the sixth: two lefts x two rights, the third right is too far)
    assert want[0] == ["0 0 100 399 + 0 1", "0 0 1000 1299 - 2 0"]
    assert want[2] == ["0 0 0 299 + 0 1", "0 0 0 300 + 0 2"]


def test_random_hit_lists_equal_the_double_loop(exe):
    rng = np.random.default_rng(41)
    cases = []
    for it in range(300):
        n = int(rng.integers(0, 150))
        span = int(rng.choice([60, 400, 5000]))
        hits = [(int(rng.integers(0, 2)), int(rng.integers(0, span)), int(rng.choice([0, 8, 18, 20, 24, 33])), int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 4)))
                for _ in range(n)]
        lo = int(rng.choice([0, 1, 20, 50, 300]))
        hi = lo + int(rng.choice([0, 1, 30, 400, 10000]))
        cases.append((hits, lo, hi))
    got = run(exe, cases)
    want = [double_loop(h, lo, hi) for h, lo, hi in cases]
    assert sum(len(w) for w in want) > 2000 and sum(1 for w in want if any(l.split()[4] == "-" for l in w)) > 50
    assert got == want
