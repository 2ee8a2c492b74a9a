"""The keys and the chaining of `mbgc-hip m` without a GPU: mbgc_amd/host/mbgc_screen_loci.h pulls in no decoder type and no device, so
tests/screen_loci_main.cpp compiles it alone, with AddressSanitizer and UBSan, and this file holds its key lists and its loci against
tests/_screen.py, which is written from the rule: a query's hit positions in a record, ascending, cut wherever two neighbours are MORE
than max-gap apart; a piece of at least min-locus-hits positions is a locus from its first position to its last position + k - 1, with
`hits` positions and `distinct` different keys. The records here are stretches of a query laid into N (which has no k-mer), so every
hit position is placed by hand."""
import os
import subprocess

import numpy as np
import pytest

import _screen

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("loci") / "chain")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path,
                    os.path.join(HERE, "screen_loci_main.cpp")], check=True, capture_output=True, text=True, timeout=300)
    return path


def lay(length, pieces):
    """a record of `length` N with the byte strings of pieces = [(position, bytes)] laid in"""
    rec = bytearray(b"N" * length)
    for at, text in pieces:
        rec[at:at + len(text)] = text
    return bytes(rec)


def run(exe, cases):
    """cases: [(queries, records, k, max_gap, min_hits, flank)] -> per case (the program's answer, the referee's), each (keys, own, loci
    rows (query, rec, start, end, hits, distinct), region lines)"""
    text, want = "", []
    for queries, records, k, max_gap, min_hits, flank in cases:
        keys, own = _screen.key_set(queries, k)
        _, hits = _screen.screen(records, [0] * len(records), 1, keys, k)
        text += "%d %d %d %d %d %d\n%s%s" % (k, max_gap, min_hits, flank, len(queries), len(hits), "".join(q.decode() + "\n" for q in queries), "".join("%d %d %d\n" % h for h in hits))
        rows = _screen.loci(hits, keys, own, k, max_gap, min_hits)
        want.append(([int(x) for x in keys], [int(o.size) for o in own], rows, [_screen.region_line("r%d" % r[1], r[2], r[3], flank) for r in rows]))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got, cur = [], None
    for line in r.stdout.split("\n")[:-1]:
        w = line.split()
        if w[0] == "keys":
            cur = ([int(x, 16) for x in w[1:]], None, [], [])
        elif w[0] == "own":
            cur = (cur[0], [int(x) for x in w[1:]], [], [])
        elif w[0] == "end":
            assert int(w[1]) == len(cur[2])
            got.append(cur)
        else:
            cur[2].append(tuple(int(x) for x in w[:6]))
            cur[3].append(w[6])
    assert len(got) == len(cases)
    return got, want


def test_the_named_cases(exe):
    rng = np.random.default_rng(61)
    k, G = 8, 50
    Q = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 60))
    other = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 30))
    a, b = Q[0:12], Q[20:32]                                         # 5 k-mers each: positions at .. at + 4
    cases = [
        # the last position of a is 104, the first of b 104 + G: exactly max-gap, one locus of 10
        ([Q], [lay(400, [(100, a), (104 + G, b)])], k, G, 3, 0),
        # ... and one more: two loci of 5
        ([Q], [lay(400, [(100, a), (105 + G, b)])], k, G, 3, 0),
        # a piece of k + 1 bytes has two positions: one short of three; with --min-locus-hits 2 it is a locus
        ([Q], [lay(400, [(100, a), (300, Q[40:49])])], k, G, 3, 0),
        ([Q], [lay(400, [(100, a), (300, Q[40:49])])], k, G, 2, 0),
        # two queries that share keys: the second holds Q[10:40]; b is a locus of both, a of the first alone, `other` of the second
        ([Q, Q[10:40] + b"N" + other], [lay(600, [(100, a), (250, b), (450, other[:14])])], k, G, 3, 0),
        # a key twice inside one locus: 10 positions, 5 distinct keys
        ([Q], [lay(400, [(100, a), (120, a)])], k, G, 3, 0),
        # a flank that reaches in front of the record: FROM is clamped at 1; the second record's locus keeps its flank
        ([Q], [lay(200, [(2, a)]), lay(300, [(150, b)])], k, G, 3, 10),
        # no hit at all, and a query met only as its reverse complement
        ([Q], [lay(100, [])], k, G, 3, 0),
        ([Q], [lay(300, [(100, _screen.reverse_complement(a))])], k, G, 3, 5),
    ]
    got, want = run(exe, cases)
    assert got == want
    rows = [w[2] for w in want]
    assert rows[0] == [(0, 0, 100, 104 + G + 4 + k - 1, 10, 10)]
    assert rows[1] == [(0, 0, 100, 104 + k - 1, 5, 5), (0, 0, 105 + G, 109 + G + k - 1, 5, 5)]
    assert rows[2] == [(0, 0, 100, 111, 5, 5)] and rows[3] == [(0, 0, 100, 111, 5, 5), (0, 0, 300, 301 + k - 1, 2, 2)]
    assert [r[:2] + r[4:] for r in rows[4]] == [(0, 0, 5, 5), (0, 0, 5, 5), (1, 0, 5, 5), (1, 0, 7, 7)] and want[4][1] == [53, 23 + 23]
    assert rows[5] == [(0, 0, 100, 124 + k - 1, 10, 5)]
    assert want[6][3] == ["r0:1-24", "r1:141-172"]
    assert rows[7] == [] and rows[8] == [(0, 0, 100, 111, 5, 5)] and want[8][3] == ["r0:96-117"]


def test_random_layouts_equal_the_referee(exe):
    rng = np.random.default_rng(67)
    letters = np.frombuffer(b"ACGTacgtU", dtype=np.uint8)
    cases = []
    for it in range(120):
        k = int(rng.choice([1, 3, 8, 21, 32]))
        queries = [bytes(rng.choice(letters, int(rng.integers(k, k + 80)))) for _ in range(int(rng.integers(1, 4)))]
        if it % 3 == 0:
            queries.append(queries[0][len(queries[0]) // 3:] + b"n" + queries[-1][:k + 5])          # shares keys with two others
        records = []
        for _ in range(int(rng.integers(1, 4))):
            pieces = []
            for _ in range(int(rng.integers(0, 12))):
                q = queries[int(rng.integers(0, len(queries)))]
                lo = int(rng.integers(0, len(q)))
                piece = q[lo:lo + int(rng.integers(1, 50))]
                pieces.append((int(rng.integers(0, 900)), _screen.reverse_complement(piece) if rng.integers(0, 2) else piece))
            records.append(lay(1000, pieces))
        cases.append((queries, records, k, int(rng.choice([0, 1, 10, 60, 500])), int(rng.choice([1, 2, 3, 8])), int(rng.choice([0, 7, 2000]))))
    got, want = run(exe, cases)
    assert sum(len(w[2]) for w in want) > 300 and sum(1 for w in want if any(r[4] != r[5] for r in w[2])) > 10
    assert got == want
