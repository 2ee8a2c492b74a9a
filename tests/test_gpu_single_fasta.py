"""Single fasta file mode on the GPU: mbgc_fasta_split_dev against the restatement of mgmpInSplit_next (tests/_singlefasta.py,
itself pinned on the reference CLI by tests/test_single_fasta_rule.py), and `mbgc-hip c -i` — the sequential schedule against
the reference CLI's digests, the rounds against the oracle-driven reference loop fed the restatement's elements, the window
protocol against the default window."""
import gzip
import hashlib
import json
import lzma
import os
import struct
import subprocess

import numpy as np
import pytest

import _driver
import _orc
import _singlefasta as sfa
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
STREAMS = ("literals", "mapOff", "mapOff5th", "mapLen", "gapDelta", "flags", "locksPos", "refExtSize")
MIB = 1 << 20


# ---- C: the export ------------------------------------------------------------------------------------------
class DevSplit:
    def __init__(self, data, shift=0):
        import torch
        from mbgc_amd import fasta
        self.n = len(data)
        self.buf = torch.from_numpy(np.frombuffer(b"\0" * shift + data + b"\0" * 16, dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr() + shift
        self.p = fasta.FastaParser()

    def __call__(self, n, is_end, first_min, next_min, max_elems):
        return self.p.split_dev(self.ptr, n, is_end, first_min, next_min, max_elems)


def check(data, first_min, next_min, max_elems=64, shift=0):
    d = DevSplit(data, shift)
    for is_end in (True, False):
        got = d(len(data), is_end, first_min, next_min, max_elems)
        assert got == sfa.split_window(data, is_end, first_min, next_min, max_elems), (is_end, first_min, next_min)
    d.p.close()


REC = b">a\nAC\n>b\nGT\n>c\nAA\n"           # '>' at 0, 6, 12; 18 bytes


@pytest.mark.parametrize("data,first_min,next_min", [
    (REC, 6, 6),                              # a '>' exactly at the threshold
    (REC, 7, 5),                              # one byte before the threshold: the next one counts
    (REC, 13, 2),                             # none behind it
    (b">x > y\nAC\n>z > w\nGG\n", 1, 1),      # '>' inside header lines
    (b">x > y\nAC\n>z > w\nGG\n", 2, 4),
    (REC, 18, 1), (REC, 17, 1), (REC, 19, 1),  # an element exactly n long, one byte less, the threshold behind the end
    (REC * 3, 1, 100),                        # a tail shorter than nextMin
    (REC.replace(b"\n", b"\r\n") * 400, 50, 700),   # CRLF
    (b">" * 9000, 1, 4097), (b"A" * 9000, 1, 1), (b"A" * 4095 + b">" + b"A" * 4096 + b">", 1, 4096),
])
def test_split_edge_cases(data, first_min, next_min):
    check(data, first_min, next_min)
    check(data, first_min, next_min, max_elems=2)
    check(data, first_min, next_min, shift=3)                      # (a window that starts anywhere in its buffer)


def test_split_window_that_ends_before_the_next_mark():
    """the search runs off the window: the elements found so far (none, for a contig longer than the window), then, with the
    window extended, all of them"""
    data = b">a\n" + b"ACGT" * 5000 + b"\n>b\n" + b"GG" * 3000 + b"\n>c\nAC\n"
    full = sfa.split_window(data, True, 100, 100)
    assert len(full) == 3
    d = DevSplit(data)
    assert d(15_000, False, 100, 100, 8) == []                    # inside the first contig
    assert d(full[0] + 50, False, 100, 100, 8) == full[:1]        # the second element's threshold lies behind the window
    assert d(full[0] + 3000, False, 100, 100, 8) == full[:1]      # ... its threshold inside, its end not
    assert d(len(data), False, 100, 100, 8) == full[:2]
    assert d(len(data), True, 100, 100, 8) == full


@pytest.mark.parametrize("seed,marks,first_min,next_min", [(1, 40, 1000, 50_000), (2, 4000, 65536, 200_000), (3, 3, 10, 10), (4, 100_000, 7, 4096)])
def test_split_random_bytes(seed, marks, first_min, next_min):
    rng = np.random.default_rng(seed)
    n = 3 * MIB + int(rng.integers(0, 5000))
    a = rng.integers(0, 256, n).astype(np.uint8)
    a[a == ord(">")] = ord("A")
    a[rng.integers(0, n, marks)] = ord(">")
    data = a.tobytes()
    check(data, first_min, next_min, max_elems=4096, shift=int(rng.integers(0, 16)))
    cut = int(rng.integers(n // 3, n))
    d = DevSplit(data)
    assert d(cut, False, first_min, next_min, 4096) == sfa.split_window(data[:cut], False, first_min, next_min, 4096)


def test_split_of_a_growing_buffer_scans_only_what_was_appended():
    """mbgc_fasta_split_buf_dev: the window grows call by call, the elements start at the end of the last one found, and the
    tiles of the bytes scanned before stand — the ends must be those of one call over everything"""
    rng = np.random.default_rng(11)
    n = 2 * MIB + 777
    a = rng.integers(0, 256, n).astype(np.uint8)
    a[a == ord(">")] = ord("A")
    a[rng.integers(0, n, 300)] = ord(">")
    data = a.tobytes()
    want = sfa.split_window(data, True, 5000, 60_000)
    d = DevSplit(data, shift=5)
    got, done, scanned, have = [], 0, 0, 0
    for step in (100_000, 4096, 1, 300_001, 8191, n):
        have = min(n, have + step)
        ends = d.p.split_buf_dev(d.ptr, done, have, scanned, have == n, 60_000 if got else 5000, 60_000, 1000)
        assert ends == [done + e for e in sfa.split_window(data[done:have], have == n, 60_000 if got else 5000, 60_000)]
        got += ends
        done, scanned = (ends[-1] if ends else done), have
    assert got == want


# ---- D, E: the tool -----------------------------------------------------------------------------------------
def run_tool(args, cwd, env=None):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def streams_of(tmp_path, prefix):
    return {k: (tmp_path / (prefix + "." + k)).read_bytes() for k in STREAMS}


def listeria():
    exp = json.load(open(os.path.join(LIST, "expected_t1_single.json")))
    return b"".join(lzma.open(os.path.join(LIST, f + ".xz")).read() for f in exp["files"])


@pytest.mark.parametrize("kind,args", [("t1", ["-t1"]), ("m3", ["-m", "3", "-t1"])])
def test_listeria_sequential_single_file_equals_reference_cli(tmp_path, kind, args):
    exp = json.load(open(os.path.join(LIST, "expected_%s_single.json" % kind)))
    (tmp_path / "all.fna").write_bytes(listeria())
    out = run_tool(["c"] + args + ["-i", "all.fna", "lm"], str(tmp_path)).stdout
    assert "single-file elements: 1" in out
    for name, e in exp["streams"].items():
        b = (tmp_path / ("lm." + name)).read_bytes()
        assert len(b) == e["bytes"], (name, len(b), e["bytes"])
        assert hashlib.md5(b).hexdigest() == e["md5"], name
    assert (tmp_path / "lm.refExtSize").read_bytes() == b""       # (a single-file archive has no lazy decompression support)
    assert list(struct.unpack("<1I", (tmp_path / "lm.seqCounts").read_bytes())) == exp["sequence_counts"]


def collection(kind):
    if kind == "long":                                             # 1.5 % divergence, contigs of 1.5 Mbp and a few short ones
        base = synth.base_codes(1_500_000, 81)
        contigs = []
        for i in range(9):
            g = synth.genome(base, i, 0.015)
            contigs += [g] if i % 3 else [g[:40_000], g[40_000:100_000], g[100_000:]]
        return sfa.multi_fasta(contigs)
    base = synth.base_codes(600_000, 82)                           # 420 contigs of about 30 kb
    contigs = []
    for i in range(21):
        g = synth.genome(base, i, 0.01)
        cuts = [0] + [30_000 * k + (17 * k * (i + 1)) % 900 for k in range(1, 20)] + [g.size]
        contigs += [g[a:b] for a, b in zip(cuts, cuts[1:])]
    return sfa.multi_fasta(contigs)


def oracle_rounds(data, r):
    elems = sfa.elements(data)
    g0 = sfa.parsed(elems[0])[0]
    targets = [sfa.parsed(e)[0] for e in elems[1:]]
    estimate = 1 + (len(data) - len(elems[0]) + sfa.MIN_BASIC_BLOCK_SIZE - 1) // sfa.MIN_BASIC_BLOCK_SIZE     # MGMP.cpp:113-115
    lim, _ = _driver.ref_length_limit(estimate, sum(c.size for c in g0))
    o = _orc.OracleMatcher(lim)
    res = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o, _orc.emit_params(1, lazyDecompressionSupport=0)), g0, targets, r, lazy=False)
    o.close()
    want = dict(res["streams"], locksPos=res["locks"], refExtSize=res["refExtSize"])
    want["literals"] = b"".join(c.tobytes() + b"\xa2" for c in g0) + want["literals"]
    return want, [len(t) for t in targets]


@pytest.mark.parametrize("kind,r", [("long", 2), ("long", 5), ("short", 2), ("short", 5), ("gz", 2), ("gz", 5)])
def test_rounds_equal_oracle_driver_on_the_restatements_elements(tmp_path, kind, r):
    data = collection("short" if kind == "gz" else kind)
    assert len(data) >= 12 * MIB
    name = "all.fa.gz" if kind == "gz" else "all.fa"
    (tmp_path / name).write_bytes(gzip.compress(data, 1) if kind == "gz" else data)
    out = run_tool(["c", "-R", str(r), "-i", name, "out"], str(tmp_path))
    want, counts = oracle_rounds(data, r)
    assert len(counts) >= 4
    got = streams_of(tmp_path, "out")
    for k in STREAMS:
        assert got[k] == want[k], k
    raw = (tmp_path / "out.seqCounts").read_bytes()
    assert list(struct.unpack("<%dI" % (len(raw) // 4), raw)) == counts
    assert ("single-file elements: %d" % (len(counts) + 1)) in out.stdout
    assert "Switching to sequential" not in out.stderr


def test_the_automatic_round_size_is_the_size_it_prints(tmp_path):
    """without -R the rounds are sized by the sliding window (windowRoundSize with its guess for an element's bytes): the run
    must write what `-R <the size it printed>` writes, and that is the oracle-driven loop's result"""
    import re
    data = collection("long")
    (tmp_path / "all.fa").write_bytes(data)
    out = run_tool(["c", "-i", "all.fa", "auto"], str(tmp_path)).stdout
    m = re.search(r"rounds of (\d+) targets", out)
    assert m and int(m.group(1)) >= 1, out
    r = int(m.group(1))
    run_tool(["c", "-R", str(r), "-i", "all.fa", "fixed"], str(tmp_path))
    assert digest(tmp_path, "auto") == digest(tmp_path, "fixed")
    want, _ = oracle_rounds(data, r)
    got = streams_of(tmp_path, "auto")
    for k in STREAMS:
        assert got[k] == want[k], k


def test_a_small_file_falls_back_to_the_sequential_schedule(tmp_path):
    base = synth.base_codes(520_000, 83)
    contigs = [synth.genome(base, i, 0.015) for i in range(10)]
    data = sfa.multi_fasta(contigs)
    assert 5 * MIB <= len(data) < 6 * MIB
    (tmp_path / "all.fa").write_bytes(data)
    out = run_tool(["c", "-i", "all.fa", "out"], str(tmp_path))
    assert "Switching to sequential matching mode (input file too small)." in out.stderr
    assert "single-file elements: 1" in out.stdout
    estimate = 1 + (len(data) - sfa.MIN_BASIC_BLOCK_SIZE + sfa.MIN_BASIC_BLOCK_SIZE - 1) // sfa.MIN_BASIC_BLOCK_SIZE   # MGMP.cpp:113-115
    lim, _ = _driver.ref_length_limit(estimate, contigs[0].size)
    o = _orc.OracleMatcher(lim)
    oe = _orc.OracleEmitter(o, _orc.emit_params(1, lazyDecompressionSupport=0))
    res = _driver.encode_sequential(o, oe, [contigs], lazy=False)
    want = dict(oe.streams(), locksPos=res["locks"], refExtSize=res["refExtSize"])
    want["literals"] = contigs[0].tobytes() + b"\xa2" + want["literals"]
    got = streams_of(tmp_path, "out")
    for k in STREAMS:
        assert got[k] == want[k], k
    assert (tmp_path / "out.seqCounts").read_bytes() == struct.pack("<I", 10)
    o.close()


def test_single_file_with_several_gpus_is_refused(tmp_path):
    (tmp_path / "all.fa").write_bytes(b">a\nACGT\n")
    r = subprocess.run([TOOL, "c", "--gpus", "2", "-i", "all.fa", "out"], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-i (single fasta file mode) runs on one GPU" in r.stderr, r.stderr


def digest(tmp_path, prefix):
    h = hashlib.md5()
    for k in STREAMS + ("seqCounts",):
        h.update((tmp_path / (prefix + "." + k)).read_bytes())
    return h.hexdigest()


def test_repeated_single_file_runs_write_the_same_bytes(tmp_path):
    (tmp_path / "all.fa").write_bytes(collection("short"))
    digests = set()
    for _ in range(3):
        run_tool(["c", "-R", "3", "-i", "all.fa", "o"], str(tmp_path))
        digests.add(digest(tmp_path, "o"))
    assert len(digests) == 1


@pytest.mark.parametrize("args", [["-R", "3"], ["-t1"]])
@pytest.mark.parametrize("kind", ["long", "short"])
def test_a_small_window_writes_the_bytes_of_the_default_window(tmp_path, kind, args):
    """--window-kib 256: elements span several windows, and the 1.5 Mbp contigs of `long` are longer than one"""
    (tmp_path / "all.fa").write_bytes(collection(kind))
    run_tool(["c"] + args + ["-i", "all.fa", "d"], str(tmp_path))
    for kib in ("256", "1000"):
        run_tool(["c"] + args + ["--window-kib", kib, "-i", "all.fa", "w"], str(tmp_path))
        assert digest(tmp_path, "w") == digest(tmp_path, "d"), kib
        for k in STREAMS:
            assert (tmp_path / ("w." + k)).read_bytes() == (tmp_path / ("d." + k)).read_bytes(), k
