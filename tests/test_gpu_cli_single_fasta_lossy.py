"""`mbgc-hip c --lossy-file <fastaFile>` (the reference's `mbgc c -L -i <fastaFile>`; `--lossy -i` stays refused, as
tests/test_gpu_fasta_lossy.py holds it) on the GPU, against the restatement tests/_singlefasta_lossy.py (held
to the reference CLI by tests/test_single_fasta_lossy_rule.py): the rounds against the oracle-driven reference loop over the
restatement's elements, the per-element line lengths, the sequential schedule against the tool's own lossless run on the
normalised copy and against the reference CLI's recorded digests, the window protocol, the fallback, the FASTQ refusal and the
way back through `d --fasta` and `v`."""
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
import _singlefasta_lossy as sfl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
STREAMS = ("literals", "mapOff", "mapOff5th", "mapLen", "gapDelta", "flags", "locksPos", "refExtSize")
MIB = 1 << 20


def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def outputs(tmp, prefix):
    return {f[len(prefix) + 1:]: open(os.path.join(tmp, f), "rb").read() for f in sorted(os.listdir(tmp)) if f.startswith(prefix + ".")}


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """a damaged file of 8.8 MB: junk in front, CRLF parts, ragged widths, empty and CR-only lines, '>' and '@' inside header lines,
    '@' headers — G0 and four targets; parsed once"""
    tmp = str(tmp_path_factory.mktemp("lossy_single"))
    data = sfl.synth_single(8_600_000, 8, 5)
    assert 7 * MIB <= len(data) <= 9 * MIB
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        f.write(data)
    return tmp, data, sfl.rounds(data)


def oracle_rounds(data, parsed, r):
    contigs = lambda p: [np.frombuffer(s, dtype=np.uint8) for _, s in p["records"]]
    g0, targets = contigs(parsed[0]), [contigs(p) for p in parsed[1:]]
    estimate = 1 + (len(data) - len(sfa.elements(data)[0]) + sfa.MIN_BASIC_BLOCK_SIZE - 1) // sfa.MIN_BASIC_BLOCK_SIZE       # MGMP.cpp:113-115
    lim, _ = _driver.ref_length_limit(estimate, sum(c.size for c in g0))
    o = _orc.OracleMatcher(lim)
    res = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o, _orc.emit_params(1, lazyDecompressionSupport=0)), g0, targets, r, lazy=False)
    o.close()
    want = dict(res["streams"], locksPos=res["locks"], refExtSize=res["refExtSize"])
    want["literals"] = b"".join(c.tobytes() + b"\xa2" for c in g0) + want["literals"]
    return want, [len(t) for t in targets]


@pytest.mark.parametrize("r", [2, 5])
def test_rounds_equal_oracle_driver_on_the_restatements_elements(big, r):
    tmp, data, parsed = big
    out = tool(["c", "-R", str(r), "--lossy-file", "all.fa", "r%d" % r], tmp)
    want, counts = oracle_rounds(data, parsed, r)
    assert len(counts) >= 4
    got = outputs(tmp, "r%d" % r)
    for k in STREAMS:
        assert got[k] == want[k], k
    assert list(struct.unpack("<%dI" % (len(got["seqCounts"]) // 4), got["seqCounts"])) == counts
    assert ("single-file elements: %d" % (len(counts) + 1)) in out.stdout and "Switching to sequential" not in out.stderr
    # .dnaLineLengths is per element: every element's own longest line, not the file's
    lines = [p["dna_line_len"] for p in parsed]
    assert np.frombuffer(got["dnaLineLengths"], dtype="<u8").tolist() == lines
    assert sum(x != sfl.sequential(data)["dna_line_len"] for x in lines) >= 2


def test_round_trip_of_the_rounds(big, tmp_path):
    tmp, data, parsed = big
    tool(["c", "-R", "3", "--lossy-file", "all.fa", "rt"], tmp)
    tool(["d", "--fasta", str(tmp_path / "back"), "rt", str(tmp_path / "b")], tmp)
    text = sfl.rounds_text(data)
    assert (tmp_path / "back" / "all.fa").read_bytes() == text
    r = tool(["v", "--flat", "--root", str(tmp_path / "back"), "rt"], tmp, ok=False)
    assert r.returncode == 0 and "correctly decoded 1 out of 1 files" in r.stdout, r.stdout + r.stderr
    (tmp_path / "back" / "all.fa").write_bytes(data)                                   # the damaged original is not what the set holds
    assert tool(["v", "--flat", "--root", str(tmp_path / "back"), "rt"], tmp, ok=False).returncode != 0


@pytest.mark.parametrize("args", [["-t1"], ["-m", "3", "-t1"]], ids=["t1", "m3"])
def test_sequential_equals_the_lossless_run_on_the_normalised_copy(big, tmp_path, args):
    """the file is ONE target read by one kseq_read_lossy: the same records, the file's longest line. The first record holds that
    line and is longer than it, so the lossless reader finds the same line length in the copy. (--ref-factor: the two files differ in
    size, and the size would size the reference buffer.)"""
    tmp, data, parsed = big
    norm = sfl.sequential_text(data)
    assert norm != data and len(norm) != len(data)
    os.mkdir(str(tmp_path / "n"))
    (tmp_path / "n" / "all.fa").write_bytes(norm)
    tool(["c"] + args + ["--ref-factor", "8", "--lossy-file", "all.fa", str(tmp_path / "lossy")], tmp)
    tool(["c"] + args + ["--ref-factor", "8", "-i", "all.fa", str(tmp_path / "norm")], str(tmp_path / "n"))
    a, b = outputs(str(tmp_path), "lossy"), outputs(str(tmp_path), "norm")
    assert sorted(a) == sorted(b) and len(a) >= 12
    for k in a:
        if k != "names":
            assert a[k] == b[k], k
    p = sfl.sequential(data)
    assert a["seqCounts"] == struct.pack("<I", len(p["records"]))
    assert np.frombuffer(a["dnaLineLengths"], dtype="<u8").tolist()[-1] == p["dna_line_len"] == 100
    if args == ["-t1"]:                                                                # the way back: the restatement's text
        tool(["d", "--fasta", str(tmp_path / "back"), str(tmp_path / "lossy"), str(tmp_path / "b")], tmp)
        assert (tmp_path / "back" / "all.fa").read_bytes() == norm
        r = tool(["v", "--flat", "--root", str(tmp_path / "back"), str(tmp_path / "lossy")], tmp, ok=False)
        assert r.returncode == 0, r.stdout + r.stderr


def test_golden_fixture(tmp_path):
    exp = json.load(open(os.path.join(LIST, "expected_lossy_single.json")))
    data = sfl.damaged_listeria([lzma.open(os.path.join(LIST, f + ".xz")).read() for f in exp["files"]])
    assert len(data) == exp["input_bytes"] and hashlib.md5(data).hexdigest() == exp["input_md5"]
    (tmp_path / "all.fna").write_bytes(data)
    out = tool(["c", "-t1", "--lossy-file", "all.fna", "lm"], str(tmp_path)).stdout
    assert "single-file elements: 1" in out
    for name, e in exp["streams"].items():
        b = (tmp_path / ("lm." + name)).read_bytes()
        assert len(b) == e["bytes"], (name, len(b), e["bytes"])
        assert hashlib.md5(b).hexdigest() == e["md5"], name
    assert list(struct.unpack("<1I", (tmp_path / "lm.seqCounts").read_bytes())) == exp["sequence_counts"]
    assert np.fromfile(str(tmp_path / "lm.dnaLineLengths"), dtype="<u8").tolist()[-1:] == exp["dna_line_lengths"]


@pytest.mark.parametrize("args", [["-R", "3"], ["-t1"]], ids=["R3", "t1"])
def test_a_small_window_writes_the_bytes_of_the_default_window(tmp_path, args):
    """--window-kib 256: '@'-headed records, records longer than a window (0.5 Mbp), more junk in front than a tile holds — the
    first window's first marker stands in its second tile; batches and elements span windows"""
    junk = b"# a comment of eighty bytes or so, repeated until it is longer than one tile\r\n" * 60 + b"\n  "
    assert len(junk) > 4096 and b">" not in junk and b"@" not in junk
    data = sfl.synth_single(8_200_000, 8, 9, junk)
    assert b"\n@" in data and max(len(s) for _, s in sfl.sequential(data)["records"]) > 256 * 1024
    (tmp_path / "all.fa").write_bytes(data)
    tool(["c"] + args + ["--lossy-file", "all.fa", "d"], str(tmp_path))
    want = outputs(str(tmp_path), "d")
    assert want["seqCounts"] and len(want["literals"]) > 100_000
    for kib in ("256", "1000"):
        tool(["c"] + args + ["--window-kib", kib, "--lossy-file", "all.fa", "w"], str(tmp_path))
        got = outputs(str(tmp_path), "w")
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == want[k], (kib, k)


def test_a_small_file_falls_back_to_the_sequential_schedule(tmp_path):
    data = sfl.synth_single(600_000, 6, 5)
    (tmp_path / "all.fa").write_bytes(data)
    out = tool(["c", "--lossy-file", "all.fa", "auto"], str(tmp_path))
    assert "Switching to sequential matching mode (input file too small)." in out.stderr and "single-file elements: 1" in out.stdout
    tool(["c", "-t1", "--lossy-file", "all.fa", "t1"], str(tmp_path))
    a, b = outputs(str(tmp_path), "auto"), outputs(str(tmp_path), "t1")
    assert sorted(a) == sorted(b) and len(a) >= 12
    for k in a:
        assert a[k] == b[k], k
    p = sfl.sequential(data)
    assert a["seqCounts"] == struct.pack("<I", len(p["records"])) and len(p["records"]) == 18
    tool(["d", "--fasta", "back", "auto", "b"], str(tmp_path))
    assert (tmp_path / "back" / "all.fa").read_bytes() == sfl.sequential_text(data)


@pytest.mark.parametrize("args", [["-R", "2"], ["-t1"]], ids=["R2", "t1"])
def test_fastq_is_refused(big, tmp_path, args):
    """a '+' where a sequence line could start, in a later element (a later batch): the list mode's message"""
    tmp, data, parsed = big
    at = data.index(b"\n", 5_000_000) + 1
    assert data[at] not in b">@\r\n" and at > sum(len(e) for e in sfa.elements(data)[:2])
    (tmp_path / "fq.fa").write_bytes(data[:at] + b"+\n" + data[at:])
    r = tool(["c"] + args + ["--lossy-file", "fq.fa", "o"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "FASTQ input is not supported" in r.stderr and "fq.fa" in r.stderr, r.stderr


def test_several_gpus_stay_refused(tmp_path):
    (tmp_path / "all.fa").write_bytes(b"junk>a\r\nACGT\r\n")
    r = tool(["c", "--gpus", "2", "--lossy-file", "all.fa", "out"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "-i (single fasta file mode) runs on one GPU" in r.stderr, r.stderr


def test_the_lists_option_with_a_single_file_names_the_option_to_give(tmp_path):
    (tmp_path / "all.fa").write_bytes(b"junk>a\r\nACGT\r\n")
    r = tool(["c", "--lossy", "-i", "all.fa", "out"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "--lossy-file" in r.stderr, r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("out.")]
