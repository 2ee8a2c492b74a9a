"""Single fasta file mode (`mbgc c -i <fastaFile>`): the split rule, pinned on the reference CLI.

tests/_singlefasta.py restates mgmpInSplit_next. Here the reference's developer build compresses a multi-FASTA file in its
parallel schedule and dumps its streams (`v -D`): the sequence-counts stream (one u32 per element) and the DNA line
lengths (one u64 per element) depend on where the file was cut and on nothing the threads' timing decides. They must
be what the restatement's elements give. The sequential encoding of the concatenated Listeria genomes is deterministic as a
whole and is pinned as a fixture (tests/golden/make_single_fasta_golden.py)."""
import importlib.util
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import _singlefasta as sfa
from mbgc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = os.path.join(ROOT, "oracle", "_ref", "mbgc-dev")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_single_fasta_golden", os.path.join(ROOT, "tests", "golden", "make_single_fasta_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def short_contigs(seed, total, mean):
    rng = np.random.default_rng(seed)
    base = synth.base_codes(total, seed)
    g, out, at = synth.genome(base, 0, 0.0), [], 0
    while at < total:
        n = int(rng.integers(mean // 2, mean * 3 // 2))
        out.append(g[at:at + n])
        at += n
    return out


def gt_in_header_at_threshold():
    """a header line that starts before the threshold of element 1 (its start + 2 MiB) and holds a '>' behind it: the reference
    cuts there, in the middle of the line"""
    contigs = short_contigs(5, 10_500_000, 30_000)
    data = sfa.multi_fasta(contigs)
    e0 = sfa.split_window(data)[0]
    thr = e0 + sfa.MIN_BASIC_BLOCK_SIZE
    h = data.rindex(b"\n>", 0, thr) + 1                            # the last header line that starts before the threshold
    body = data.index(b"\n", h)
    assert body < thr                                             # (it ends before it, too: the line is rewritten to reach across)
    # the record's lines stay as they are; its header grows until a '>' in it stands just behind the threshold
    name = b">odd" + b"_" * (thr - h - 3) + b"-> with a mark"
    data = data[:h] + name + data[body:]
    ends = sfa.split_window(data)
    assert ends[0] == e0 and ends[1] == h + len(name) - len(b"> with a mark") and ends[1] == thr + 2 and data[ends[1] - 1] != 10
    return data


def cases():
    yield "listeria", lambda: _golden_script().concatenated()
    yield "short_contigs", lambda: sfa.multi_fasta(short_contigs(3, 12_000_000, 5_000))
    yield "gt_in_header", gt_in_header_at_threshold
    # the last element shorter than 2 MiB: contigs of 0.7 Mbp, 13 of them — 64 KiB+ for G0, four targets of three contigs, a rest of one
    yield "short_last", lambda: sfa.multi_fasta(short_contigs(7, 9_300_000, 700_000))


@pytest.mark.parametrize("name,make", list(cases()), ids=[c[0] for c in cases()])
def test_reference_cuts_where_the_restatement_cuts(tmp_path, name, make):
    if not os.path.exists(DEV):
        pytest.skip("oracle/_ref not built")
    data = make()
    path = tmp_path / "all.fa"
    path.write_bytes(data)
    r = subprocess.run([DEV, "c", "-i", str(path), str(tmp_path / "a.mbgc")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Switching to sequential" not in r.stderr, r.stderr[-2000:]
    subprocess.run([DEV, "v", "-D", str(tmp_path / "a.mbgc")], check=True, capture_output=True, cwd=str(tmp_path), timeout=600)
    # (the dumps are numbered as the coders meet them; the collective section starts with names, sequence counts, header templates,
    # headers, line lengths — MBGC_Decoder.cpp:1085-1090 — and the names stream of a single-file archive is the file's name)
    dumps = [(tmp_path / ("a.mbgc_dump_%02d" % i)) for i in range(1, 30)]
    names = [i for i, p in enumerate(dumps) if p.exists() and p.read_bytes() == b"all.fa\xbb"]
    assert len(names) == 1
    counts = dumps[names[0] + 1].read_bytes()
    lines = dumps[names[0] + 4].read_bytes()
    counts = list(struct.unpack("<%dI" % (len(counts) // 4), counts))
    lines = list(struct.unpack("<%dQ" % (len(lines) // 8), lines))
    elems = sfa.elements(data)
    assert len(elems) >= 5                                         # G0 and at least SINGLEFILE_PARALLEL_MIN_TARGETS targets
    if name == "short_last":
        assert len(elems[-1]) < sfa.MIN_BASIC_BLOCK_SIZE
    mine = [sfa.parsed(e) for e in elems]
    assert counts == [len(c) for c, _ in mine]
    assert lines == [ll for _, ll in mine]


def test_restatement_known_answers():
    s = sfa.split_window
    d = b">a\nAC\n>b\nGT\n>c\nAA\n"
    assert s(d, True, 1, 1) == [6, 12, 18]
    assert s(d, True, 6, 1) == [6, 12, 18]                         # a '>' exactly at the threshold
    assert s(d, True, 7, 1) == [12, 18]                            # one byte behind it: the next one
    assert s(d, True, 13, 100) == [18]                             # none behind the threshold: the end of the file
    assert s(d, False, 13, 100) == []                              # ... which a window does not know
    assert s(d, False, 1, 4) == [6, 12]                            # the last element's end is not decided inside the window
    assert s(b">x > y\nAC\n", True, 1, 1) == [3, 10]               # any '>' counts
    assert s(d, True, 18, 1) == [18] and s(d, True, 1, 1, max_elems=2) == [6, 12]
    assert s(b"", True, 1, 1) == []


@pytest.mark.parametrize("kind", ["t1", "m3"])
def test_sequential_single_file_fixture_is_the_reference_cli(tmp_path, kind):
    exp = json.load(open(os.path.join(LIST, "expected_%s_single.json" % kind)))
    assert exp["sequence_counts"] == [62] and exp["input_bytes"] == 9178158
    if not os.path.exists(DEV):
        pytest.skip("oracle/_ref not built")
    got = _golden_script().reference_streams(kind, str(tmp_path))
    assert got["streams"] == exp["streams"]
