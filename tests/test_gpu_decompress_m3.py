"""`mbgc-hip c -m 3`, then `mbgc-hip d --restore-rc` in a fresh process: the reverse-complement pass over the literals is inverted on
the device and the collection comes back — the same bytes from default `d`, `--serial` and `--no-index`, the FASTA files with
`--fasta`; on streams without the pass the switch changes nothing; damaged maps end with a message and exit 1, and so do three
mutants of a run's own maps that the referee of tests/_rcrestore.py refuses, while three it accepts give the collection back."""
import json
import lzma
import os

import numpy as np
import pytest

import _rcdata
import _rcmut
import _rcrestore
from mbgc_amd import synth
from test_gpu_decompress import LIST, OUTS, check_outputs, copy_run, cut, expected, tool, write_collection
from test_gpu_decompress_fasta import files_of

pytestmark = pytest.mark.gpu
MARK = bytes([0xA4])


def read(tmp, name):
    return open(os.path.join(tmp, name), "rb").read()


def write_m3_collection(tmp):
    """write_collection(tmp, 5, 100_000) with the first record of file 0 — under -m 3 the initial reference, which goes to the
    literals raw — extended by the reverse complement of 5000 of its own bases: something for the pass to cut"""
    paths = write_collection(tmp, 5, 100_000)
    g0 = synth.genome(synth.base_codes(100_000, 55), 0, 0.015)
    with open(paths[0], "wb") as f:
        f.write(synth.fasta_bytes(np.concatenate([g0, _rcdata.revcomp(g0[1000:6000])]), 0))
    return paths


def the_pass_cut_something(tmp, prefix="out"):
    assert os.path.getsize(os.path.join(tmp, prefix + ".rcMapOff")) > 0
    assert MARK in read(tmp, prefix + ".literals")


def decode_three_ways(tmp, prefix):
    for name, extra in (("d0", []), ("d1", ["--serial"]), ("d2", ["--no-index"])):
        tool(["d", "--restore-rc"] + extra + [prefix, name], tmp)
    for ext in OUTS:
        a = read(tmp, "d0." + ext)
        for other in ("d1", "d2"):
            assert read(tmp, other + "." + ext) == a, (other, ext)


@pytest.fixture(scope="module")
def m3_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("m3"))
    paths = write_m3_collection(tmp)
    tool(["c", "-m", "3", "list.txt", "out"], tmp)
    the_pass_cut_something(tmp)
    return tmp, paths


def test_collection_comes_back(m3_run):
    tmp, paths = m3_run
    decode_three_ways(tmp, "out")
    check_outputs(tmp, "d0", expected(paths, False))


def test_refusal_without_the_switch_names_it(m3_run):
    tmp, _ = m3_run
    r = tool(["d", "out", "plain"], tmp, ok=False)
    assert r.returncode == 1 and "-m 3" in r.stderr and "rcMapOff" in r.stderr and "--restore-rc" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "plain.seq"))


def test_single_fasta_input(tmp_path):
    tmp = str(tmp_path)
    base = synth.base_codes(110_000, 5)
    recs = []
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        for i in range(9):
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                if i == 0 and j == 0:
                    c = np.concatenate([c, _rcdata.revcomp(c[1000:6000])])
                f.write(synth.fasta_bytes(c, i * 10 + j))
                recs.append(c.tobytes())
    tool(["c", "-m", "3", "-i", "all.fa", "out"], tmp)
    the_pass_cut_something(tmp)
    decode_three_ways(tmp, "out")
    lens = np.fromfile(os.path.join(tmp, "d0.contigLens"), dtype="<u8")
    assert lens.tolist() == [len(r) for r in recs] and read(tmp, "d0.seq") == b"".join(recs)
    assert int(np.fromfile(os.path.join(tmp, "d0.seqCounts"), dtype="<u4").sum()) == len(recs)


def test_fasta_files_come_back(m3_run):
    tmp, paths = m3_run
    tool(["d", "--restore-rc", "--fasta", "fa", "out", "fx"], tmp)
    got = files_of(os.path.join(tmp, "fa"))
    assert sorted(got) == sorted(os.path.basename(p) for p in paths)
    for p in paths:
        assert got[os.path.basename(p)] == read(tmp, p), p                       # (every input file ends with a newline)


def test_listeria(tmp_path):
    tmp = str(tmp_path)
    exp = json.load(open(os.path.join(LIST, "expected_t1.json")))
    paths = []
    for f in exp["files"]:
        p = os.path.join(tmp, f)
        with open(p, "wb") as o:
            o.write(lzma.open(os.path.join(LIST, f + ".xz")).read())
        paths.append(p)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "-m", "3", "-t1", "list.txt", "lm"], tmp)
    tool(["d", "--restore-rc", "lm", "d0"], tmp)
    check_outputs(tmp, "d0", expected(paths, False))


def test_the_switch_changes_nothing_on_other_streams(tmp_path):
    tmp = str(tmp_path)
    write_collection(tmp, 6, 100_000)
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    tool(["d", "out", "a"], tmp)
    tool(["d", "--restore-rc", "out", "b"], tmp)
    for ext in OUTS:
        assert read(tmp, "a." + ext) == read(tmp, "b." + ext), ext


def refused(tmp):
    r = tool(["d", "--restore-rc", "out", "back"], tmp, ok=False)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "mbgc-hip d: " in r.stderr and ("malformed" in r.stderr or "cannot open" in r.stderr), r.stderr
    assert not os.path.exists(os.path.join(tmp, "back.seq"))
    return r.stderr


def test_truncated_rcmaplen_is_refused(m3_run, tmp_path):
    copy_run(m3_run[0], str(tmp_path), lambda name, d: d[:-1] if name == "rcMapLen" else d)
    assert "malformed" in refused(str(tmp_path))


def test_missing_rcmapoff_is_refused(m3_run, tmp_path):
    copy_run(m3_run[0], str(tmp_path), lambda name, d: d)
    os.remove(os.path.join(str(tmp_path), "out.rcMapOff"))
    assert "cannot open" in refused(str(tmp_path))


def test_longer_rcmapoff_is_refused(m3_run, tmp_path):
    copy_run(m3_run[0], str(tmp_path), lambda name, d: d + b"\x00\x00\x00\x00" if name == "rcMapOff" else d)
    assert "malformed" in refused(str(tmp_path))


def test_bench_line(m3_run):
    tmp, _ = m3_run
    out = tool(["d", "--restore-rc", "--bench", "out", "bench"], tmp).stdout
    line = json.loads(next(l for l in out.splitlines() if l.startswith("{")))
    assert line["rc_restore_ms"] > 0 and line["rc_marks"] == read(tmp, "out.literals").count(MARK) and line["rc_max_chain"] >= 1
    assert line["value"] > 0


@pytest.fixture(scope="module")
def m3_t1_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("m3t1"))
    paths = write_m3_collection(tmp)
    tool(["c", "-m", "3", "-t1", "list.txt", "out"], tmp)
    the_pass_cut_something(tmp)
    return tmp, paths


def own_map_mutants(tmp):
    """mutants of the run's own rcMapOff / rcMapLen (other literals would invalidate the streams that count them), labelled by the
    referee -> ({name: (rcMapOff, rcMapLen)} accepted: the same restored literals from other bytes; {name: (rcMapOff, rcMapLen,
    the plan's words)} refused)"""
    cut, off, ln = read(tmp, "out.literals"), read(tmp, "out.rcMapOff"), read(tmp, "out.rcMapLen")
    want = _rcrestore.restore_bounded(cut, off, ln, 4)
    vals = _rcrestore.values_of(ln)
    min_len, deltas = vals[0][0], [v for v, _ in vals[1:]]
    put = _rcrestore.put_byte_frugal
    assert not isinstance(want, str) and want[1] == len(deltas) >= 1 and min_len >= 1
    d0 = cut.index(MARK)                                                         # where match 0 starts, in restored coordinates
    accepted = {
        "every value in 3 bytes": (off, b"".join(_rcmut.padded(v, 3) for v, _ in vals)),
        "a minimal length of 1 less under differences of 1 more": (off, put(min_len - 1) + b"".join(put(v + 1) for v in deltas)),
        "the minimal length in 10 bytes": (off, _rcmut.padded(min_len, 10) + ln[vals[0][1]:]),
    }
    refused = {
        "a source one byte into its match": ((d0 - (min_len + deltas[0]) + 1).to_bytes(4, "little") + off[4:], ln, "the source of match 0 does not end before the match starts"),
        "a length of 2^63": (off, put(min_len) + put(2 ** 63) + ln[vals[0][1] + vals[1][1]:], "the lengths add up beyond 64 bits"),
        "one value too few": (off, ln[:-vals[-1][1]], "%d values for the minimal length and %d marks" % (len(deltas), len(deltas))),
    }
    for name, (o, l) in accepted.items():
        assert (o, l) != (off, ln) and _rcrestore.restore_bounded(cut, o, l, 4)[:4] == want[:4], name   # (all but the minimal length)
    for name, (o, l, _) in refused.items():
        assert isinstance(_rcrestore.restore_bounded(cut, o, l, 4), str), name
    return accepted, refused


def test_mutants_of_the_runs_own_maps(m3_t1_run, tmp_path):
    src, paths = m3_t1_run
    accepted, refused_ones = own_map_mutants(src)
    for k, (name, (off, ln)) in enumerate(sorted(accepted.items())):
        tmp = str(tmp_path / ("a%d" % k))
        os.mkdir(tmp)
        copy_run(src, tmp, lambda f, d: off if f == "rcMapOff" else ln if f == "rcMapLen" else d)
        tool(["d", "--restore-rc", "out", "back"], tmp)
        check_outputs(tmp, "back", expected(paths, False))
    for k, (name, (off, ln, words)) in enumerate(sorted(refused_ones.items())):
        tmp = str(tmp_path / ("r%d" % k))
        os.mkdir(tmp)
        copy_run(src, tmp, lambda f, d: off if f == "rcMapOff" else ln if f == "rcMapLen" else d)
        err = refused(tmp)
        assert "malformed" in err and words in err, (name, err)
