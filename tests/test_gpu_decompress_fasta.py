"""`mbgc-hip c`, then `mbgc-hip d --fasta <dir>` in a fresh process: the input FASTA files must come back byte for byte (under
-U: the restatement over the upper-cased records), the same from default `d`, `--serial` and `--no-index`; stream sets without
the three side files still decode without --fasta; damaged side files and clashing names are refused with nothing written."""
import gzip
import os
import shutil

import numpy as np
import pytest

import _fasta
from _fastaout import format_fasta
from mbgc_amd import synth
from test_gpu_decompress import cut, tool, write_collection

pytestmark = pytest.mark.gpu
SIDE = ("names", "headers", "dnaLineLengths")


def files_of(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


def decode_three_ways(tmp, prefix="out"):
    a = None
    for name, extra in (("f0", []), ("f1", ["--serial"]), ("f2", ["--no-index"])):
        tool(["d"] + extra + ["--fasta", name, prefix, name + "x"], tmp)
        got = files_of(os.path.join(tmp, name))
        if a is None:
            a = got
        assert got == a, name
    return a


CASES = [(["-R", "3"], 7), (["-t1"], 5), (["-m", "2", "-R", "3"], 7), (["-L", "-R", "3"], 7), (["-U", "-R", "4"], 9)]


@pytest.mark.parametrize("args,n", CASES, ids=[" ".join(a) for a, _ in CASES])
def test_files_come_back(tmp_path, args, n):
    tmp = str(tmp_path)
    paths = write_collection(tmp, n, 100_000 + 2000 * n)
    tool(["c"] + args + ["list.txt", "out"], tmp)
    got = decode_three_ways(tmp)
    assert sorted(got) == sorted(os.path.basename(p) for p in paths)
    for p in paths:
        data = open(p, "rb").read()
        if "-U" in args:
            o = _fasta.oracle_parse(data, True)
            data = format_fasta(o["records"], o["dna_line_len"])
        assert got[os.path.basename(p)] == data, p
    assert os.path.exists(os.path.join(tmp, "f0x.seq"))                            # the .seq outputs are written as before


def test_reference_buffer_wraps(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 9, 120_000)
    with open(paths[1], "ab") as f:
        f.write(synth.fasta_bytes(synth.genome(synth.base_codes(2_400_000, 77), 1, 0.3), 901))
    for i in range(80):
        p = os.path.join(tmp, "u%02d.fa" % i)
        with open(p, "wb") as f:
            f.write(synth.fasta_bytes(synth.genome(synth.base_codes(60_000, 1000 + i), 0, 0.0), 2000 + i))
        paths.append(p)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "--ref-factor", "1", "-R", "2", "list.txt", "out"], tmp)
    tool(["d", "--fasta", "deep/er/back", "out", "b"], tmp)                        # (directories above it are made too)
    got = files_of(os.path.join(tmp, "deep", "er", "back"))
    assert len(got) == len(paths)
    for p in paths:
        assert got[os.path.basename(p)] == open(p, "rb").read(), p


@pytest.mark.parametrize("args", [[], ["-t1"]], ids=["rounds", "t1"])
def test_single_fasta_input(tmp_path, args):
    tmp = str(tmp_path)
    base = synth.base_codes(110_000, 5)
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        for i in range(100 if not args else 9):
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                f.write(synth.fasta_bytes(c, i * 10 + j))
    tool(["c", "-i", "all.fa"] + args + ["out"], tmp)
    got = decode_three_ways(tmp)
    assert list(got) == ["all.fa"]
    assert got["all.fa"] == open(os.path.join(tmp, "all.fa"), "rb").read()


def test_crlf_gzip_other_width_and_missing_last_newline(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 7, 100_000)
    g = [synth.genome(synth.base_codes(100_000, 55), i, 0.015) for i in range(7)]
    expect = {os.path.basename(p): open(p, "rb").read() for p in paths}
    crlf = synth.fasta_bytes(g[2], 20, 59).replace(b"\n", b"\r\n") + synth.fasta_bytes(g[2][:7001], 21, 59).replace(b"\n", b"\r\n")
    open(paths[2], "wb").write(crlf)
    expect["g02.fa"] = crlf
    plain = synth.fasta_bytes(g[3], 30) + synth.fasta_bytes(g[3][500:9000], 31)
    with gzip.open(paths[3] + ".gz", "wb") as f:
        f.write(plain)
    os.remove(paths[3])
    paths[3] += ".gz"
    expect["g03.fa"] = plain                                                       # comes back inflated, without .gz
    w60 = synth.fasta_bytes(g[4], 40, 60) + synth.fasta_bytes(g[4][:60 * 7], 41, 60)   # 60 columns among 80; a record of whole lines
    open(paths[4], "wb").write(w60)
    expect["g04.fa"] = w60
    cutoff = open(paths[5], "rb").read()
    assert cutoff.endswith(b"\n") and not cutoff.endswith(b"\n\n")
    open(paths[5], "wb").write(cutoff[:-1])                                        # no trailing newline: the last line is ended, as the reference does
    o = _fasta.oracle_parse(cutoff[:-1])
    expect["g05.fa"] = format_fasta(o["records"], o["dna_line_len"])
    assert expect["g05.fa"] == cutoff
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    for args in (["-R", "3"], ["-t1"]):
        tool(["c"] + args + ["list.txt", "out"], tmp)
        back = "back" + args[0]
        tool(["d", "--fasta", back, "out", "b"], tmp)
        got = files_of(os.path.join(tmp, back))
        assert sorted(got) == sorted(expect)
        for name in expect:
            assert got[name] == expect[name], (args, name)


# ---- the side files: not needed without --fasta, checked with it
@pytest.fixture(scope="module")
def small_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fa"))
    write_collection(tmp, 6, 100_000)
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    for ext in SIDE:
        assert os.path.getsize(os.path.join(tmp, "out." + ext)) > 0
    return tmp


def copy_run(src, dst, change):
    for f in os.listdir(src):
        if f.startswith("out."):
            data = change(f[4:], open(os.path.join(src, f), "rb").read())
            if data is not None:
                with open(os.path.join(dst, f), "wb") as o:
                    o.write(data)


def refused(tmp):
    r = tool(["d", "--fasta", "dir", "out", "back"], tmp, ok=False)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "mbgc-hip d: " in r.stderr
    assert not os.path.exists(os.path.join(tmp, "back.seq"))
    assert not os.path.exists(os.path.join(tmp, "dir")) or not os.listdir(os.path.join(tmp, "dir"))
    return r.stderr


def test_side_file_layout(small_run):
    names = open(os.path.join(small_run, "out.names"), "rb").read().split(b"\n")
    assert names[-1] == b"" and [os.path.basename(n.decode()) for n in names[:-1]] == ["g%02d.fa" % i for i in range(6)]
    heads, n = open(os.path.join(small_run, "out.headers"), "rb").read(), 0
    want = b""
    for i in range(6):
        for h, _ in _fasta.oracle_parse(open(os.path.join(small_run, "g%02d.fa" % i), "rb").read())["records"]:
            want += h + b"\n"
            n += 1
    assert heads == want
    assert np.fromfile(os.path.join(small_run, "out.dnaLineLengths"), dtype="<u8").tolist() == [80] * 6


def test_without_fasta_the_side_files_are_not_needed(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: None if name in SIDE else d)
    tool(["d", "out", "plain"], str(tmp_path))
    assert os.path.getsize(os.path.join(str(tmp_path), "plain.seq")) > 500_000


def test_missing_headers_is_refused(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: None if name == "headers" else d)
    err = refused(str(tmp_path))
    assert "malformed" in err and ".headers" in err


def test_header_line_removed_is_refused(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: d[d.index(b"\n") + 1:] if name == "headers" else d)
    assert "malformed" in refused(str(tmp_path))


def test_line_lengths_one_short_is_refused(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: d[:-8] if name == "dnaLineLengths" else d)
    assert "malformed" in refused(str(tmp_path))


def test_name_missing_is_refused(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: d[d.index(b"\n") + 1:] if name == "names" else d)
    assert "malformed" in refused(str(tmp_path))


def test_two_units_with_one_basename_are_refused(tmp_path):
    tmp = str(tmp_path)
    paths = write_collection(tmp, 5, 100_000)
    os.mkdir(os.path.join(tmp, "other"))
    twin = os.path.join(tmp, "other", os.path.basename(paths[2]))
    shutil.copy(paths[4], twin)
    paths[4] = twin
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c", "-R", "2", "list.txt", "out"], tmp)
    err = refused(tmp)
    assert "same file" in err and "g02.fa" in err


def test_m3_is_refused_with_fasta_too(tmp_path):
    tmp = str(tmp_path)
    write_collection(tmp, 5, 100_000)
    tool(["c", "-m", "3", "list.txt", "out"], tmp)
    err = refused(tmp)
    assert "-m 3" in err and "rcMapOff" in err
