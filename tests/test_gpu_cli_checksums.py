"""`mbgc-hip c --checksums`, `d --check`, `mbgc-hip t` and `r --checksums` on the 7-file collection of write_collection. The oracle
of a manifest is Python: zlib.crc32 per slice of <out>.seq by <out>.contigLens of an unselected `mbgc-hip d` of the same streams,
and zlib.crc32 of the four side files. The oracle of a damaged set is `d` without --check on it and the same arithmetic."""
import os
import re
import shutil
import struct
import zlib

import numpy as np
import pytest

import _singlefasta as sfa
from mbgc_amd import synth
from test_gpu_decompress_select import Full, N, tool, write_collection

pytestmark = pytest.mark.gpu

STREAMS = {"m1R3": (["-m", "1", "-R", "3"], []), "m0t1": (["-m", "0", "-t1"], []), "m3t1": (["-m", "3", "-t1"], ["--restore-rc"])}
SIDE = ("meta", "names", "headers", "dnaLineLengths")


def read(tmp, name):
    with open(os.path.join(tmp, name), "rb") as f:
        return f.read()


def python_manifest(tmp, prefix, seq, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = b"MBGCCRC1" + struct.pack("<Q", len(lens))
    out += b"".join(struct.pack("<I", zlib.crc32(read(tmp, prefix + "." + e))) for e in SIDE)
    return out + b"".join(struct.pack("<I", zlib.crc32(seq[off[k]:off[k + 1]])) for k in range(len(lens)))


def decoded(tmp, streams, out, extra=()):
    tool(["d"] + list(extra) + [streams, out], tmp)
    return read(tmp, out + ".seq"), np.fromfile(os.path.join(tmp, out + ".contigLens"), dtype="<u8")


def copy_set(tmp, src, dst):
    for f in os.listdir(tmp):
        if f.startswith(src + "."):
            shutil.copy(os.path.join(tmp, f), os.path.join(tmp, dst + f[len(src):]))


def summary(stdout):
    m = re.search(r"^checksums: (\d+) of (\d+) contigs checked, (\d+) differ$", stdout, re.M)
    assert m, stdout
    return tuple(int(x) for x in m.groups())


def bad_contigs(stdout):
    return [int(x) for x in re.findall(r"^checksum ERROR: contig (\d+) \(", stdout, re.M)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    made = {}

    def get(mode):
        if mode not in made:
            tmp = str(tmp_path_factory.mktemp(mode))
            paths = write_collection(tmp, N, 100_000 + 2000 * N)
            plain = tool(["c"] + STREAMS[mode][0] + ["list.txt", "base"], tmp)
            with_option = tool(["c"] + STREAMS[mode][0] + ["--checksums", "list.txt", "out"], tmp)
            full = Full(tmp, paths, STREAMS[mode][1])
            full.plain_stdout, full.option_stdout = plain.stdout, with_option.stdout
            made[mode] = full
        return made[mode]
    return get


@pytest.mark.parametrize("mode", list(STREAMS))
def test_c_checksums_writes_the_manifest_and_changes_nothing_else(runs, mode):
    full = runs(mode)
    tmp = full.tmp
    base = sorted(f[5:] for f in os.listdir(tmp) if f.startswith("base."))
    out = sorted(f[4:] for f in os.listdir(tmp) if f.startswith("out."))
    assert out == sorted(base + ["checksums"])
    for ext in base:
        assert read(tmp, "out." + ext) == read(tmp, "base." + ext), ext
    assert full.option_stdout == full.plain_stdout                    # (the option adds no line of its own)
    assert read(tmp, "out.checksums") == python_manifest(tmp, "out", full.seq, full.lens)


@pytest.mark.parametrize("mode", list(STREAMS))
def test_t_and_d_check_on_an_intact_set(runs, mode):
    full = runs(mode)
    tmp, extra = full.tmp, STREAMS[mode][1]
    n = len(full.lens)
    work = os.path.join(tmp, "empty_" + mode)
    os.mkdir(work)
    r = tool(["t"] + extra + ["../out"], work)
    assert summary(r.stdout) == (n, n, 0) and "checksum ERROR" not in r.stdout
    assert os.listdir(work) == []                                     # t writes nothing
    r = tool(["d"] + extra + ["--check", "--fasta", "chk_fa", "out", "chk"], tmp)
    assert summary(r.stdout) == (n, n, 0)
    for ext in ("seq", "contigLens", "seqCounts"):
        assert read(tmp, "chk." + ext) == read(tmp, "full." + ext)
    for f in os.listdir(os.path.join(tmp, "full_fa")):
        assert read(tmp, "chk_fa/" + f) == read(tmp, "full_fa/" + f)
    assert sorted(os.listdir(os.path.join(tmp, "chk_fa"))) == sorted(os.listdir(os.path.join(tmp, "full_fa")))


def test_one_flipped_literal(runs):
    full = runs("m1R3")
    tmp = full.tmp
    copy_set(tmp, "out", "flip")
    lit = bytearray(read(tmp, "flip.literals"))
    at = next(i for i, b in enumerate(lit) if b in b"ACGT")
    lit[at] = b"ACGT"[(b"ACGT".index(lit[at]) + 1) % 4]
    with open(os.path.join(tmp, "flip.literals"), "wb") as f:
        f.write(lit)
    seq, lens = decoded(tmp, "flip", "flipback")
    want = python_manifest(tmp, "flip", seq, lens)
    have = read(tmp, "flip.checksums")
    n = len(lens)
    expected = [k for k in range(n) if want[32 + 4 * k:36 + 4 * k] != have[32 + 4 * k:36 + 4 * k]]
    assert expected and 0 in expected                                 # the flipped contig is G0's, and whoever copies that base follows
    r = tool(["t", "flip"], tmp, ok=False)
    assert r.returncode == 2, r.stderr
    assert summary(r.stdout) == (n, n, len(expected))
    assert bad_contigs(r.stdout) == expected


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_manifest_entry_changed(runs, where):
    full = runs("m1R3")
    tmp = full.tmp
    n = len(full.lens)
    j = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    copy_set(tmp, "out", "ent")
    m = bytearray(read(tmp, "ent.checksums"))
    m[32 + 4 * j] ^= 1
    with open(os.path.join(tmp, "ent.checksums"), "wb") as f:
        f.write(m)
    r = tool(["t", "ent"], tmp, ok=False)
    assert r.returncode == 2, r.stderr
    assert summary(r.stdout) == (n, n, 1) and bad_contigs(r.stdout) == [j]
    f = int(np.searchsorted(full.first, j, side="right") - 1)
    header = read(tmp, "out.headers").split(b"\n")[j].decode()[:60]
    got = zlib.crc32(full.seq[full.off[j]:full.off[j + 1]])
    line = "checksum ERROR: contig %d (file %s, record %d: %s) expected %08x got %08x" % (j, full.paths[f], j - int(full.first[f]), header, got ^ 1, got)
    assert line in r.stdout.splitlines(), r.stdout


def test_changed_headers(runs):
    full = runs("m1R3")
    tmp = full.tmp
    copy_set(tmp, "out", "hdr")
    h = bytearray(read(tmp, "hdr.headers"))
    h[3] = ord("X") if h[3] != ord("X") else ord("Y")
    with open(os.path.join(tmp, "hdr.headers"), "wb") as f:
        f.write(h)
    r = tool(["t", "hdr"], tmp, ok=False)
    assert r.returncode == 2, r.stderr
    assert "checksum ERROR: hdr.headers differs" in r.stdout.splitlines()
    assert summary(r.stdout)[2] == 0


def test_selection_decides_what_is_checked(runs):
    full = runs("m1R3")
    tmp = full.tmp
    n = len(full.lens)
    select = ["--select-seq", "1 99pct"]                              # records 11, 21, 31, 41, 61: five files
    r = tool(["t"] + select + ["out"], tmp)
    assert summary(r.stdout) == (5, n, 0)
    headers = read(tmp, "out.headers").split(b"\n")[:n]
    chosen = [k for k in range(n) if b"1 99pct" in headers[k]]
    assert len(chosen) == 5
    not_chosen = next(k for k in range(1, n) if k not in chosen)
    for name, k, code in (("selno", not_chosen, 0), ("selyes", chosen[2], 2)):
        copy_set(tmp, "out", name)
        m = bytearray(read(tmp, name + ".checksums"))
        m[32 + 4 * k + 2] ^= 0x40
        with open(os.path.join(tmp, name + ".checksums"), "wb") as f:
            f.write(m)
        r = tool(["t"] + select + [name], tmp, ok=False)
        assert r.returncode == code, (name, r.stdout, r.stderr)
        assert summary(r.stdout) == (5, n, 1 if code else 0)
        assert bad_contigs(r.stdout) == ([k] if code else [])


def test_uppercase(runs):
    tmp = runs("m1R3").tmp
    tool(["c", "-m", "1", "-R", "3", "-U", "--checksums", "list.txt", "up"], tmp)
    seq, lens = decoded(tmp, "up", "upback")
    assert seq == seq.upper() and seq != runs("m1R3").seq
    assert read(tmp, "up.checksums") == python_manifest(tmp, "up", seq, lens)
    assert summary(tool(["t", "up"], tmp).stdout) == (len(lens), len(lens), 0)


def test_single_fasta_with_a_small_window(tmp_path):
    tmp = str(tmp_path)
    base = synth.base_codes(900_000, 12)
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        f.write(sfa.multi_fasta([synth.genome(base, i, 0.015) for i in range(8)]))
    out = tool(["c", "-i", "all.fa", "--window-kib", "64", "--checksums", "out"], tmp)
    assert "Switching to sequential" not in out.stderr
    seq, lens = decoded(tmp, "out", "back")
    assert len(lens) == 8
    assert read(tmp, "out.checksums") == python_manifest(tmp, "out", seq, lens)
    assert summary(tool(["t", "out"], tmp).stdout) == (8, 8, 0)


def test_repack_writes_the_new_sets_manifest(runs):
    tmp = runs("m1R3").tmp
    tool(["r", "--select", "g01.fa", "--select", "g03.fa", "--select", "g05.fa", "--checksums", "out", "new"], tmp)
    seq, lens = decoded(tmp, "new", "newback")
    assert read(tmp, "new.checksums") == python_manifest(tmp, "new", seq, lens)
    assert summary(tool(["t", "new"], tmp).stdout) == (len(lens), len(lens), 0)


def test_refusals(runs):
    tmp = runs("m1R3").tmp
    r = tool(["c", "--gpus", "2", "--checksums", "list.txt", "no"], tmp, ok=False)
    assert r.returncode != 0 and len(r.stderr.strip().splitlines()) == 1 and "--checksums runs on one GPU" in r.stderr
    assert not [f for f in os.listdir(tmp) if f.startswith("no.")]
    r = tool(["c", "--bench", "--checksums", "list.txt", "no"], tmp, ok=False)
    assert r.returncode != 0 and len(r.stderr.strip().splitlines()) == 1 and "--bench" in r.stderr
    for args in (["t", "base"], ["d", "--check", "base", "no"]):
        r = tool(args, tmp, ok=False)
        assert r.returncode == 1 and "base.checksums not found: write it with mbgc-hip c --checksums" in r.stderr, r.stderr
    assert not [f for f in os.listdir(tmp) if f.startswith("no.")]
    copy_set(tmp, "out", "more")
    m = read(tmp, "more.checksums")
    (n,) = struct.unpack_from("<Q", m, 8)
    with open(os.path.join(tmp, "more.checksums"), "wb") as f:
        f.write(m[:8] + struct.pack("<Q", n + 1) + m[16:] + b"\0\0\0\0")
    r = tool(["t", "more"], tmp, ok=False)
    assert r.returncode == 1 and "more.checksums" in r.stderr, r.stderr
