"""`mbgc-hip c`, then `mbgc-hip d` in a fresh process: the collection must come back — .seq / .contigLens / .seqCounts against
the bases tests/_fasta.py parses from the input files — and default `d`, `d --serial` and `d --no-index` must write the same
bytes. Malformed stream sets end with a message and exit 1."""
import lzma
import os
import re
import subprocess

import numpy as np
import pytest

import _fasta
import _meta
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
LIST = os.path.join(ROOT, "tests", "golden", "listeria")
OUTS = ("seq", "contigLens", "seqCounts")


def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def cut(g, k):
    cuts = [0] + [g.size * i // k + (7 * i) % 13 for i in range(1, k)] + [g.size]
    return [g[cuts[i]:cuts[i + 1]] for i in range(k)]


def write_collection(tmp, n, length, div=0.015, seed=55):
    """n synthetic genomes as FASTA files, targets cut into 2-3 records; one record of random bases (no match), one shorter than
    the k-mer, one target identical to G0 (loads nothing)"""
    base = synth.base_codes(length, seed)
    gs = [synth.genome(base, i, div) for i in range(n)]
    files = [[gs[0]]] + [cut(g, 2 + i % 2) for i, g in enumerate(gs[1:], 1)]
    files[2].append(synth.genome(synth.base_codes(9000, seed + 1), 0, 0.0))          # random bases
    files[3].insert(1, gs[3][100:117].copy())                                        # shorter than the k-mer
    files[n - 2] = [gs[0].copy()]                                                    # identical to G0
    lower = np.frombuffer(b"acgt", dtype=np.uint8)
    files[1][0] = files[1][0].copy()
    files[1][0][50:90] = lower[np.arange(40) % 4]                                    # (lower case: kept, or folded under -U)
    paths = []
    for i, contigs in enumerate(files):
        p = os.path.join(tmp, "g%02d.fa" % i)
        with open(p, "wb") as f:
            for j, c in enumerate(contigs):
                f.write(synth.fasta_bytes(c, i * 10 + j))
        paths.append(p)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    return paths


def expected(paths, uppercase):
    recs = [[s for _, s in _fasta.oracle_parse(open(p, "rb").read(), uppercase)["records"]] for p in paths]
    return recs


def check_outputs(tmp, name, recs_per_unit):
    seq = open(os.path.join(tmp, name + ".seq"), "rb").read()
    lens = np.fromfile(os.path.join(tmp, name + ".contigLens"), dtype="<u8")
    counts = np.fromfile(os.path.join(tmp, name + ".seqCounts"), dtype="<u4")
    flat = [s for unit in recs_per_unit for s in unit]
    assert lens.tolist() == [len(s) for s in flat]
    assert seq == b"".join(flat)
    assert counts.tolist() == [len(u) for u in recs_per_unit]


def decode_three_ways(tmp, prefix):
    """default, --serial, --no-index: byte-identical outputs; -> stdout of the default run"""
    outs = {}
    for name, extra in (("d0", []), ("d1", ["--serial"]), ("d2", ["--no-index"])):
        outs[name] = tool(["d"] + extra + [prefix, name], tmp).stdout
    for ext in OUTS:
        a = open(os.path.join(tmp, "d0." + ext), "rb").read()
        for other in ("d1", "d2"):
            assert open(os.path.join(tmp, other + "." + ext), "rb").read() == a, (other, ext)
    return outs["d0"]


CASES = [
    (["-m", "0", "-R", "3"], 7), (["-m", "1", "-R", "3"], 7), (["-m", "2", "-R", "3"], 7),
    (["-m", "0", "-t1"], 5), (["-m", "1", "-t1"], 6), (["-m", "2", "-t1"], 5),
    (["-L", "-R", "3"], 7), (["-L", "-t1"], 5),
    (["-s", "15", "-R", "3"], 6), (["-s", "15", "-t1"], 5),
    (["-U", "-R", "4"], 9),
    # other matching lengths (-k: the matcher's L, matchTexts' minimal length and .meta's k): K = 12, 20, 28 (L = 40) and 16
    (["-k", "16", "-R", "3"], 7), (["-k", "24", "-t1"], 5), (["-k", "40", "-R", "3"], 7), (["-k", "20", "-m", "2", "-R", "3"], 7),
]


@pytest.mark.parametrize("args,n", CASES, ids=[" ".join(a) for a, _ in CASES])
def test_collection_comes_back(tmp_path, args, n):
    tmp = str(tmp_path)
    paths = write_collection(tmp, n, 100_000 + 2000 * n)
    tool(["c"] + args + ["list.txt", "out"], tmp)
    assert os.path.exists(os.path.join(tmp, "out.meta"))
    if "-k" in args:
        assert _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())["k"] == int(args[args.index("-k") + 1])
    out = decode_three_ways(tmp, "out")
    check_outputs(tmp, "d0", expected(paths, "-U" in args))
    m = re.search(r"waves: (\d+) for (\d+) targets", out)
    assert m and int(m.group(2)) == (n if "-t1" in args else n - 1)
    if "-t1" in args:
        assert int(m.group(1)) == int(m.group(2))                                   # every target alone
    elif args[-2:] == ["-R", "3"] and "-L" not in args and "-s" not in args:
        assert int(m.group(1)) < int(m.group(2))                                    # some wave held more than one target
        assert int(re.search(r"widest wave: (\d+) targets", out).group(1)) > 1


@pytest.mark.parametrize("args", [["-R", "2"], ["-t1"], ["-L", "-R", "2"]], ids=lambda a: " ".join(a))
def test_reference_buffer_wraps_at_least_twice(tmp_path, args):
    """--ref-factor 1: the smallest buffer the tool makes, 2 x MIN_BASIC_BLOCK_SIZE (2 MiB) = 4 MiB. -t1 has no window: three
    unrelated contigs of 2.4 Mbp, each loaded with its reverse complement, go round it three times. A round loads up to the
    window's end — the buffer's end before the first lap, then a sixteenth of the buffer: one such contig fills the first lap, 80
    unrelated files of 60 kbp in rounds of two (240 kbp with the reverse complements, just inside the window) the next two."""
    tmp = str(tmp_path)
    paths = write_collection(tmp, 9, 120_000)
    big = synth.base_codes(2_400_000, 77)
    if "-t1" in args:
        for i in range(3, 6):
            with open(paths[i], "ab") as f:
                f.write(synth.fasta_bytes(synth.genome(big, i, 0.3), 900 + i))
    else:
        with open(paths[1], "ab") as f:
            f.write(synth.fasta_bytes(synth.genome(big, 1, 0.3), 901))
        for i in range(80):
            p = os.path.join(tmp, "u%02d.fa" % i)
            with open(p, "wb") as f:
                f.write(synth.fasta_bytes(synth.genome(synth.base_codes(60_000, 1000 + i), 0, 0.0), 2000 + i))
            paths.append(p)
        with open(os.path.join(tmp, "list.txt"), "w") as f:
            f.write("\n".join(paths) + "\n")
    c = tool(["c", "--ref-factor", "1"] + args + ["list.txt", "out"], tmp)
    meta = _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())
    assert meta["laps"] >= 2, meta["laps"]                                           # the case covers the wrap, or fails
    assert "final reference length: %d" % meta["max_ref_length"] in c.stdout
    decode_three_ways(tmp, "out")
    check_outputs(tmp, "d0", expected(paths, False))


@pytest.mark.parametrize("args", [[], ["-t1"]], ids=["rounds", "t1"])
def test_single_fasta_input(tmp_path, args):
    tmp = str(tmp_path)
    base = synth.base_codes(110_000, 5)
    recs = []
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        for i in range(100 if not args else 9):
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                f.write(synth.fasta_bytes(c, i * 10 + j))
                recs.append(c.tobytes())
    tool(["c", "-i", "all.fa"] + args + ["out"], tmp)
    meta = _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())
    assert meta["single_fasta"] and meta["sequential"] == bool(args)
    decode_three_ways(tmp, "out")
    seq = open(os.path.join(tmp, "d0.seq"), "rb").read()
    lens = np.fromfile(os.path.join(tmp, "d0.contigLens"), dtype="<u8")
    counts = np.fromfile(os.path.join(tmp, "d0.seqCounts"), dtype="<u4")
    assert lens.tolist() == [len(r) for r in recs] and seq == b"".join(recs)
    c_counts = np.fromfile(os.path.join(tmp, "out.seqCounts"), dtype="<u4")          # what c wrote: the targets' records
    assert counts.tolist() == ([] if args else [meta["g0_contigs"]]) + c_counts.tolist()
    assert int(counts.sum()) == len(recs)


@pytest.mark.parametrize("args", [["-t1"], ["-R", "2"]], ids=lambda a: " ".join(a))
def test_listeria(tmp_path, args):
    tmp = str(tmp_path)
    import json
    exp = json.load(open(os.path.join(LIST, "expected_t1.json")))
    paths = []
    for f in exp["files"]:
        p = os.path.join(tmp, f)
        with open(p, "wb") as o:
            o.write(lzma.open(os.path.join(LIST, f + ".xz")).read())
        paths.append(p)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    tool(["c"] + args + ["list.txt", "lm"], tmp)
    decode_three_ways(tmp, "lm")
    check_outputs(tmp, "d0", expected(paths, False))


# ---- rejection: a message, exit 1, no fault and no hang (the automaton's bounds checks catch every one of these)
@pytest.fixture(scope="module")
def small_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("rej"))
    write_collection(tmp, 6, 100_000)
    tool(["c", "-R", "3", "list.txt", "out"], tmp)
    return tmp


def copy_run(src, dst, change):
    for f in os.listdir(src):
        if f.startswith("out."):
            data = open(os.path.join(src, f), "rb").read()
            data = change(f[4:], data)
            with open(os.path.join(dst, f), "wb") as o:
                o.write(data)


def refused(tmp, extra=()):
    r = tool(["d"] + list(extra) + ["out", "back"], tmp, ok=False)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "mbgc-hip d: " in r.stderr
    assert not os.path.exists(os.path.join(tmp, "back.seq"))
    return r.stderr


@pytest.mark.parametrize("extra", [[], ["--no-index"], ["--serial"]], ids=lambda e: " ".join(e) or "default")
def test_truncated_maplen_is_refused(small_run, tmp_path, extra):
    copy_run(small_run, str(tmp_path), lambda name, d: d[:-1] if name == "mapLen" else d)
    assert "malformed" in refused(str(tmp_path), extra)


@pytest.mark.parametrize("extra", [[], ["--no-index"]], ids=lambda e: " ".join(e) or "default")
def test_trailing_byte_in_gapdelta_is_refused(small_run, tmp_path, extra):
    copy_run(small_run, str(tmp_path), lambda name, d: d + b"\x01" if name == "gapDelta" else d)
    assert "malformed" in refused(str(tmp_path), extra)


@pytest.mark.parametrize("stream,delta", [(3, 1), (1, -4), (5, 1), (0, 1)])
def test_index_entry_off_by_one_is_refused(small_run, tmp_path, stream, delta):
    def change(name, d):
        if name != "meta":
            return d
        m = _meta.parse(d)
        m["index"][2][stream] += delta
        return _meta.build(m)
    copy_run(small_run, str(tmp_path), change)
    assert "malformed" in refused(str(tmp_path))
    tool(["d", "--no-index", "out", "fine"], str(tmp_path))                        # the streams themselves are whole


def test_m3_is_refused(tmp_path):
    tmp = str(tmp_path)
    write_collection(tmp, 5, 100_000)
    tool(["c", "-m", "3", "list.txt", "out"], tmp)
    err = refused(tmp)
    assert "-m 3" in err and "rcMapOff" in err


def test_missing_meta_is_refused(small_run, tmp_path):
    copy_run(small_run, str(tmp_path), lambda name, d: d)
    os.remove(os.path.join(str(tmp_path), "out.meta"))
    assert ".meta" in refused(str(tmp_path))
