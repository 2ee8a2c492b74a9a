"""`mbgc-hip d --region 'PATTERN:FROM-TO'`: parts of records, the closure and the fill cut to them. The oracle is the unselected `d` of
the same streams, cut in Python: a piece is bytes [FROM - 1, min(TO, length)) of a record of full.seq, the pieces ordered by record,
FROM, TO, identical ones once. The set is a chain — 8 files of one 64 KiB contig, file i = file i - 1 with a substitution about
every 500 bases — and a file of three records, compressed with `c` and with `c -m 3`."""
import os
import re
import zlib

import numpy as np
import pytest

from _regionprobe import OUTS, WIDTH, Full, args_of, expect, fasta, piece_text, run_regions, tool
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
LEN, CHAIN, G = 64 << 10, 8, 256                       # G: the granule that ships (mbgc_decoder.h: regionGranule)


def headers():
    """per file, per record; the last file's second header holds a ':' of its own"""
    return [[b"chain%d link %d of the chain" % (i, i)] for i in range(CHAIN)] + [[b"trio_a first of three", b"trio:b second:of three", b"trio_c third of three"]]


def write_set(tmp):
    rng = np.random.default_rng(77)
    codes = synth.base_codes(LEN, 4242)
    seqs = []
    for i in range(CHAIN):
        if i:
            codes = codes.copy()
            at = np.flatnonzero(rng.random(LEN) < 1 / 500)
            codes[at] = (codes[at] + rng.integers(1, 4, at.size)) & 3
        seqs.append([synth.ACGT[codes].tobytes()])
    seqs.append([synth.ACGT[synth.genome_codes(codes, 50 + j, 0.01)[j * 1000:j * 1000 + 9000 + 17 * j]].tobytes() for j in range(3)])
    paths = []
    for i, (hs, ss) in enumerate(zip(headers(), seqs)):
        paths.append(os.path.join(tmp, "f%02d.fa" % i))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(fasta(h, s) for h, s in zip(hs, ss)))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        f.write(b"".join(open(p, "rb").read() for p in paths))
    return paths


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("region"))
    write_set(tmp)
    tool(["c", "list.txt", "out"], tmp)
    tool(["c", "-m", "3", "list.txt", "m3"], tmp)
    tool(["c", "-i", "all.fa", "one"], tmp)
    return {"plain": Full(tmp, headers=headers()), "m3": Full(tmp, ["--restore-rc"], "m3", headers=headers()), "one": Full(tmp, [], "one", True, headers=headers())}


LAST = b"chain%d " % (CHAIN - 1)
CASES = {
    "middle": [(LAST, 30_001, 32_048)],
    "first-base": [(LAST, 1, 1)],
    "last-base": [(LAST, LEN, LEN)],
    "one-past-a-granule-edge": [(LAST, 5 * G, 5 * G + 1)],         # the last byte of granule 4 and the first of granule 5
    "up-to-a-granule-edge": [(LAST, 5 * G + 1, 6 * G)],            # granule 5 exactly: not a byte of its neighbours
    "one-before-and-behind": [(LAST, 5 * G, 6 * G + 1)],
    "to-beyond-the-end": [(LAST, LEN - 99, LEN + 5000)],
    "from-beyond-the-end": [(LAST, LEN + 1, LEN + 10), (LAST, 10, 20)],
    "overlapping": [(LAST, 1000, 3000), (LAST, 2000, 2500), (LAST, 2000, 4000)],
    "twice": [(LAST, 700, 900), (LAST, 700, 900)],
    "three-records": [(b"trio", 8000, 9020)],                      # record 0 has 9000 bases, 1: 9017, 2: 9034
    "colon-in-header": [(b"trio:b second:of", 5, 44)],
}


@pytest.mark.parametrize("case", list(CASES))
def test_regions_are_the_python_cut(sets, case):
    full = sets["plain"]
    out, pieces = run_regions(full, CASES[case], case.replace("-", "_"))
    if case == "from-beyond-the-end":
        assert "1 out of range" in out and len(pieces) == 1
    if case == "overlapping":
        assert len(pieces) == 3                                    # each is written
    if case == "twice":
        assert len(pieces) == 1
    if case == "three-records":
        assert [r for r, _, _ in pieces] == [CHAIN, CHAIN + 1, CHAIN + 2] and [n for _, _, n in pieces] == [1001, 1018, 1021]


def test_only_out_of_range_writes_nothing_and_counts(sets):
    full = sets["plain"]
    out, pieces = run_regions(full, [(LAST, LEN + 1, LEN + 2)], "nothing")
    assert pieces == [] and "regions: 0 pieces of 0 records, 0 bases, 1 out of range" in out


def test_select_excludes_the_file(sets):
    full = sets["plain"]
    specs = [(b"link", 100, 199)]                                  # every chain record
    pieces, _ = full.cut(specs, files={2, 5})
    out = tool(["d", "--select", "f02.fa", "--select", "f05.fa"] + args_of(specs) + ["out", "sel"], full.tmp).stdout
    for ext, want in zip(OUTS, expect(full, pieces)):
        assert open(os.path.join(full.tmp, "sel." + ext), "rb").read() == want, ext
    assert len(pieces) == 2 and "regions: 2 pieces of 2 records, 200 bases, 0 out of range" in out


def test_fasta_line_breaks_and_header_text(sets):
    full = sets["plain"]
    specs = [(LAST, 101, 100 + 3 * WIDTH + 5), (b"trio", 1, WIDTH), (b"trio:b", 8000, 99999)]
    out, pieces = run_regions(full, specs, "fa", fasta_args=[])
    assert sorted(os.listdir(os.path.join(full.tmp, "fa_fa"))) == ["f%02d.fa" % (CHAIN - 1), "f%02d.fa" % CHAIN]      # a file without a piece is not written
    for f in (CHAIN - 1, CHAIN):
        want = b"".join(piece_text(full, r, a, n) for r, a, n in pieces if full.file_of[r] == f)
        assert open(os.path.join(full.tmp, "fa_fa", "f%02d.fa" % f), "rb").read() == want, f
    text = open(os.path.join(full.tmp, "fa_fa", "f%02d.fa" % CHAIN), "rb").read()
    assert b">trio:b:8000-9017 second:of three\n" in text and b">trio_a:1-70 first of three\n" in text


def test_fasta_gzip_reads_back_with_zlib(sets):
    full = sets["plain"]
    out, pieces = run_regions(full, [(LAST, 101, 5000), (LAST, 60_000, 60_100)], "gz", fasta_args=["--gzip"])
    data = open(os.path.join(full.tmp, "gz_fa", "f%02d.fa.gz" % (CHAIN - 1)), "rb").read()
    text = b""
    while data:
        d = zlib.decompressobj(31)
        text += d.decompress(data) + d.flush()
        assert d.eof
        data = d.unused_data
    assert text == b"".join(piece_text(full, r, a, n) for r, a, n in pieces)


@pytest.mark.parametrize("extra", [["--serial"], ["--no-index"]], ids=["serial", "no-index"])
def test_serial_and_no_index_give_the_same_bytes(sets, extra):
    run_regions(sets["plain"], CASES["middle"] + CASES["three-records"], "v" + extra[0].strip("-").replace("-", ""), extra)


def test_restore_rc_on_the_m3_set(sets):
    full = sets["m3"]
    r = tool(["d"] + args_of(CASES["middle"]) + ["m3", "no"], full.tmp, ok=False)
    assert r.returncode == 1 and "--restore-rc" in r.stderr
    run_regions(full, CASES["middle"] + CASES["three-records"] + CASES["one-before-and-behind"], "m3r")


def test_single_fasta_set(sets):
    full = sets["one"]
    out, pieces = run_regions(full, CASES["middle"] + CASES["three-records"], "onep", fasta_args=[])
    assert np.fromfile(os.path.join(full.tmp, "onep.seqCounts"), dtype="<u4").tolist() == [4]      # the one file
    assert open(os.path.join(full.tmp, "onep_fa", "all.fa"), "rb").read() == b"".join(piece_text(full, r, a, n) for r, a, n in pieces)


def test_region_list_and_bench_and_closure_out(sets):
    full = sets["plain"]
    with open(os.path.join(full.tmp, "regions.txt"), "w") as f:
        f.write("chain7 :30001-32048\n\ntrio:b second:of:5-44\n")
    pieces, _ = full.cut(CASES["middle"] + CASES["colon-in-header"])
    out = tool(["d", "--region-list", "regions.txt", "--closure-out", "list.closure", "out", "list"], full.tmp).stdout
    for ext, want in zip(OUTS, expect(full, pieces)):
        assert open(os.path.join(full.tmp, "list." + ext), "rb").read() == want, ext
    closure = np.fromfile(os.path.join(full.tmp, "list.closure"), dtype=np.uint8)
    planned = full.lens.size - 1                                   # the first file is the initial reference
    assert closure.size == planned and closure[CHAIN - 2] == 2 and closure[CHAIN] == 2 and not closure[CHAIN + 1:].any()
    out = tool(["d", "--bench", "--region-list", "regions.txt", "out", "benchno"], full.tmp).stdout
    assert re.search(r'"regions": 2, "region_bases": 2088, "granule_bytes": %d' % G, out), out
    assert not os.path.exists(os.path.join(full.tmp, "benchno.seq"))


def test_narrowing(sets):
    """a 2 KiB region of the last chain file fills less than a quarter of what --select-seq of that record fills: with records of
    about 500 bases the needed span grows by about a record and a granule per level of the chain"""
    full = sets["plain"]
    out, _ = run_regions(full, [(LAST, 30_001, 32_048)], "narrow")
    whole = tool(["d", "--select-seq", LAST.decode(), "out", "whole"], full.tmp).stdout
    filled = lambda text: int(re.search(r"closure: \d+ of \d+ contigs, (\d+) of \d+ bases", text).group(1))
    print("filled: region %d, --select-seq %d" % (filled(out), filled(whole)))
    assert 0 < filled(out) < filled(whole) / 4


def test_refusals(sets):
    full = sets["plain"]

    def refused(args, word, letter="d"):
        r = tool(args, full.tmp, ok=False)
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert "mbgc-hip %s: " % letter in r.stderr and word in r.stderr, r.stderr
        assert not os.path.exists(os.path.join(full.tmp, "no.seq"))
    refused(["d", "--region", "chain7 :1-5", "--select-seq", "chain7", "out", "no"], "--select-seq")
    open(os.path.join(full.tmp, "pats.txt"), "w").write("chain7\n")
    refused(["d", "--region", "chain7 :1-5", "--select-seq-list", "pats.txt", "out", "no"], "--select-seq")
    refused(["d", "--region", "chain7 :1-5", "--check", "out", "no"], "--check")
    refused(["t", "--region", "chain7 :1-5", "out"], "--region", "t")
    refused(["v", "--region", "chain7 :1-5", "out"], "--region", "v")
    refused(["r", "--region", "chain7 :1-5", "out", "no"], "--region", "r")
    refused(["d", "--region", "chain7 :5-1", "out", "no"], "FROM lies behind TO")
    refused(["d", "--region", "chain7 :0-1", "out", "no"], "1-based")
    refused(["d", "--region", ":1-2", "out", "no"], "empty pattern")
    refused(["d", "--region", "chain7", "out", "no"], "PATTERN:FROM-TO")
    refused(["d", "--region", "no-such-record:1-2", "out", "no"], "--region: no record of the collection matches")
    open(os.path.join(full.tmp, "none.txt"), "w").close()
    refused(["d", "--region-list", "none.txt", "out", "no"], "the list of regions is empty")


def test_without_region_nothing_changes(sets):
    full = sets["plain"]
    again = tool(["d", "out", "again"], full.tmp).stdout
    assert again == full.stdout and "regions:" not in again and "closure:" not in again
    for ext in OUTS:
        assert open(os.path.join(full.tmp, "again." + ext), "rb").read() == open(os.path.join(full.tmp, "out_full." + ext), "rb").read()
    recs = [s for p in sorted(os.listdir(full.tmp)) if re.fullmatch(r"f\d\d\.fa", p)
            for s in re.findall(rb">[^\n]*\n([^>]*)", open(os.path.join(full.tmp, p), "rb").read())]
    assert full.seq == b"".join(s.replace(b"\n", b"") for s in recs)                  # the unselected run is the input's bases
