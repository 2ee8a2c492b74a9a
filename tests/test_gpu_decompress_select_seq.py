"""`mbgc-hip d --select-seq`: only the records whose header contains a pattern, and the contigs they depend on, are decoded. The
oracle is the unselected `d --fasta` of the same streams, cut in Python: every full file is parsed into records, a record is kept
when its header line (without the '>') contains a pattern (`bytes.__contains__`) and — with --select — its file's name does, and
.seq / .contigLens are sliced by the same record indices. The three outputs and the --fasta directory (file set and bytes) must be
that cut, from the default run, --serial, --no-index and streams of c -t1 and c -m 3; --closure-out must be per contig."""
import os
import re
import types
import zlib

import numpy as np
import pytest

import _singlefasta as sfa
import test_gpu_decompress_select as whole_files
from mbgc_amd import synth
from test_gpu_decompress_select import Full, N, OUTS, tool, write_collection

pytestmark = pytest.mark.gpu
STREAMS = {"m1R3": (["-m", "1", "-R", "3"], []), "m0t1": (["-m", "0", "-t1"], []), "m3t1": (["-m", "3", "-t1"], ["--restore-rc"])}
RUNS = [("m1R3", []), ("m1R3", ["--serial"]), ("m1R3", ["--no-index"]), ("m0t1", []), ("m3t1", [])]
# the headers of write_collection: "synth%05d synthetic genome %d 99pct identity" with the number 10 x file + record; file 0 (G0's): 0;
# 1: 10-12; 2: 20-22 (22: random bases); 3: 30-33 (31: shorter than k); 4: 40, 41; 5: 50 (identical to G0); 6: 60, 61
CASES = {
    "middle": (["--select-seq", "synth00011 "], [b"synth00011 "], None),                                  # one record in the middle of a file
    "file3": (["--select-seq", "genome 3"], [b"genome 3"], None),                                          # 30, 31, 32, 33
    "scattered": (["--select-seq", "1 99pct"], [b"1 99pct"], None),                                        # 11, 21, 31, 41, 61: five files
    "g0": (["--select-seq", "synth00000 "], [b"synth00000 "], None),                                       # the record of G0's file
    "both": (["--select", "g03.fa", "--select", "g06", "--select-seq", "1 99pct"], [b"1 99pct"], [b"g03.fa", b"g06"]),   # 31, 61
    "list": (["--select-seq-list", "records.txt", "--select-seq", "genome 50 "], [b"synth00022 ", b"genome 60 ", b"synth00012 ", b"genome 50 "], None),
}


def records_of(text):
    """a FASTA file's text -> [(header line without '>', the record's text)]"""
    starts = [0] + [m.start() + 1 for m in re.finditer(b"\n>", text)] if text else []
    out = []
    for a, b in zip(starts, starts[1:] + [len(text)]):
        assert text[a:a + 1] == b">"
        out.append((text[a + 1: text.index(b"\n", a)], text[a:b]))
    return out


class Cut:
    """what a record selection leaves of an unselected run (Full): the oracle"""

    def __init__(self, full, patterns, file_patterns=None, one_file=False):
        names = ["all.fa"] if one_file else [os.path.basename(p) for p in full.paths]
        listed = ["all.fa"] if one_file else full.paths
        self.chosen, self.fasta, counts, g = [], {}, [], 0                             # chosen: indices into the unselected run's contigs
        for f, name in enumerate(names):
            recs = records_of(open(os.path.join(full.tmp, "full_fa", name), "rb").read())
            passes = file_patterns is None or any(q in listed[f].encode() for q in file_patterns)
            keep = [j for j, (h, _) in enumerate(recs) if passes and any(q in h for q in patterns)]
            if keep:
                self.fasta[name] = b"".join(recs[j][1] for j in keep)
                counts.append(len(keep))
            self.chosen += [g + j for j in keep]
            g += len(recs)
        assert g == full.lens.size
        self.seq = b"".join(full.seq[full.off[c]:full.off[c + 1]] for c in self.chosen)
        self.lens = full.lens[self.chosen].astype("<u8").tobytes()
        self.counts = np.asarray(counts, dtype="<u4").tobytes()
        self.files = len(counts)


def check_cut(full, cut, args, name, extra=(), fasta_args=(), fasta_suffix=""):
    """one `d` run with a record selection against the cut; -> (stdout, the bytes of --closure-out)"""
    tmp = full.tmp
    out = tool(["d"] + full.extra + list(extra) + args + ["--fasta", name + "_fa"] + list(fasta_args) + ["--closure-out", name + ".closure", "out", name], tmp).stdout
    for ext, want in zip(OUTS, (cut.seq, cut.lens, cut.counts)):
        assert open(os.path.join(tmp, name + "." + ext), "rb").read() == want, (name, ext)
    assert sorted(os.listdir(os.path.join(tmp, name + "_fa"))) == sorted(f + fasta_suffix for f in cut.fasta)
    closure = np.fromfile(os.path.join(tmp, name + ".closure"), dtype=np.uint8)
    shift = full.lens.size - full.planned                                             # G0's contigs, which are no target's (none under -t1)
    assert closure.size == full.planned
    chosen_planned = [c - shift for c in cut.chosen if c >= shift]
    assert np.flatnonzero(closure == 2).tolist() == chosen_planned                    # 2 exactly on the chosen contigs
    assert not closure[(max(chosen_planned) + 1 if chosen_planned else 0):].any()     # nothing behind the last chosen contig is needed
    m = re.search(r"closure: (\d+) of (\d+) contigs, (\d+) of (\d+) bases, (\d+) selected, (\d+) dependency targets", out)
    assert m, out
    assert int(m.group(1)) == int((closure != 0).sum()) and int(m.group(2)) == full.planned and int(m.group(5)) == cut.files
    assert "records: %d of %d chosen in %d files\n" % (len(cut.chosen), full.lens.size, cut.files) in out
    assert "decoded: %d contigs, %d bases\n" % (len(cut.chosen), len(cut.seq)) in out
    return out, closure


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    made = {}

    def get(mode):
        if mode not in made:
            tmp = str(tmp_path_factory.mktemp(mode))
            paths = write_collection(tmp, N, 100_000 + 2000 * N)
            tool(["c"] + STREAMS[mode][0] + ["list.txt", "out"], tmp)
            with open(os.path.join(tmp, "records.txt"), "w") as f:
                f.write("synth00022 \ngenome 60 \n\nsynth00012 \n")
            made[mode] = Full(tmp, paths, STREAMS[mode][1])
        return made[mode]
    return get


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode,extra", RUNS, ids=["default", "serial", "no-index", "t1", "m3"])
def test_selected_records_come_back(runs, mode, extra, case):
    full = runs(mode)
    args, patterns, file_patterns = CASES[case]
    cut = Cut(full, patterns, file_patterns)
    assert cut.chosen and len(cut.chosen) < full.lens.size
    name = case + "".join(extra).replace("-", "")
    check_cut(full, cut, args, name, extra)
    for f, text in cut.fasta.items():
        assert open(os.path.join(full.tmp, name + "_fa", f), "rb").read() == text, (name, f)


def test_the_cases_choose_what_they_are_named_for(runs):
    full = runs("m1R3")
    first = full.first.tolist()
    assert Cut(full, CASES["middle"][1]).chosen == [first[1] + 1]
    assert Cut(full, CASES["file3"][1]).chosen == list(range(first[3], first[4])) and first[4] - first[3] == 4
    assert Cut(full, CASES["scattered"][1]).chosen == [first[f] + 1 for f in (1, 2, 3, 4, 6)]
    assert Cut(full, CASES["g0"][1]).chosen == [0]
    assert Cut(full, CASES["both"][1], CASES["both"][2]).chosen == [first[3] + 1, first[6] + 1]
    assert Cut(full, CASES["list"][1]).chosen == [first[1] + 2, first[2] + 2, first[5], first[6]]


def test_an_unchosen_contig_of_a_file_with_chosen_ones_is_not_filled_for_its_own_sake(runs):
    """--closure-out is per contig: with one record of file 6 chosen, the file's other record is 0 unless something chosen was matched
    against it — and it lies behind the chosen one, so nothing was"""
    full = runs("m1R3")
    cut = Cut(full, [b"synth00060 "])
    out, closure = check_cut(full, cut, ["--select-seq", "synth00060 "], "one_of_two")
    planned = list(full.planned_range(6))
    assert len(planned) == 2 and closure[planned].tolist() == [2, 0]
    whole, _ = whole_files.check_selection(full, [6], ["--select", "g06.fa"], whole_files.VARIANTS[:1])
    bases = lambda text: int(re.search(r"contigs, (\d+) of", text).group(1))
    assert bases(out) < bases(whole)                                                  # less is decoded than for the whole file


def gunzip_members(data):
    """-> (the text, the number of gzip members it came in)"""
    text, members = b"", 0
    while data:
        assert data[:2] == b"\x1f\x8b"
        d = zlib.decompressobj(31)
        text += d.decompress(data) + d.flush()
        assert d.eof
        data, members = d.unused_data, members + 1
    return text, members


def test_gzip_files_hold_the_cut_and_scattered_records_of_a_batch_are_one_member(runs):
    full = runs("m1R3")
    # file 3: 31 (17 bases) and 33 with 32 between them — two runs of one file, 39 KB of text, in one batch of 64 KiB; file 6's record
    # (57 KB) is the next batch
    patterns = [b"synth00031 ", b"synth00033 ", b"synth00061 "]
    args = sum((["--select-seq", q.decode()] for q in patterns), [])
    cut = Cut(full, patterns)
    assert cut.chosen == [full.first[3] + 1, full.first[3] + 3, full.first[6] + 1]
    assert len(cut.fasta["g03.fa"]) < 64 << 10
    check_cut(full, cut, args, "gz", fasta_args=["--gzip", "--batch-kib", "64"], fasta_suffix=".gz")
    for f, text in cut.fasta.items():
        got, members = gunzip_members(open(os.path.join(full.tmp, "gz_fa", f + ".gz"), "rb").read())
        assert got == text, f
        assert members == 1, (f, members)


def test_bench_reports_the_match(runs):
    full = runs("m1R3")
    out = tool(["d", "--bench", "--select-seq", "1 99pct", "--select-seq-host", "out", "bench"], full.tmp).stdout
    m = re.search(r'"header_match_ms": ([0-9.]+), "records_chosen": (\d+)', out)
    assert m and int(m.group(2)) == 5, out
    assert '"header_match_host_ms"' in out and "records: 5 of %d chosen in 5 files" % full.lens.size in out
    assert not os.path.exists(os.path.join(full.tmp, "bench.seq"))                    # (--bench writes no sequence files, as before)


# ---- refusals: a message, exit 1, nothing written
def refused(tmp, tool_args, word, letter="d"):
    r = tool(tool_args, tmp, ok=False)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "mbgc-hip %s: " % letter in r.stderr and word in r.stderr, r.stderr
    if letter != "d":
        assert len(r.stderr.strip().splitlines()) == 1, r.stderr                      # one clear line
    for f in ("no.seq", "no.contigLens", "no.seqCounts", "no.closure", "no_fa", "no.meta"):
        assert not os.path.exists(os.path.join(tmp, f)), f


def test_refusals(runs, tmp_path):
    full = runs("m1R3")
    sinks = ["--fasta", "no_fa", "--closure-out", "no.closure", "out", "no"]
    refused(full.tmp, ["d", "--select-seq", "no-such-record"] + sinks, "--select-seq: no record of the collection matches")
    refused(full.tmp, ["d", "--select", "g02.fa", "--select-seq", "synth00011 "] + sinks, "--select-seq: no record of the collection matches")   # (11 is file 1's)
    refused(full.tmp, ["d", "--select", "no-such-file", "--select-seq", "synth00011 "] + sinks, "--select: no file of the collection matches")
    refused(full.tmp, ["d", "--select-seq", ""] + sinks, "empty pattern")
    open(os.path.join(full.tmp, "empty.txt"), "w").close()
    refused(full.tmp, ["d", "--select-seq-list", "empty.txt"] + sinks, "the list of patterns is empty")
    refused(full.tmp, ["v", "--select-seq", "synth00011 ", "out"], "--select-seq", "v")
    refused(full.tmp, ["r", "--select-seq-list", "records.txt", "out", "no"], "--select-seq", "r")
    tmp = str(tmp_path)
    for f in os.listdir(full.tmp):
        if f.startswith("out.") and f not in ("out.headers", "out.names"):
            with open(os.path.join(tmp, f), "wb") as o:
                o.write(open(os.path.join(full.tmp, f), "rb").read())
    r = tool(["d", "--select-seq", "synth00011 ", "out", "no"], tmp, ok=False)
    assert r.returncode == 1 and "malformed stream set: cannot open" in r.stderr and "out.headers" in r.stderr
    with open(os.path.join(tmp, "out.headers"), "wb") as o:
        o.write(open(os.path.join(full.tmp, "out.headers"), "rb").read())
    tool(["d", "--select-seq", "synth00011 ", "out", "yes"], tmp)                      # the headers alone are enough without --select and --fasta
    assert open(os.path.join(tmp, "yes.seq"), "rb").read() == Cut(full, [b"synth00011 "]).seq
    r = tool(["d", "--select", "g01", "--select-seq", "synth00011 ", "out", "no"], tmp, ok=False)
    assert r.returncode == 1 and "malformed stream set: cannot open" in r.stderr and "out.names" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "no.seq"))


def test_select_alone_is_as_before(runs):
    """--select without --select-seq: the outputs by check_selection's rules (whole files, every contig of a chosen file 2, one
    .seqCounts entry per chosen file), and the four lines of stdout in their format, no `records:` line among them"""
    full = runs("m1R3")
    out, closure = whole_files.check_selection(full, [2, N - 2], ["--select", "g02.fa", "--select", "g%02d.fa" % (N - 2)])
    lines = out.splitlines()
    assert len(lines) == 4, out
    assert re.fullmatch(r"closure: \d+ of %d contigs, \d+ of \d+ bases, 2 selected, \d+ dependency targets" % full.planned, lines[0])
    assert re.fullmatch(r"waves: \d+ for %d targets" % (N - 1), lines[1])
    assert re.fullmatch(r"widest wave: \d+ targets", lines[2])
    want = full.expect([2, N - 2])
    assert lines[3] == "decoded: %d contigs, %d bases" % (len(want[1]) // 8, len(want[0]))


# ---- a single-FASTA set: its elements are no files, --select has nothing to choose from, --select-seq has
@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """12 records of 0.9 Mbp in one file: G0 is the first, the targets of the round schedule are the elements of 2 MiB behind it —
    records 1-3, 4-6, 7-9, 10-11"""
    tmp = str(tmp_path_factory.mktemp("single"))
    base = synth.base_codes(900_000, 12)
    data = sfa.multi_fasta([synth.genome(base, i, 0.015) for i in range(12)])
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        f.write(data)
    out = tool(["c", "-i", "all.fa", "out"], tmp)
    assert "Switching to sequential" not in out.stderr
    assert [len(records_of(e)) for e in sfa.elements(data)] == [1, 3, 3, 3, 2]
    tool(["d", "--fasta", "full_fa", "out", "full"], tmp)
    lens = np.fromfile(os.path.join(tmp, "full.contigLens"), dtype="<u8")
    # (what Cut and check_cut read of a Full; planned: G0 is the first record)
    return types.SimpleNamespace(tmp=tmp, paths=["all.fa"], extra=[], seq=open(os.path.join(tmp, "full.seq"), "rb").read(), lens=lens,
                                 off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), planned=11)


@pytest.mark.parametrize("which", [(4, 10), (0, 5, 6)], ids=["two-targets", "g0-and-a-run"])
def test_single_fasta_records(single, which):
    full = single
    patterns = [b"synth%05d " % r for r in which]
    cut = Cut(full, patterns, one_file=True)
    assert cut.chosen == list(which) and list(cut.fasta) == ["all.fa"]
    assert np.frombuffer(cut.counts, dtype="<u4").tolist() == [len(which)]           # one entry: the one file
    name = "s" + "_".join(str(r) for r in which)
    out, closure = check_cut(full, cut, sum((["--select-seq", q.decode()] for q in patterns), []), name)
    assert open(os.path.join(full.tmp, name + "_fa", "all.fa"), "rb").read() == cut.fasta["all.fa"]
    m = re.search(r"closure: \d+ of \d+ contigs, (\d+) of (\d+) bases, 1 selected", out)
    assert m and int(m.group(1)) < int(m.group(2)), out                               # fewer bases than the whole


def test_single_fasta_select_by_name_is_still_refused(single):
    refused(single.tmp, ["d", "--select", "all.fa", "--fasta", "no_fa", "--closure-out", "no.closure", "out", "no"], "it has one name, there is nothing to select")
    refused(single.tmp, ["d", "--select", "all.fa", "--select-seq", "synth00004 ", "--fasta", "no_fa", "out", "no"], "it has one name, there is nothing to select")
