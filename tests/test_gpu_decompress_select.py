"""`mbgc-hip d --select`: only the chosen files and the contigs they depend on are decoded. The chosen files must come back as the
slices of an unselected `d` of the same streams — .seq / .contigLens / .seqCounts and the --fasta files, the same bytes from the
default, --serial and --no-index runs — and the closure (--closure-out: a byte per contig of the targets) must hold what the
files were matched against and, where that is known, nothing else."""
import os
import re
import subprocess

import numpy as np
import pytest

import _driver
import _meta
import _orc
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
OUTS = ("seq", "contigLens", "seqCounts")
VARIANTS = (("v0", []), ("v1", ["--serial"]), ("v2", ["--no-index"]))


def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def cut(g, k):
    cuts = [0] + [g.size * i // k + (7 * i) % 13 for i in range(1, k)] + [g.size]
    return [g[cuts[i]:cuts[i + 1]] for i in range(k)]


def write_files(tmp, files, prefix="g"):
    paths = []
    for i, contigs in enumerate(files):
        p = os.path.join(tmp, "%s%02d.fa" % (prefix, i))
        with open(p, "wb") as f:
            for j, c in enumerate(contigs):
                f.write(synth.fasta_bytes(c, i * 10 + j))
        paths.append(p)
    return paths


def write_list(tmp, paths):
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")


def write_collection(tmp, n, length, div=0.015, seed=55):
    """n synthetic genomes as FASTA files, targets cut into 2-3 records; one record of random bases (no match), one shorter than
    the k-mer, one target identical to G0 (loads nothing) — the shapes of test_gpu_decompress.py"""
    base = synth.base_codes(length, seed)
    gs = [synth.genome(base, i, div) for i in range(n)]
    files = [[gs[0]]] + [cut(g, 2 + i % 2) for i, g in enumerate(gs[1:], 1)]
    files[2].append(synth.genome(synth.base_codes(9000, seed + 1), 0, 0.0))          # random bases
    files[3].insert(1, gs[3][100:117].copy())                                        # shorter than the k-mer
    files[n - 2] = [gs[0].copy()]                                                    # identical to G0
    lower = np.frombuffer(b"acgt", dtype=np.uint8)
    files[1][0] = files[1][0].copy()
    files[1][0][50:90] = lower[np.arange(40) % 4]                                    # (lower case: kept, or folded under -U)
    paths = write_files(tmp, files)
    write_list(tmp, paths)
    return paths


class Full:
    """an unselected `d --fasta` of the streams under tmp: what every selection is a slice of"""

    def __init__(self, tmp, paths, extra=()):
        self.tmp, self.paths, self.extra = tmp, paths, list(extra)
        self.stdout = tool(["d"] + self.extra + ["--fasta", "full_fa", "out", "full"], tmp).stdout
        self.seq = open(os.path.join(tmp, "full.seq"), "rb").read()
        self.lens = np.fromfile(os.path.join(tmp, "full.contigLens"), dtype="<u8")
        self.counts = np.fromfile(os.path.join(tmp, "full.seqCounts"), dtype="<u4")
        assert len(self.counts) == len(paths)                                        # one entry per file of the list, -t1 or not
        self.first = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)    # file -> its first contig of the output
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        meta = _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())
        self.sequential = bool(meta["sequential"])
        # contigs of the targets (what --closure-out counts) in front of file f's: without -t1 the first file is G0, no target
        self.planned_first = self.first - (0 if self.sequential else int(self.counts[0]))
        self.planned = int(self.first[-1] - (0 if self.sequential else int(self.counts[0])))

    def expect(self, chosen):
        seq = b"".join(self.seq[self.off[self.first[f]]:self.off[self.first[f + 1]]] for f in chosen)
        lens = np.concatenate([self.lens[self.first[f]:self.first[f + 1]] for f in chosen])
        return seq, lens.astype("<u8").tobytes(), self.counts[list(chosen)].astype("<u4").tobytes()

    def planned_range(self, f):
        """file f's contigs among the targets' (none for G0's file, which is no target unless -t1 makes it one)"""
        if f == 0 and not self.sequential:
            return range(0)
        return range(int(self.planned_first[f]), int(self.planned_first[f + 1]))


def check_selection(full, chosen, select_args, variants=VARIANTS):
    """d --select under every variant: the outputs are the slices of the unselected run, --fasta writes the chosen files only"""
    tmp = full.tmp
    want = dict(zip(OUTS, full.expect(chosen)))
    names = sorted(os.path.basename(full.paths[f]) for f in chosen)
    outs = {}
    tag = "s" + "_".join(str(f) for f in chosen) + "_"                               # (the runs of a mode share a directory: every selection writes under names of its own)
    variants = [(tag + name, extra) for name, extra in variants]
    for name, extra in variants:
        outs[name] = tool(["d"] + full.extra + extra + select_args + ["--fasta", name + "_fa", "--closure-out", name + ".closure", "out", name], tmp).stdout
        for ext in OUTS:
            assert open(os.path.join(tmp, name + "." + ext), "rb").read() == want[ext], (name, ext)
        assert sorted(os.listdir(os.path.join(tmp, name + "_fa"))) == names
        for f in names:
            assert open(os.path.join(tmp, name + "_fa", f), "rb").read() == open(os.path.join(tmp, "full_fa", f), "rb").read(), (name, f)
        closure = np.fromfile(os.path.join(tmp, name + ".closure"), dtype=np.uint8)
        assert closure.size == full.planned
        for f in chosen:
            assert (closure[list(full.planned_range(f))] == 2).all()
        m = re.search(r"closure: (\d+) of (\d+) contigs, (\d+) of (\d+) bases, (\d+) selected, (\d+) dependency targets", outs[name])
        assert m, outs[name]
        assert int(m.group(1)) == int((closure != 0).sum()) and int(m.group(2)) == full.planned and int(m.group(5)) == len(chosen)
    return outs[variants[0][0]], np.fromfile(os.path.join(tmp, variants[0][0] + ".closure"), dtype=np.uint8)


# ---- 1. selected files come back
MODES = {"m1R3": (["-m", "1", "-R", "3"], []), "m0t1": (["-m", "0", "-t1"], []), "LR3": (["-L", "-R", "3"], []), "m3t1": (["-m", "3", "-t1"], ["--restore-rc"])}
N = 7


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    made = {}

    def get(mode):
        if mode not in made:
            tmp = str(tmp_path_factory.mktemp(mode))
            paths = write_collection(tmp, N, 100_000 + 2000 * N)
            tool(["c"] + MODES[mode][0] + ["list.txt", "out"], tmp)
            made[mode] = Full(tmp, paths, MODES[mode][1])
        return made[mode]
    return get


@pytest.mark.parametrize("which", ["late", "two", "g0"])
@pytest.mark.parametrize("mode", list(MODES))
def test_selected_files_come_back(runs, mode, which):
    full = runs(mode)
    if which == "late":
        check_selection(full, [N - 1], ["--select", "g%02d.fa" % (N - 1)])
    elif which == "two":
        with open(os.path.join(full.tmp, "pats.txt"), "w") as f:
            f.write("g02.fa\ng%02d.fa\n" % (N - 2))
        check_selection(full, [2, N - 2], ["--select-list", "pats.txt"])
    else:
        out, closure = check_selection(full, [0], ["--select", "/g00.fa"])
        if not full.sequential:
            assert not closure.any()                                                 # G0 is literals: nothing is filled


def test_target_identical_to_g0_depends_on_nothing(runs):
    full = runs("m1R3")
    out, closure = check_selection(full, [N - 2], ["--select", "g%02d.fa" % (N - 2)], VARIANTS[:1])
    assert "1 selected, 0 dependency targets" in out
    assert int((closure != 0).sum()) == len(full.planned_range(N - 2))


# ---- 2. the closure is tight where it is known
@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """two unrelated families, five files each, interleaved: A0 (G0), B0, A1, B1, ..., A4, B4"""
    tmp = str(tmp_path_factory.mktemp("fam"))
    files = []
    for i in range(5):
        for seed in (55, 9055):
            files.append(cut(synth.genome(synth.base_codes(100_000, seed), i, 0.015), 2))
    paths = write_files(tmp, files)
    write_list(tmp, paths)
    tool(["c", "-R", "2", "list.txt", "out"], tmp)
    return Full(tmp, paths)


def test_closure_keeps_to_the_family(families):
    full = families
    out, closure = check_selection(full, [9], ["--select", "g09.fa"], VARIANTS[:1])    # the last B file
    for f in (2, 4, 6, 8):
        assert not closure[list(full.planned_range(f))].any(), f                     # no contig of an A target
    assert (closure[list(full.planned_range(1))] == 1).all()                         # the first B file carried B into the reference
    assert (closure[list(full.planned_range(9))] == 2).all()
    out, closure = check_selection(full, [8], ["--select", "g08.fa"], VARIANTS[:1])    # the last A file: the mirror image
    for f in (1, 3, 5, 7, 9):
        assert not closure[list(full.planned_range(f))].any(), f
    assert (closure[list(full.planned_range(8))] == 2).all()


# ---- 3. a deep chain: g_i is a 1.5 % mutation of g_(i - 1)
def test_deep_chain(tmp_path):
    tmp = str(tmp_path)
    codes = [synth.base_codes(100_000, 321)]
    for i in range(1, 8):
        codes.append(synth.genome_codes(codes[-1], i, 0.015))
    gs = [synth.ACGT[c] for c in codes]
    # the drive on the CPU: the last file has matches into bytes that entered the reference with an earlier target — an input
    # where everything matches G0 would prove nothing
    o = _orc.OracleMatcher(8_000_000)
    res = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o), [gs[0]], [[g] for g in gs[1:]], 2)
    last = np.asarray(res["matches"][-1], dtype=np.uint64).reshape(-1, 3)
    g0_end = 1 + 2 * gs[0].size + 2                                                 # G0, its reverse complement, a separator
    assert (last[:, 0] > g0_end).sum() > 10
    paths = write_files(tmp, [[g] for g in gs])
    write_list(tmp, paths)
    tool(["c", "-R", "2", "list.txt", "out"], tmp)
    full = Full(tmp, paths)
    out, closure = check_selection(full, [7], ["--select", "g07.fa"])
    assert (closure[list(full.planned_range(1))] != 0).all()                         # the sweep went through every unit down to the first target
    assert int(re.search(r"(\d+) dependency targets", out).group(1)) >= 2


# ---- 4. laps: the reference buffer goes round more than once
def test_selection_from_the_last_lap(tmp_path):
    """--ref-factor 1 (a 4 MiB buffer) and the files of test_reference_buffer_wraps_at_least_twice: one contig of 2.4 Mbp fills the
    first lap, 80 files of 60 kbp the next two; every third of them is a 1 % mutation of the file two before it. The copy's
    original lies where other contigs lay a lap earlier: the wrong lap shows as foreign contigs in the closure or as wrong bytes."""
    tmp = str(tmp_path)
    paths = write_collection(tmp, 9, 120_000)
    with open(paths[1], "ab") as f:
        f.write(synth.fasta_bytes(synth.genome(synth.base_codes(2_400_000, 77), 1, 0.3), 901))
    us = []
    for i in range(80):
        u = synth.genome_codes(us[i - 2], 5000 + i, 0.01) if i % 3 == 2 else synth.base_codes(60_000, 1000 + i)
        us.append(u)
        p = os.path.join(tmp, "u%02d.fa" % i)
        with open(p, "wb") as f:
            f.write(synth.fasta_bytes(synth.ACGT[u], 2000 + i))
        paths.append(p)
    write_list(tmp, paths)
    tool(["c", "--ref-factor", "1", "-R", "2", "list.txt", "out"], tmp)
    assert _meta.parse(open(os.path.join(tmp, "out.meta"), "rb").read())["laps"] >= 2
    full = Full(tmp, paths)
    copy, original = 9 + 77, 9 + 75
    out, closure = check_selection(full, [copy], ["--select", "u77.fa"])
    marked = set(np.flatnonzero(closure).tolist())
    assert marked == set(full.planned_range(copy)) | set(full.planned_range(original)), sorted(marked)
    assert (closure[list(full.planned_range(original))] == 1).all()


# ---- 5. refusals: a message, exit 1, nothing written
def refused(tmp, extra, word):
    r = tool(["d"] + extra + ["--fasta", "no_fa", "--closure-out", "no.closure", "out", "no"], tmp, ok=False)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "mbgc-hip d: " in r.stderr and word in r.stderr, r.stderr
    for f in ("no.seq", "no.contigLens", "no.seqCounts", "no.closure", "no_fa"):
        assert not os.path.exists(os.path.join(tmp, f)), f


def test_refusals(runs, tmp_path):
    full = runs("m1R3")
    refused(full.tmp, ["--select", "no-such-file"], "matches")
    open(os.path.join(full.tmp, "empty.txt"), "w").close()
    refused(full.tmp, ["--select-list", "empty.txt"], "empty")
    tmp = str(tmp_path)
    for f in os.listdir(full.tmp):
        if f.startswith("out.") and f != "out.names":
            with open(os.path.join(tmp, f), "wb") as o:
                o.write(open(os.path.join(full.tmp, f), "rb").read())
    r = tool(["d", "--select", "g03", "out", "no"], tmp, ok=False)
    assert r.returncode == 1 and "cannot open" in r.stderr and ".names" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "no.seq"))


def test_single_fasta_streams_are_refused(tmp_path):
    tmp = str(tmp_path)
    base = synth.base_codes(110_000, 5)                                              # (the -t1 shape of test_gpu_decompress.py's -i case)
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        for i in range(9):
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                f.write(synth.fasta_bytes(c, i * 10 + j))
    tool(["c", "-i", "all.fa", "-t1", "out"], tmp)
    refused(tmp, ["--select", "all.fa"], "one FASTA file")


# ---- 6. without --select nothing changes
def test_plain_d_is_as_before(runs):
    full = runs("m1R3")
    lines = full.stdout.splitlines()
    assert len(lines) == 3
    assert re.fullmatch(r"waves: \d+ for %d targets" % (N - 1), lines[0])
    assert re.fullmatch(r"widest wave: \d+ targets", lines[1])
    assert lines[2] == "decoded: %d contigs, %d bases" % (full.lens.size, len(full.seq))
    assert "closure:" not in full.stdout
    recs = [c for p in full.paths for c in _driver.parse_fasta(p)]
    assert full.lens.tolist() == [c.size for c in recs] and full.seq == b"".join(c.tobytes() for c in recs)
    assert sorted(os.listdir(os.path.join(full.tmp, "full_fa"))) == sorted(os.path.basename(p) for p in full.paths)
