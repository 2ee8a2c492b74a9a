"""`mbgc-hip r`: chosen files of a stream set repacked into a new one without a base leaving the device. The acceptance oracle is the
route the command replaces: F = the files `mbgc-hip d [input side] --fasta dir in tmp` writes, in its order; every file `r [input
side] [output side] in out` writes, except .names, equals what `mbgc-hip c [output side] list(F) ref` writes, and out.names holds
the chosen units' own lines of in.names (the first one twice where c writes it twice). `c` is held to the oracle and the reference
elsewhere, so this holds `r`."""
import os
import subprocess

import numpy as np
import pytest

from mbgc_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
N = 8
CHOSEN = [1, 3, 5]                                                                   # not neighbours, and not the original G0
SELECT = ["--select", "g01.fa", "--select", "g03.fa", "--select", "g05.fa"]
STREAMS = ("literals", "locksPos", "gapDelta", "flags", "mapOff", "mapOff5th", "mapLen", "refExtSize", "meta", "headers", "dnaLineLengths")


def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def cut(g, k):
    cuts = [0] + [g.size * i // k + (7 * i) % 13 for i in range(1, k)] + [g.size]
    return [g[cuts[i]:cuts[i + 1]] for i in range(k)]


def write_collection(tmp, n=N, length=60_000, div=0.015, seed=55):
    """n synthetic genomes as FASTA files (the shapes of test_gpu_decompress_select.py): targets cut into 2-3 records, one record of
    random bases, one shorter than the k-mer, one target identical to G0, a lower-case stretch — and an insert of 8000 random bases
    that file 4 brings and file 5 carries too, so that file 5 has matches into what file 4 put into the reference"""
    base = synth.base_codes(length, seed)
    gs = [synth.genome(base, i, div) for i in range(n)]
    insert = synth.base_codes(8000, seed + 7)
    for i in (4, 5):
        gs[i] = np.concatenate([gs[i][:20_000], synth.genome(insert, i, div), gs[i][20_000:]])
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


def rewrap(path, width):
    """the FASTA file with every sequence in lines of `width` bases (0: one line), as d --fasta breaks them"""
    out, seq = [], []

    def flush():
        s = b"".join(seq)
        if s:
            w = width if width else len(s)
            out.extend(s[i:i + w] + b"\n" for i in range(0, len(s), w))
        seq.clear()
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            flush()
            out.append(line + b"\n")
        else:
            seq.append(line)
    flush()
    with open(path, "wb") as f:
        f.write(b"".join(out))


class Sets:
    """the collection, its input stream sets (made when first asked for) and the `d --fasta` runs over them"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.paths = write_collection(tmp)
        self.made, self.decoded, self.tags = set(), {}, 0

    def input_set(self, name, c_args):
        if name not in self.made:
            tool(["c"] + c_args + ["list.txt", name], self.tmp)
            self.made.add(name)
        return name

    def tag(self):
        self.tags += 1
        return "t%02d" % self.tags

    def fasta(self, in_prefix, in_args):
        """d [in_args] --fasta: (the directory, the files written in d's order = the chosen files in collection order)"""
        key = (in_prefix, tuple(in_args))
        if key not in self.decoded:
            d = self.tag() + "_fa"
            tool(["d"] + in_args + ["--fasta", d, in_prefix, d + "_out"], self.tmp)
            written = set(os.listdir(os.path.join(self.tmp, d)))
            order = [os.path.basename(p) for p in self.paths if os.path.basename(p) in written]
            assert len(order) == len(written)
            self.decoded[key] = (d, order)
        return self.decoded[key]

    def check(self, in_prefix, in_args, out_args, width=None, extra_in=()):
        """r against c over the files of d --fasta; extra_in: input-side options that change how r decodes, not what F is"""
        tmp, t = self.tmp, self.tag()
        d, order = self.fasta(in_prefix, in_args)
        fdir = d
        if width is not None:                                                        # -l N: c sees the files wrapped to N by the test
            fdir = t + "_wrapped"
            os.mkdir(os.path.join(tmp, fdir))
            for f in order:
                with open(os.path.join(tmp, fdir, f), "wb") as o:
                    o.write(open(os.path.join(tmp, d, f), "rb").read())
                rewrap(os.path.join(tmp, fdir, f), width)
        with open(os.path.join(tmp, t + "_list.txt"), "w") as f:
            f.write("".join(os.path.join(tmp, fdir, x) + "\n" for x in order))
        ref = tool(["c"] + out_args + [t + "_list.txt", t + "_ref"], tmp, ok=False)
        got = tool(["r"] + in_args + list(extra_in) + out_args + ([] if width is None else ["-l", str(width)]) + [in_prefix, t + "_out"], tmp, ok=False)
        assert got.returncode == ref.returncode, (ref.stderr, got.stderr)
        ref_files = sorted(f[len(t) + 5:] for f in os.listdir(tmp) if f.startswith(t + "_ref."))
        out_files = sorted(f[len(t) + 5:] for f in os.listdir(tmp) if f.startswith(t + "_out."))
        assert ref_files == out_files, (ref_files, out_files)
        if ref.returncode:                                                           # (the same message for the same cause)
            assert ref.stderr.strip().splitlines()[-1] == got.stderr.strip().splitlines()[-1]
            return t + "_out", order
        for ext in out_files:
            if ext != "names":
                assert open(os.path.join(tmp, t + "_out." + ext), "rb").read() == open(os.path.join(tmp, t + "_ref." + ext), "rb").read(), (ext, out_args)
        assert set(STREAMS) < set(out_files)
        by_name = {os.path.basename(p): p for p in self.paths}
        names = [by_name[x] for x in order]
        ref_names = open(os.path.join(tmp, t + "_ref.names")).read().splitlines()
        if len(ref_names) == len(names) + 1:                                         # -t1 / -m 3 / one file: the first file is G0's and target 0's
            names.insert(0, names[0])
        assert open(os.path.join(tmp, t + "_out.names")).read().splitlines() == names
        assert [os.path.basename(x) for x in ref_names] == [os.path.basename(x) for x in names]
        if width is not None:
            lens = np.fromfile(os.path.join(tmp, t + "_out.dnaLineLengths"), dtype="<u8")
            assert lens.size == len(names) and (lens == width).all()
        return t + "_out", order


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return Sets(str(tmp_path_factory.mktemp("repack")))


ROUNDS = ("in", ["-R", "2"])                                                         # targets (1, 2), (3, 4), (5, 6), (7)


# ---- 1. identity
def test_identity(sets):
    tmp = sets.tmp
    src = sets.input_set("ident", [])
    tool(["r", src, "ident_out"], tmp)
    exts = sorted(f[6:] for f in os.listdir(tmp) if f.startswith("ident."))
    assert set(STREAMS) | {"names"} <= set(exts)
    assert exts == sorted(f[10:] for f in os.listdir(tmp) if f.startswith("ident_out."))
    for ext in exts:
        assert open(os.path.join(tmp, "ident_out." + ext), "rb").read() == open(os.path.join(tmp, "ident." + ext), "rb").read(), ext


# ---- 2. a selection whose closure is larger than itself
def test_selection_depends_on_files_left_out(sets):
    src = sets.input_set(*ROUNDS)
    tool(["d"] + SELECT + ["--closure-out", "sel.closure", src, "sel"], sets.tmp)
    closure = np.fromfile(os.path.join(sets.tmp, "sel.closure"), dtype=np.uint8)
    assert (closure == 2).sum() > 0 and (closure == 1).sum() > 0                     # contigs of files that were not chosen are decoded


@pytest.mark.parametrize("extra", [[], ["--serial"], ["--no-index"]], ids=["default", "serial", "noindex"])
def test_selection(sets, extra):
    src = sets.input_set(*ROUNDS)
    out, order = sets.check(src, SELECT, [], extra_in=extra)
    assert order == ["g01.fa", "g03.fa", "g05.fa"]


# ---- 3. changed parameters
@pytest.mark.parametrize("out_args", [["-m", "0"], ["-m", "2"], ["-m", "3"], ["-t1"], ["-k", "24"], ["-s", "15"], ["-R", "2"]],
                         ids=["m0", "m2", "m3", "t1", "k24", "s15", "R2"])
def test_output_parameters(sets, out_args):
    src = sets.input_set(*ROUNDS)
    out, _ = sets.check(src, SELECT, out_args)
    if out_args == ["-m", "3"]:
        for ext in ("rcMapOff", "rcMapLen"):
            assert os.path.exists(os.path.join(sets.tmp, out + "." + ext))          # (compared with c's by check)


def test_input_set_of_t1(sets):
    sets.check(sets.input_set("int1", ["-t1"]), SELECT, [])


def test_input_set_of_m3(sets):
    src = sets.input_set("inm3", ["-m", "3"])
    sets.check(src, ["--restore-rc"] + SELECT, [])
    r = tool(["r"] + SELECT + [src, "m3no"], sets.tmp, ok=False)
    assert r.returncode == 1 and "--restore-rc" in r.stderr
    assert not [f for f in os.listdir(sets.tmp) if f.startswith("m3no.")]


# ---- 4. -U and -l
def test_uppercase(sets):
    src = sets.input_set(*ROUNDS)
    select = ["--select", "g01.fa", "--select", "g02.fa", "--select", "g04.fa"]
    out, _ = sets.check(src, select, ["-U"])
    text = open(os.path.join(sets.tmp, sets.fasta(src, select)[0], "g01.fa"), "rb").read()
    assert b"acgtacgt" in text                                                       # the chosen files do hold lower-case bases
    assert b"acgtacgt" not in open(os.path.join(sets.tmp, out + ".literals"), "rb").read()


@pytest.mark.parametrize("schedule", [[], ["-t1"]], ids=["rounds", "t1"])
@pytest.mark.parametrize("width", [70, 0])
def test_line_length(sets, width, schedule):
    sets.check(sets.input_set(*ROUNDS), [], schedule, width=width)


# ---- 5. round trip
def test_round_trip(sets):
    tmp = sets.tmp
    src = sets.input_set(*ROUNDS)
    d, order = sets.fasta(src, SELECT)
    tool(["r"] + SELECT + ["--verify", src, "rt"], tmp)
    tool(["d", "--fasta", "rt_fa", "rt", "rt_seq"], tmp)
    assert sorted(os.listdir(os.path.join(tmp, "rt_fa"))) == sorted(order)
    for f in order:
        assert open(os.path.join(tmp, "rt_fa", f), "rb").read() == open(os.path.join(tmp, d, f), "rb").read(), f
        assert open(os.path.join(tmp, "rt_fa", f), "rb").read() == open(os.path.join(tmp, f), "rb").read(), f      # ... which are the files compressed
    r = tool(["v", "--flat", "--root", d, "rt"], tmp)
    assert "correctly decoded 3 out of 3 files" in r.stdout


# ---- 6. one file
def test_one_file(sets):
    out, order = sets.check(sets.input_set(*ROUNDS), ["--select", "g03.fa"], [])
    assert order == ["g03.fa"]


# ---- 7. refusals: one line, exit status 1, nothing under the output prefix
def refused(tmp, args, word):
    r = tool(["r"] + args, tmp, ok=False)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (args, r.stderr)
    assert not [f for f in os.listdir(tmp) if f.startswith("no.")], args


def test_refusals(sets, tmp_path):
    tmp = sets.tmp
    src = sets.input_set(*ROUNDS)
    refused(tmp, ["--select", "no-such-file", src, "no"], "no file of the collection matches")
    refused(tmp, [src, src], "the output prefix is the input prefix")
    refused(tmp, ["--gpus", "2", src, "no"], "--gpus")
    refused(tmp, ["-i", "g00.fa", "no"], "-i is an option of mbgc-hip c")
    refused(tmp, ["--lossy", src, "no"], "--lossy")
    refused(tmp, ["--inflate", "device", src, "no"], "--inflate")
    refused(tmp, ["--backend", "coders.so", src, "no"], "--backend")
    one = str(tmp_path)
    base = synth.base_codes(110_000, 5)                                              # (the -i shape of test_gpu_decompress_select.py)
    with open(os.path.join(one, "all.fa"), "wb") as f:
        for i in range(9):
            for j, c in enumerate(cut(synth.genome(base, i, 0.015), 2 + i % 2)):
                f.write(synth.fasta_bytes(c, i * 10 + j))
    tool(["c", "-i", "all.fa", "-t1", "single"], one)
    refused(one, ["single", "no"], "one FASTA file")
