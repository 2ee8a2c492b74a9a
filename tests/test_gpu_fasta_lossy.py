"""The lossy input stage on the device (MBGC_FASTA_LOSSY, `mbgc-hip c --lossy`): the HIP parser against the restatement of
kseq_read_lossy (tests/_fasta_lossy.py) on edge cases, random damaged files and everything placed around the 4096-byte chunk
edges; the lossless rule through the new entry point; the tool on damaged collections against its own lossless run on their
normalised copies, back through `d --fasta`, and against the reference CLI where oracle/_ref is built."""
import os
import subprocess

import numpy as np
import pytest

import _fasta
import _refh
from _fasta_lossy import EDGE_LOSSY, EFASTQ, lossy_parse, normalise
from mbgc_amd import synth
from test_fasta_input import EDGE, hip_parse, same_ok
from test_fasta_lossy import damaged_fasta, through_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
CHUNK = 4096


def hip_parse2(files, upper=False, lossy=True, flags=None):
    """test_fasta_input.hip_parse through mbgc_fasta_parse_batch_dev2"""
    import torch
    from mbgc_amd import fasta
    blob = b"".join(files)
    offs = np.zeros(len(files) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(f) for f in files])
    dev = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to("cuda:0")
    out = torch.zeros(max(len(blob), 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    r = p.parse_batch_dev(dev.data_ptr(), offs, out.data_ptr(), out.numel(), upper, lossy=lossy, flags=flags)
    seq = out.cpu().numpy().tobytes()
    res = []
    for i, f in enumerate(files):
        recs = r["records"][int(r["rec_base"][i]): int(r["rec_base"][i + 1])]
        base = int(r["seq_base"][i])
        records = [(f[int(x["headerOff"]): int(x["headerOff"] + x["headerLen"])],
                    seq[base + int(x["seqOff"]): base + int(x["seqOff"] + x["seqLen"])]) for x in recs]
        res.append(dict(status=int(r["status"][i]), records=records, dna_line_len=int(r["dna_line_len"][i]),
                        seq=seq[base: int(r["seq_base"][i + 1])]))
    p.close()
    return res


def check(files, upper=False):
    for h, f in zip(hip_parse2(files, upper), files):
        o = lossy_parse(f, upper)
        assert h["status"] == o["status"], (h["status"], o["status"], f[:200])
        if o["status"] == 0:
            assert h["records"] == o["records"], f[:200]
            assert h["seq"] == o["seq"] and h["dna_line_len"] == o["dna_line_len"], f[:200]


@pytest.mark.parametrize("upper", [False, True])
def test_edge_cases(upper):
    check(list(EDGE_LOSSY), upper)
    assert [h["status"] for h in hip_parse2([b"@r\nAC\n+\nII\n", b">h\nAC\n"])] == [EFASTQ, 0]


@pytest.mark.parametrize("upper", [False, True])
def test_random_damaged_batches(upper):
    rng = np.random.default_rng(41 + upper)
    for it in range(6):
        check([damaged_fasta(rng) for _ in range(40)], upper)


def chunk_edge_files():
    files = []
    body = (b"ACGTTGCA" * 1100)
    tails = [b"\r\nACGT\n", b"\nAC\r\n", b"\r", b"A\r", b"A\r\n", b"\r\n\r\nAC\n", b"\n\r\nAC\n", b"\r\r\nAC\n", b"\n\r", b"\n\n\r\nAC\r\n",
             b"\n>g\r\n\r\nAC\n", b"\n>g\n\r", b"\n@g\n\n\r\n\nAC\n", b"\n>", b"\r\n@", b"\n+\n"]
    for off in (4094, 4095, 4096, 4097, 2 * CHUNK - 1, 2 * CHUNK):
        for t in tails:
            files.append(b">h\n" + body[: off - 3] + t)                 # the tail starts at file offset `off`
            files.append(b">h\n" + b"\n" * (off - 3) + t)               # ... behind nothing but empty lines
            files.append(b">" + b"h" * (off - 1) + t)                   # ... behind a header that runs up to it
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK):                  # a CR as a chunk's last byte at the end of the file
        files.append(b">h\n" + body[: n - 4] + b"\r")
        files.append(b">h\n" + body[: n - 5] + b"\n\r")
        files.append(b">h\n" + b"\n" * (n - 4) + b"\r")
    for junk in (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 700, 2 * CHUNK, 2 * CHUNK + 1, 2 * CHUNK + 3000):   # the first marker in the second and third chunk
        for fill in (b"x", b"\n", b"x\r\n"):
            j = (fill * junk)[:junk]
            files.append(j + b">h x\r\nACGT\r\nAC\n\r\n>g\n\r\nA\n")
            files.append(j + b"@h\n" + body[: 2 * CHUNK + 5] + b"\r\n" + body[:77] + b"\r\n")
            files.append(j)                                              # ... and none at all
            files.append(j + b">")
    for run in (CHUNK + 1, CHUNK + 500, 2 * CHUNK, 3 * CHUNK + 7):       # more than a chunk of empty lines between the header and a CR-only line
        for lead in (b">h\n", b">" + b"h" * 4000 + b"\r\n", b">h\nACGT\n>g\n", b">h\n\r\n", b">h\nA\n", b">h\nA\r\n", b">h\n\r\r\n"):
            files.append(lead + b"\n" * run + b"\r\nACGT\nAC\n")
            files.append(lead + b"\n" * run + b"\r")
    for h in (4093, 4094, 4095, 4096, 4097):                             # a header ending CR LF across the edge
        files.append(b">" + b"h" * h + b"\r\nACGT\r\nAC\r\n")
        files.append(b">h\nAC\n>" + b"g" * (h - 6) + b"\r\n\r\nAC\r\n")
        files.append(b">" + b"h" * h + b"\r")
    return files


def test_chunk_edges():
    files = chunk_edge_files()
    assert len(files) > 400
    check(files)
    check(files[::7], True)


def test_host_file_call():
    """mbgc_fasta_parse_host2 (the first file of a list goes through it)"""
    from mbgc_amd import fasta
    p = fasta.FastaParser()
    for f in EDGE_LOSSY[:2] + [b"", b"junk", b"x" * 5000 + b">h\r\n\r\nAC\r\n", b">h\nAC\n+\n"]:
        h, o = p.parse_host(f, lossy=True), lossy_parse(f)
        assert h["status"] == o["status"]
        if o["status"] == 0:
            assert h["records"] == o["records"] and h["dna_line_len"] == o["dna_line_len"] and h["seq"] == o["seq"]
        same_ok(p.parse_host(f), _fasta.oracle_parse(f))
    p.close()


def test_lossless_rule_through_the_new_entry_point():
    files = [f for f in EDGE]
    for upper in (False, True):
        old = hip_parse(files, upper)
        new = hip_parse2(files, upper, lossy=False, flags=1 if upper else 0)
        for a, b, f in zip(old, new, files):
            assert a["status"] == b["status"]
            if a["status"] == 0:
                assert a == b
            same_ok(b, _fasta.oracle_parse(f, upper))


# ---- the tool
def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def text(contigs, i, widths, eol=b"\n", marker=b">", last_eol=True):
    out = bytearray()
    for j, c in enumerate(contigs):
        out += marker + ("synth%05d damaged genome %d contig %d" % (i, i, j)).encode() + eol
        s, at, k = c.tobytes(), 0, 0
        while at < len(s):
            w = widths[k % len(widths)]
            out += s[at:at + w] + eol
            at += w
            k += 1
    return bytes(out) if last_eol else bytes(out)[: -len(eol)]


def damaged_collection():
    """8 genomes of 60 kbp in 3 contigs each, every file damaged in its own way; every file has a record longer than its longest
    line, so the lossless reader finds the same line length in the normalised copy"""
    base = synth.base_codes(60_000, 61)
    files = []
    for i in range(8):
        g = synth.genome(base, i, 0.015)
        cuts = [0, 20_000 + 13 * i, 41_000 + 7 * i, g.size]
        cs = [g[cuts[k]:cuts[k + 1]] for k in range(3)]
        if i == 0: f = text(cs, i, [80], b"\r\n")                                        # CRLF throughout
        elif i == 1: f = text(cs, i, [80, 61, 80, 100])                                  # ragged
        elif i == 2: f = b"a line of junk\r\n\nmore of it " + text(cs, i, [70])          # bytes in front of the first '>', which stands inside a line
        elif i == 3: f = text(cs, i, [80]).replace(b"A\nC", b"A\n\n\nC")                  # empty lines
        elif i == 4: f = text(cs, i, [60, 59], b"\r\n", b"@")                            # '@' records, CRLF, ragged
        elif i == 5:                                                                     # empty and CR-only lines behind a record's first line: nothing
            head, rest = text(cs, i, [80, 79]).split(b"contig 1\n")                      # (a CR that stays is held to the restatement by the parser tests:
            f = head + b"contig 1\n" + rest[:81] + b"\n\r\n\r\n" + rest[81:]              # the reference's literal coder has no symbol for one in a long record)
        elif i == 6: f = text(cs, i, [80]).replace(b"G\nT", b"G\r\nT")                    # some lines end CRLF, some LF
        else: f = text(cs, i, [90, 90, 45], last_eol=False) + b"\r"                      # no line end behind the last line, but a CR
        files.append(f)
    return files


@pytest.fixture(scope="module")
def collection(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lossy"))
    files = damaged_collection()
    norm = [normalise(f) for f in files]
    for f, n in zip(files, norm):
        assert _fasta.oracle_parse(f)["status"] != 0 or b"\r" in f
        o, p = _fasta.oracle_parse(n), lossy_parse(f)
        assert o["status"] == 0 and o["records"] == p["records"] and o["dna_line_len"] == p["dna_line_len"] > 0
    for d, group in (("raw", files), ("norm", norm)):
        os.makedirs(os.path.join(tmp, d, "in"))
        for i, f in enumerate(group):
            with open(os.path.join(tmp, d, "in", "g%02d.fa" % i), "wb") as o:
                o.write(f)
        with open(os.path.join(tmp, d, "list.txt"), "w") as o:
            o.write("".join("in/g%02d.fa\n" % i for i in range(len(group))))
    return tmp, files, norm


@pytest.mark.parametrize("args", [["-t1"], ["-R", "3"]], ids=["t1", "R3"])
def test_tool_on_damaged_files_equals_lossless_on_normalised_copies(collection, args):
    tmp, files, norm = collection
    name = "o" + args[0].strip("-")
    tool(["c", "--lossy"] + args + ["list.txt", name], os.path.join(tmp, "raw"))
    tool(["c"] + args + ["list.txt", name], os.path.join(tmp, "norm"))
    outs = sorted(f for f in os.listdir(os.path.join(tmp, "raw")) if f.startswith(name + "."))
    assert outs == sorted(f for f in os.listdir(os.path.join(tmp, "norm")) if f.startswith(name + ".")) and len(outs) >= 12
    for f in outs:
        assert open(os.path.join(tmp, "raw", f), "rb").read() == open(os.path.join(tmp, "norm", f), "rb").read(), f
    want = [lossy_parse(f)["dna_line_len"] for f in files]
    want = want[:1] + want if args == ["-t1"] else want                          # (-t1: the first contig is the reference, the first file a target too)
    assert np.fromfile(os.path.join(tmp, "raw", name + ".dnaLineLengths"), dtype="<u8").tolist() == want
    tool(["d", "--fasta", "back" + name, name, "b" + name], os.path.join(tmp, "raw"))
    for i, n in enumerate(norm):
        assert open(os.path.join(tmp, "raw", "back" + name, "g%02d.fa" % i), "rb").read() == n, i


@pytest.mark.skipif(not (_refh.available() and os.access(_refh.REF_MBGC, os.X_OK)), reason="oracle/_ref not built")
def test_reference_cli_extracts_the_same_files(collection, tmp_path):
    tmp, files, norm = collection
    back = through_reference(str(tmp_path), {"g%02d.fa" % i: f for i, f in enumerate(files)})
    for i, n in enumerate(norm):
        assert back["g%02d.fa" % i] == n, i


def test_refusals(collection, tmp_path):
    tmp, files, norm = collection
    raw = os.path.join(tmp, "raw")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nACGT\n+\nIIII\n")
    (tmp_path / "l.txt").write_text("%s\n%s\n%s\n" % (os.path.join(raw, "in", "g00.fa"), os.path.join(raw, "in", "g01.fa"), fq))
    r = tool(["c", "--lossy", "-R", "2", "l.txt", "o"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "FASTQ input is not supported" in r.stderr and "reads.fq" in r.stderr, r.stderr
    r = tool(["c", "--lossy", "-i", os.path.join(raw, "in", "g01.fa"), "o"], str(tmp_path), ok=False)
    assert r.returncode != 0 and "--lossy" in r.stderr and "-i" in r.stderr, r.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]
    r = tool(["c", "-R", "3", "list.txt", "refused"], raw, ok=False)               # the same list without --lossy: as before, with the hint
    assert r.returncode != 0 and "inconsistent line length" in r.stderr and "Consider the lossy mode (--lossy)." in r.stderr, r.stderr
