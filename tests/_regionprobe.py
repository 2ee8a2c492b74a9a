"""What the tests of `mbgc-hip d --region` share. The probe side: mbgc_decoder_region_probe (mbgc_amd/host/mbgc_decoder.cpp) through
ctypes, its bitmaps unpacked, and `check` — the device's closure against the host's and the masked fill against the unselected
decode. The tool side: `Full`, the unselected `d` of a stream set that every piece is a cut of, and `run_regions`, which holds
`d --region` to the Python cut of it. And the collections on which the closure has work to do (rc-chain, many-records, wrap), each
compressed once per session and shared by the files that ask for it."""
import ctypes as C
import os
import subprocess

import numpy as np

from mbgc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbgc_amd", "mbgc-hip")
OUTS = ("seq", "contigLens", "seqCounts")
WIDTH = 70
SENTINEL = 0xEE
PROBE_OUT = (("granBase", "<u8"), ("needDev", "<u4"), ("needHost", "<u4"), ("contigDev", "<u4"), ("contigHost", "<u4"), ("filled", "<u8"), ("seqOff", "<u8"),
             ("contigLen", "<u8"), ("recBase", "<u8"), ("recDest", "<u8"), ("masked", np.uint8))


def tool(args, cwd, ok=True):
    r = subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def fasta(header, seq):
    return b">" + header + b"\n" + b"".join(seq[i:i + WIDTH] + b"\n" for i in range(0, len(seq), WIDTH))


# ---- the probe
def host_lib():
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    L.mbgc_decoder_region_probe.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint64]
    return L


def probe(host, tmp, prefix, pieces, granule, name, serial=0, restore_rc=0):
    arr = np.ascontiguousarray(np.asarray(pieces, dtype=np.uint64).reshape(-1, 3))
    err = C.create_string_buffer(512)
    out = os.path.join(tmp, name)
    r = host.mbgc_decoder_region_probe(os.path.join(tmp, prefix).encode(), restore_rc, serial, arr.ctypes.data_as(C.POINTER(C.c_uint64)), len(arr), granule, out.encode(), err, 512)
    assert r == 0, err.value
    rd = lambda ext, dt: np.fromfile(out + "." + ext, dtype=dt)
    return {k: rd(k, dt) for k, dt in PROBE_OUT}


def bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def check(p, full_seq, pieces, granule):
    """device == host; every byte a needed record writes is the unmasked fill's; every other byte of the buffer kept the sentinel"""
    assert np.array_equal(p["needDev"], p["needHost"]) and np.array_equal(p["contigDev"], p["contigHost"])
    assert p["filled"][0] == p["filled"][1]
    lens, off = p["contigLen"], p["seqOff"]
    g0n = lens.size - (p["granBase"].size - 1)
    full_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    full = np.frombuffer(full_seq, dtype=np.uint8)
    if full.size != full_off[-1]:                                  # (-t1, -m 3, -i: the first file is a target as well, the unselected run writes the planned contigs only)
        assert full.size == full_off[-1] - full_off[g0n]
        full_off -= full_off[g0n]
    need = bits(p["needDev"], int(p["granBase"][-1]))
    contig = bits(p["contigDev"], lens.size - g0n)
    for c, a, n in pieces:                                         # what went in is in
        if c >= g0n:
            assert need[int(p["granBase"][c - g0n]) + a // granule] and need[int(p["granBase"][c - g0n]) + (a + n - 1) // granule] and contig[c - g0n]
    filled = 0
    for k in range(lens.size - g0n):
        n = int(lens[g0n + k])
        got = p["masked"][int(off[g0n + k]):int(off[g0n + k + 1])]
        if not contig[k]:
            assert got.size == 0                                   # no place in the buffer
            continue
        assert got.size == n
        gneed = need[int(p["granBase"][k]):int(p["granBase"][k + 1])]
        dest = np.append(p["recDest"][int(p["recBase"][k]):int(p["recBase"][k + 1])], n).astype(np.int64)
        touched = np.zeros(n, dtype=bool)
        for a, b in zip(dest[:-1], dest[1:]):
            if b > a and gneed[a // granule:(b - 1) // granule + 1].any():
                touched[a:b] = True
        assert touched[np.repeat(gneed, granule)[:n]].all()        # a needed granule is written whole
        want = full[full_off[g0n + k]:full_off[g0n + k + 1]]
        assert np.array_equal(got[touched], want[touched]), k
        assert (got[~touched] == SENTINEL).all(), k
        filled += int(touched.sum())
    assert filled == p["filled"][0]
    return need, contig, filled


# ---- the tool against the Python cut of the unselected run
class Full:
    """the unselected run: what every piece is a cut of. headers: per file, per record"""

    def __init__(self, tmp, extra=(), prefix="out", one_file=False, *, headers):
        self.tmp, self.extra, self.prefix, self.one_file = tmp, list(extra), prefix, one_file
        self.stdout = tool(["d"] + self.extra + [prefix, prefix + "_full"], tmp).stdout
        self.seq = open(os.path.join(tmp, prefix + "_full.seq"), "rb").read()
        self.lens = np.fromfile(os.path.join(tmp, prefix + "_full.contigLens"), dtype="<u8")
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.headers = [h for hs in headers for h in hs]
        self.file_of = [i for i, hs in enumerate(headers) for _ in hs]
        assert self.lens.size == len(self.headers)

    def cut(self, specs, files=None):
        """specs: [(pattern, FROM, TO)] -> (pieces [(record, from0, len)], skipped)"""
        pieces, skipped = set(), 0
        for pat, a, b in specs:
            for r, h in enumerate(self.headers):
                if pat in h and (files is None or self.file_of[r] in files):
                    if a > self.lens[r]:
                        skipped += 1
                    else:
                        pieces.add((r, a - 1, min(b, int(self.lens[r])) - a + 1))
        return sorted(pieces), skipped


def expect(full, pieces):
    seq = b"".join(full.seq[full.off[r] + a:full.off[r] + a + n] for r, a, n in pieces)
    lens = np.asarray([n for _, _, n in pieces], dtype="<u8").tobytes()
    per_file = {}
    for r, _, _ in pieces:
        f = 0 if full.one_file else full.file_of[r]
        per_file[f] = per_file.get(f, 0) + 1
    return seq, lens, np.asarray([per_file[f] for f in sorted(per_file)], dtype="<u4").tobytes()


def args_of(specs):
    return sum((["--region", "%s:%d-%d" % (p.decode(), a, b)] for p, a, b in specs), [])


def run_regions(full, specs, name, extra=(), files=None, fasta_args=None, region_args=None):
    """region_args: how the specs reach the tool when not as one --region each (a --region-list the caller wrote)"""
    pieces, skipped = full.cut(specs, files)
    sink = (["--fasta", name + "_fa"] + list(fasta_args)) if fasta_args is not None else []
    out = tool(["d"] + full.extra + list(extra) + (args_of(specs) if region_args is None else list(region_args)) + sink + [full.prefix, name], full.tmp).stdout
    for ext, want in zip(OUTS, expect(full, pieces)):
        assert open(os.path.join(full.tmp, name + "." + ext), "rb").read() == want, (name, ext)
    records = len({r for r, _, _ in pieces})
    assert "regions: %d pieces of %d records, %d bases, %d out of range\n" % (len(pieces), records, sum(n for _, _, n in pieces), skipped) in out, out
    return out, pieces


def piece_text(full, r, a, n):
    h = full.headers[r]
    word = h.split()[0]
    hdr = word + b":%d-%d" % (a + 1, a + n) + h[len(word):]
    return fasta(hdr, full.seq[full.off[r] + a:full.off[r] + a + n])


# ---- the collections on which the closure has work to do
def rc_codes(codes):
    return (3 - codes[::-1]).astype(np.uint8)


def write_files(tmp, headers, seqs, stem):
    """one FASTA file per entry of headers / seqs, list.txt over them and all.fa, their concatenation"""
    paths = []
    for i, (hs, ss) in enumerate(zip(headers, seqs)):
        paths.append(os.path.join(tmp, "%s%02d.fa" % (stem, i)))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(fasta(h, s) for h, s in zip(hs, ss)))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    with open(os.path.join(tmp, "all.fa"), "wb") as f:
        f.write(b"".join(open(p, "rb").read() for p in paths))
    return paths


RC_LINKS, RC_LEN = 7, 64 << 10


def rc_chain_headers():
    return [[b"link%d of the rc chain" % i] for i in range(RC_LINKS)]


def write_rc_chain(tmp, divergence=0.03):
    """7 files of one 64 KiB contig: link i is a mutation of link i - 1 as it stands in its file, and every odd link is then
    reverse-complemented, so a link reads reversed rows of the link two before it (`c -R 2` pairs the targets, and a round sees
    only the rounds before it). The divergence per link is 3 %: at 1.5 % a 16 KiB request in the last link marks 2 earlier links
    of the plain set (links 4 and 2), at 3 % enough matches fall through to older links for it to mark 3 (links 4, 3, 2), and 5
    of the `-i` set"""
    codes = [synth.base_codes(RC_LEN, 9091)]
    for i in range(1, RC_LINKS):
        c = synth.genome_codes(codes[-1], 40 + i, divergence)
        codes.append(rc_codes(c) if i & 1 else c)
    return write_files(tmp, rc_chain_headers(), [[synth.ACGT[c].tobytes()] for c in codes], "r")


MANY = 200
MANY_SHORT = (15, 16, 17, 255, 256, 257)


def many_lengths():
    """the first file's record lengths: every fourth from the granule's edges, the others from 40..700"""
    rng = np.random.default_rng(2024)
    return [MANY_SHORT[(i // 4) % 6] if i % 4 == 0 else int(rng.integers(40, 701)) for i in range(MANY)]


def many_headers():
    return [[b"seed unrelated head of the list"], [b"a%03d len %d" % (i, n) for i, n in enumerate(many_lengths())], [b"b%03d cut of a" % i for i in range(MANY)]]


def write_many_records(tmp):
    """a%03d: 200 unrelated records of the lengths above; b%03d: 200 records of 600 to 5000 bases, each a window of the a records
    laid end to end, mutated 1 %, every fifth reverse-complemented — a window lies over many a records, so what a b record
    reads lies over as many provenance rows with the separators between them. A list's first file is the initial reference, which
    belongs to nobody and has no granules: a short unrelated file stands there, so that both files are planned."""
    rng = np.random.default_rng(2025)
    lens = many_lengths()
    a = [synth.base_codes(n, 7000 + i) for i, n in enumerate(lens)]
    cat = np.concatenate(a)
    b = []
    for i in range(MANY):
        n = int(rng.integers(600, 5001))
        at = int(rng.integers(0, cat.size - n))
        c = synth.genome_codes(cat[at:at + n], 300 + i, 0.01)
        b.append(rc_codes(c) if i % 5 == 4 else c)
    seqs = [[synth.ACGT[synth.base_codes(4096, 6999)].tobytes()], [synth.ACGT[c].tobytes() for c in a], [synth.ACGT[c].tobytes() for c in b]]
    return write_files(tmp, many_headers(), seqs, "m")


WRAP_FILES = 82


def wrap_headers():
    return [[b"wrap%02d of the wrapped set" % i] for i in range(WRAP_FILES)]


def write_wrap(tmp):
    """the sequences of test_gpu_decode_region_closure.py's wrapped set (for `c --ref-factor 1`, a 4 MiB buffer): a 2.4 Mbp contig
    fills the first lap, 80 files of 60 kbp the next two; every third is a 1 % mutation of the file two before it — of its reverse
    complement for every sixth. Contig 2 + i of the collection is file i of the 80."""
    us = []
    seqs = [[synth.ACGT[synth.base_codes(50_000, 5)].tobytes()], [synth.ACGT[synth.base_codes(2_400_000, 77)].tobytes()]]
    for i in range(80):
        if i % 3 == 2:
            u = synth.genome_codes(us[i - 2], 5000 + i, 0.01)
            if i % 6 == 5:
                u = rc_codes(u)
        else:
            u = synth.base_codes(60_000, 1000 + i)
        us.append(u)
        seqs.append([synth.ACGT[u].tobytes()])
    return write_files(tmp, wrap_headers(), seqs, "w")


class StreamSet:
    """a stream set on disk with its unselected decode: tmp / prefix, how `d` and the probe must be called for it, the header table"""

    def __init__(self, tmp, prefix, headers, d_extra=(), restore_rc=0, one_file=False):
        self.tmp, self.prefix, self.headers, self.d_extra, self.restore_rc, self.one_file = tmp, prefix, headers, list(d_extra), restore_rc, one_file
        self.full = Full(tmp, self.d_extra, prefix, one_file, headers=headers)

    def probe(self, host, pieces, granule, name="p"):
        return probe(host, self.tmp, self.prefix, pieces, granule, "%s_%s" % (self.prefix, name), restore_rc=self.restore_rc)


_SETS = {}
VARIANTS = {"rc-chain": ("rc", ["-R", "2"], "list"), "rc-chain-t1": ("rc", ["-R", "2", "-t1"], "list"), "rc-chain-m3": ("rc", ["-R", "2", "-m", "3"], "list"),
            "rc-chain-i": ("rc", ["-R", "2"], "one"), "many-records": ("many", ["-R", "1"], "list"), "wrap": ("wrap", ["--ref-factor", "1", "-R", "2"], "list")}
_WRITERS = {"rc": (write_rc_chain, rc_chain_headers), "many": (write_many_records, many_headers), "wrap": (write_wrap, wrap_headers)}


def stream_set(tmp_path_factory, name):
    """the named set, written and compressed with the variant's options on first use. many-records goes in rounds of one target: the
    targets of a round are matched against what the rounds before it loaded, and the b records are there to copy the a records"""
    if name not in _SETS:
        files, c_args, how = VARIANTS[name]
        if ("files", files) not in _SETS:
            tmp = str(tmp_path_factory.mktemp("region_" + files))
            _WRITERS[files][0](tmp)
            _SETS[("files", files)] = tmp
        tmp = _SETS[("files", files)]
        prefix = name.replace("-", "_")
        tool(["c"] + c_args + (["-i", "all.fa"] if how == "one" else ["list.txt"]) + [prefix], tmp)
        _SETS[name] = StreamSet(tmp, prefix, _WRITERS[files][1](), ["--restore-rc"] if "-m" in c_args else [], 1 if "-m" in c_args else 0, how == "one")
    return _SETS[name]
