"""The corpus of the gzip deflate (mbgc_fasta_deflate_dev, mbgc_amd/csrc/fasta_deflate.h), generated from seeds: nothing large is
committed. calls() -> [(name, buffer, [(inOff, inLen)], [class bar per job])]: one deflate call each. The bars are computed here with
Python's zlib, never from the code under test:
  HUFFMAN   DNA and protein FASTA: size <= 1.02 x zlib's Z_HUFFMAN_ONLY gzip of the same text + 16 bytes per chunk (the two encoders
            differ in block boundaries, tree headers and flush blocks only; chunking at 32 KiB costs zlib itself 0.1 %)
  RUN       a run of one byte, with or without line ends: size <= a tenth of the text (a 61-byte line as one literal and one match
            is at most 48 bits under any legal code lengths; Huffman alone gives 0.128: no bar without a working matcher)
  RANDOM    size <= the text + 10 per chunk + 18
  REPEATS   header lines that repeat: size <= the Z_HUFFMAN_ONLY size (matches must not make it worse)
  BOUND     nothing beyond mbgc_fasta_deflate_bound (which holds for every class)"""
import functools
import random
import struct
import zlib

CHUNK = 32768
HUFFMAN, RUN, RANDOM, REPEATS, BOUND = "huffman", "run", "random", "repeats", "bound"


def chunks_of(n):
    return max(1, -(-n // CHUNK))


def bound(n):
    return 18 + chunks_of(n) * 10 + n


def huffman_only(text, flush_every=None):
    """the size of zlib's Z_HUFFMAN_ONLY gzip file of the text; flush_every: with a full flush after every that many bytes"""
    z = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_HUFFMAN_ONLY)
    if not flush_every:
        return len(z.compress(text) + z.flush())
    size = 0
    for at in range(0, len(text), flush_every):
        size += len(z.compress(text[at: at + flush_every]))
        if at + flush_every < len(text):
            size += len(z.flush(zlib.Z_FULL_FLUSH))
    return size + len(z.flush())


def limit(kind, text):
    """the most bytes the gzip file of this text may take under its class bar (the bound holds besides)"""
    n = len(text)
    if kind == HUFFMAN:
        return int(1.02 * huffman_only(text)) + 16 * chunks_of(n)
    if kind == RUN:
        return n // 10
    if kind == RANDOM:
        return n + 10 * chunks_of(n) + 18
    if kind == REPEATS:
        return huffman_only(text)
    return bound(n)


def fasta(header, seq, cols=60):
    return b">" + header + b"\n" + b"".join(seq[i: i + cols] + b"\n" for i in range(0, len(seq), cols))


def dna_fasta(nbytes, seed):
    """exactly nbytes of 60-column random-ACGT FASTA (the last line is cut where the size says)"""
    r = random.Random(seed)
    t = fasta(b"contig_%d random ACGT" % seed, bytes(r.choice(b"ACGT") for _ in range(nbytes)))
    return t[:nbytes]


def soft_masked(seed):
    r = random.Random(seed)
    seq = bytearray()
    while len(seq) < 90_000:
        seq += bytes(r.choice(b"ACGT") for _ in range(r.randrange(200, 3000)))
        seq += bytes(r.choice(b"acgt") for _ in range(r.randrange(50, 1500)))
    return fasta(b"chr_soft_masked", bytes(seq[:90_000]))


def header_repeats(seed):
    r = random.Random(seed)
    return b"".join(fasta(b"NZ_JAAAAA01%05d.1 Listeria monocytogenes FDA00012345 contig, whole genome shotgun sequence" % k,
                          bytes(r.choice(b"ACGT") for _ in range(300))) for k in range(1, 401))


def fibonacci_text():
    counts = [1, 1]
    while len(counts) < 21:
        counts.append(counts[-1] + counts[-2])
    assert counts[-1] == 10946 and sum(counts) == 28656
    syms = b"ACGTNRYKMSWBDHVacgtn\n>"[:21]
    body = bytearray()
    for s, c in zip(syms, counts):
        body += bytes([s]) * c
    random.Random(5).shuffle(body)
    return bytes(body) + bytes([syms[20]]) * (CHUNK - len(body))


def protein(seed):
    r = random.Random(seed)
    letters, weights = b"ACDEFGHIKLMNPQRSTVWYBZXUO", [8, 1, 5, 7, 4, 7, 2, 6, 6, 10, 2, 4, 5, 4, 5, 7, 5, 7, 1, 3, 1, 1, 1, 1, 1]
    return b"".join(fasta(b"sp|P%05d|PROT_%d some protein OS=Listeria" % (k, k), bytes(r.choices(letters, weights, k=r.randrange(80, 900)))) for k in range(120))


@functools.lru_cache(maxsize=None)
def singles():
    """[(name, text, class)]"""
    rows = [("empty", b"", BOUND), ("one_byte", b"A", BOUND)]
    for name, n in (("chunk_minus_1", CHUNK - 1), ("chunk", CHUNK), ("chunk_plus_1", CHUNK + 1), ("two_chunks_plus_1", 2 * CHUNK + 1)):
        rows.append(("dna_" + name, dna_fasta(n, n), HUFFMAN))
    rows.append(("one_value_70000", b"T" * 70_000, RUN))
    rows.append(("n_run_100000", fasta(b"scaffold_of_N", b"N" * 100_000), RUN))
    rows.append(("soft_masked", soft_masked(3), HUFFMAN))
    rows.append(("header_repeats", header_repeats(4), REPEATS))
    rows.append(("random_70000", random.Random(6).randbytes(70_000), RANDOM))
    rows.append(("fibonacci_21", fibonacci_text(), BOUND))
    rows.append(("protein", protein(7), HUFFMAN))
    assert all(len(t) <= 160_000 for _, t, _ in rows)                       # (the largest: 400 records of 300 bases under their headers)
    return rows


@functools.lru_cache(maxsize=None)
def calls():
    """every single text as a call of one job, the text between guard bytes; then three jobs in one call, at offsets 1, 7 and 13
    modulo 16 -> [(name, buffer, [(inOff, inLen)], [class])]"""
    out = []
    for k, (name, text, kind) in enumerate(singles()):
        lead = 16 + (k * 5) % 16
        out.append((name, b"\xa5" * lead + text + b"\xa5" * 16, [(lead, len(text))], [kind]))
    by = {n: (t, c) for n, t, c in singles()}
    parts, jobs, kinds, at = [], [], [], 0
    for name, mod in (("dna_chunk_plus_1", 1), ("n_run_100000", 7), ("protein", 13)):
        text, kind = by[name]
        pad = (mod - at) % 16 + 16
        parts.append(b"\x5a" * pad)
        at += pad
        assert at % 16 == mod
        jobs.append((at, len(text)))
        kinds.append(kind)
        parts.append(text)
        at += len(text)
    parts.append(b"\x5a" * 16)
    out.append(("three_jobs", b"".join(parts), jobs, kinds))
    return out


THREE_JOBS = ("dna_chunk_plus_1", "n_run_100000", "protein")          # the singles that three_jobs holds, in its order


def write_corpus(path):
    """u32 calls; per call: u32 name length, u64 buffer length, u32 jobs, the name, the buffer, the jobs as (u64 inOff, u64 inLen)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(calls())))
        for name, buf, jobs, _ in calls():
            f.write(struct.pack("<IQI", len(name), len(buf), len(jobs)) + name.encode() + buf)
            for off, n in jobs:
                f.write(struct.pack("<QQ", off, n))


def read_outputs(path):
    """what tests/fasta_deflate_emu.cpp writes: per call u64 bytes and the gzip files back to back -> {name: bytes}"""
    out, blob, at = {}, open(path, "rb").read(), 0
    for name, _, _, _ in calls():
        n, = struct.unpack_from("<Q", blob, at)
        out[name] = blob[at + 8: at + 8 + n]
        at += 8 + n
    assert at == len(blob)
    return out
