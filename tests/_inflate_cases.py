"""The corpus of the inflate tests (tests/test_inflate_kernel_cpu.py on the CPU, tests/test_gpu_inflate.py on the device): gzip streams
from Python's zlib, and — for what zlib will not produce on request — streams written bit by bit here. The expected bytes of every
stream, also of the hand-written ones, are what zlib inflates it to; a stream meant to fail is one zlib refuses."""
import functools
import random
import struct
import zlib

OK, ESHORT, EDATA, ECHECK = 0, 1, 2, 3
NOT_OK = -1                          # "anything but OK"


def ref_inflate(gz):
    """every member of gz, by zlib; raises zlib.error where zlib refuses"""
    out, rest = [], gz
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        if not d.eof:
            raise zlib.error("input ends early")
        rest = d.unused_data
    return b"".join(out)


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    return c.compress(data) + c.flush()


def member(deflate, data, flags=0, extra=b"", name=b"", comment=b""):
    """a gzip member around a raw DEFLATE stream that inflates to data"""
    h = b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\xff"
    if flags & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h + deflate + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                 # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):                 # a Huffman code: most significant bit first
        for k in range(nbits - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """lengths -> {symbol: (code, length)}; no check that the set is a prefix code"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def _len_code(length):
    if length == 258:
        return 285, 0, 0
    c = length - 3
    if c < 8:
        return 257 + c, 0, 0
    eb = c.bit_length() - 3
    return 257 + 4 * (eb + 1) + ((c >> eb) & 3), eb, c & ((1 << eb) - 1)


def _dist_code(dist):
    c = dist - 1
    if c < 4:
        return c, 0, 0
    eb = c.bit_length() - 2
    return 2 * (eb + 1) + ((c >> eb) & 1), eb, c & ((1 << eb) - 1)


def put_tokens(w, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs; then the end-of-block code"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            s, eb, ev = _len_code(t[0])
            w.code(*lit[s])
            w.put(ev, eb)
            s, eb, ev = _dist_code(t[1])
            w.code(*dist.get(s, (0, 1)))         # (a symbol the code does not define: one bit, for the streams that are meant to fail)
            w.put(ev, eb)
    w.code(*lit[256])


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def fixed_block(w, tokens, final=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(w, data, final=True, nlen=None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


CL_LENS = [4] * 13 + [5] * 6          # the code-length code of the hand-written blocks: complete, every symbol present
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def auto_cl(lens):
    """code-length symbols for lens: zero runs by 18 / 17, everything else one by one -> [(symbol, extra value)]"""
    out, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 11:
                out.append((18, j - i - 11))
            elif j - i >= 3:
                out.append((17, j - i - 3))
            else:
                out.extend([(0, 0)] * (j - i))
            i = j
        else:
            out.append((lens[i], 0))
            i += 1
    return out


def dynamic_block(w, tokens, litlens, distlens, final=True, cl_syms=None, hlit=None, hdist=None):
    """cl_syms: the code-length symbols as they are to be written (default: auto_cl over both length lists)"""
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put((len(litlens) if hlit is None else hlit) - 257, 5)
    w.put((len(distlens) if hdist is None else hdist) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for s, ev in (auto_cl(list(litlens) + list(distlens)) if cl_syms is None else cl_syms):
        w.code(*cl[s])
        if s >= 16:
            w.put(ev, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, canonical(litlens), canonical(distlens))


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def dna(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"ACGT") for _ in range(n))


def fasta_text(lines, cols, seed):
    r = random.Random(seed)
    body = b"".join(bytes(r.choice(b"ACGT") for _ in range(cols)) + b"\n" for _ in range(lines))
    return b">contig_%d some description\n" % seed + body


def acgt_lits(ld=(2, 2, 3, 3, 3, 3)):
    """literal/length lengths with codes for A C G T, end-of-block and length symbol 257 (a match of three)"""
    lens = [0] * 258
    for s, l in zip((65, 67, 71, 84, 256, 257), ld):
        lens[s] = l
    return lens


def _hand_written():
    cases = []
    # a stored block of no bytes between two that hold some
    w = Bits()
    stored_block(w, b">x\nACGT", final=False)
    stored_block(w, b"", final=False)
    stored_block(w, b"", final=False)
    stored_block(w, b"TTGA\n", final=True)
    cases.append(("stored_len0_in_the_middle", member(w.bytes(), b">x\nACGTTTGA\n")))
    # a dynamic block with one distance code (one bit long: an incomplete set zlib accepts)
    toks = [65, 67, 71, 84, (3, 1), 65, (3, 1), 71]
    w = Bits()
    dynamic_block(w, toks, acgt_lits(), [1])
    cases.append(("dynamic_single_distance_code", member(w.bytes(), expand(toks))))
    # a dynamic block with no distance code at all
    toks = [65, 67, 71, 84, 84, 65]
    w = Bits()
    dynamic_block(w, toks, acgt_lits(), [0])
    cases.append(("dynamic_no_distance_code", member(w.bytes(), expand(toks))))
    # a repeat-16 that starts in the literal/length lengths and ends in the distance lengths
    lit, dist = acgt_lits(), [3] * 8
    cl = auto_cl(lit[:257]) + [(16, 3)] + [(3, 0)] * 3      # lens[256] = 3 is the last one written plainly; six copies: lens[257], dist[0..4]
    toks = [65, 67, 71, 84, (3, 4), 67, (3, 2), (3, 8), 84]
    w = Bits()
    dynamic_block(w, toks, lit, dist, cl_syms=cl)
    cases.append(("dynamic_repeat16_crosses_into_distances", member(w.bytes(), expand(toks))))
    # header flags
    text = fasta_text(5, 60, 3)
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    deflate = raw.compress(text) + raw.flush()
    cases.append(("header_fextra_fhcrc", member(deflate, text, flags=4 | 2, extra=b"BC\x02\x00\x34\x12")))
    cases.append(("header_all_fields", member(deflate, text, flags=4 | 8 | 16 | 2, extra=b"xy\x01\x00z", name=b"genome.fna", comment=b"a comment")))
    # the second half copies the first at distance exactly 32768 (zlib itself never reaches back that far)
    first = dna(32768, 11)
    toks = list(first) + [(258, 32768)] * 126 + [(130, 32768)] * 2
    w = Bits()
    fixed_block(w, toks)
    cases.append(("distance_32768", member(w.bytes(), first + first)))
    # every length and a spread of distances, overlapping copies among them
    r = random.Random(5)
    toks = list(dna(300, 12))
    for length in range(3, 259):
        toks.append((length, r.choice([1, 2, 3, length - 1, length, length + 1, 63, 64, 65, 257, 299])))
        toks.append(r.choice(b"ACGT"))
    w = Bits()
    fixed_block(w, toks)
    cases.append(("every_length_fixed", member(w.bytes(), expand(toks))))
    return cases


def _failing():
    cases = []
    text = fasta_text(70, 80, 21)
    good = gz(text)
    pad = b"\0" * 16                               # (a job shorter than a header and a trailer is refused before its first block)
    cases.append(("truncated_in_header", good[:7], len(text), EDATA))
    cases.append(("truncated_in_fname", member(b"", b"", flags=8, name=b"a_long_file_name.fna")[:22], 64, EDATA))
    cases.append(("truncated_mid_block", good[:len(good) // 2], len(text), EDATA))
    cases.append(("truncated_in_trailer", good[:-3], len(text), EDATA))
    cases.append(("block_type_3", member(b"\x07" + pad, b""), 64, EDATA))
    w = Bits()
    stored_block(w, b"ACGT", nlen=0x1234)
    cases.append(("len_nlen_mismatch", member(w.bytes() + pad, b"ACGT"), 64, EDATA))
    w = Bits()
    fixed_block(w, [65, (3, 2)])
    cases.append(("distance_before_member_start", member(w.bytes() + pad, b"AAAA"), 64, EDATA))
    # in a second member the distance reaches into the first member's text: still before ITS member's start
    w = Bits()
    fixed_block(w, [65, (3, 2)])
    cases.append(("distance_into_previous_member", gz(b"ACGTACGT") + member(w.bytes() + pad, b"AAAA"), 64, EDATA))
    w = Bits()
    dynamic_block(w, [65], acgt_lits((1, 1, 1, 3, 3, 3)), [1])
    cases.append(("oversubscribed_lengths", member(w.bytes() + pad, b"A"), 64, EDATA))
    w = Bits()
    dynamic_block(w, [65], acgt_lits((2, 2, 3, 3, 3, 4)), [1])
    cases.append(("incomplete_lengths", member(w.bytes() + pad, b"A"), 64, EDATA))
    for hlit in (30, 31):
        w = Bits()
        dynamic_block(w, [65], acgt_lits(), [1], hlit=257 + hlit)
        cases.append(("hlit_%d" % hlit, member(w.bytes() + pad, b"A"), 64, EDATA))
    w = Bits()
    dynamic_block(w, [65], acgt_lits(), [1], cl_syms=[(16, 0)] + auto_cl(acgt_lits() + [1]))
    cases.append(("repeat_without_previous_length", member(w.bytes() + pad, b"A"), 64, EDATA))
    w = Bits()
    dynamic_block(w, [65, (3, 1)], acgt_lits(), [0])
    cases.append(("distance_code_not_defined", member(w.bytes() + pad, b"AAAA"), 64, EDATA))
    flip = lambda b, at, bit: b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]
    cases.append(("crc_bit_flipped", flip(good, len(good) - 7, 3), len(text), ECHECK))
    cases.append(("isize_bit_flipped", flip(good, len(good) - 4, 0), len(text), ECHECK))
    cases.append(("header_crc_wrong", flip(member(b"\x03\x00", b"", flags=2), 10, 1), 64, ECHECK))
    cases.append(("data_bit_flipped", flip(good, len(good) // 2, 5), len(text) + 4096, NOT_OK))
    cases.append(("not_gzip", text[:400], 4096, EDATA))
    cases.append(("garbage_behind_the_member", good + b"trailing bytes that are no member", len(text), EDATA))
    cases.append(("reserved_flag", flip(good, 3, 7), len(text), EDATA))
    return cases


@functools.lru_cache(maxsize=None)
def corpus():
    """-> [(name, gzip bytes, outCap, expected status, expected text or None)], made once"""
    text = fasta_text(70, 80, 1)
    big = dna(1 << 20, 2)
    out = []

    def valid(name, stream, cap_extra=0):
        want = ref_inflate(stream)
        out.append((name, stream, len(want) + cap_extra, OK, want))

    valid("empty", gz(b""))
    valid("one_byte", gz(b"A"))
    valid("dna_70x80", gz(text))
    valid("dna_70x80_roomy_cap", gz(text), cap_extra=333)
    valid("level0_stored_blocks", gz(dna(150_000, 3), 0))
    valid("level1", gz(fasta_text(3000, 80, 4), 1))
    valid("level6", gz(fasta_text(3000, 80, 4), 6))
    valid("level9", gz(fasta_text(3000, 80, 4), 9))
    valid("z_fixed", gz(fasta_text(400, 80, 5), 6, zlib.Z_FIXED))
    valid("repeated_byte_300k", gz(b"N" * 300_000, 9))
    valid("random_acgt_1mib", gz(big))
    repeats = dna(5000, 6)
    valid("long_matches", gz(b"".join(repeats[i % 7:] for i in range(60)), 9))
    valid("binary_bytes", gz(random.Random(7).randbytes(70_000)))
    for name, stream in _hand_written():
        valid(name, stream)
    valid("two_members", gz(text) + gz(dna(40_000, 8), 9))
    valid("three_members_one_empty", gz(dna(33_000, 9)) + gz(b"") + gz(text, 1))
    valid("member_after_stored", gz(dna(70_000, 10), 0) + gz(text))
    out.append(("cap_one_short", gz(text), len(text) - 1, ESHORT, None))
    out.append(("cap_one_short_stored", gz(text, 0), len(text) - 1, ESHORT, None))
    out.append(("cap_zero", gz(text), 0, ESHORT, None))
    for name, stream, cap, status in _failing():
        try:
            ref_inflate(stream)
        except zlib.error:
            pass
        else:
            raise AssertionError("zlib accepts the stream of case %s" % name)
        out.append((name, stream, cap, status, None))
    return out


def write_corpus(path):
    """the corpus as tests/fasta_inflate_emu.cpp reads it"""
    with open(path, "wb") as f:
        cases = corpus()
        f.write(struct.pack("<I", len(cases)))
        for name, stream, cap, status, want in cases:
            nm = name.encode()
            f.write(struct.pack("<IQQiQ", len(nm), len(stream), cap, status, len(want) if want is not None else 0))
            f.write(nm + stream + (want or b""))
