"""Cut streams and maps no encoder wrote, for the inverse of the `-m3` reverse-complement pass (mbgc_amd/csrc/copmem_restore.h):
constructed cases, each aimed at one place where k_restore_fill, k_mark_write, k_varint_decode or k_check could be subtly wrong
and all accepted by design, and mutants of a dozen of them, which the referee (_rcrestore.restore_bounded) labels accepted or
refused. Built on the CPU with fixed seeds. tests/test_rcrestore_mutants_cpu.py holds the corpus to its conditions and sends all
of it through tests/rcrestore_emu.cpp; tests/test_gpu_rcrestore_mutants.py runs it on the device."""
import functools
import struct

import numpy as np

import _rcrestore
from _rcrestore import MARK, put_byte_frugal, restore_bounded

TILE, LANE = 4096, 16
MIN_LENS = (0, 1, 55, 200)
NOT_MARK = np.array([v for v in range(256) if v != MARK], dtype=np.uint8)
LADDER_DEPTH = 1024                                      # the deepest chain of the corpus: see ladder()
GRID_TILES = 8192                                        # the fill and the mark kernels go grid-stride above this many tiles
CLASSES = ("offset", "length", "minlen", "mark-insert", "mark-delete", "varint-byte", "mapoff-size", "maplen-size")
MAY_BE_ACCEPTED = ("offset", "length", "minlen", "varint-byte")
PER_CLASS = 40


def padded(v, nbytes):
    """the byte-frugal value v in exactly nbytes bytes (continuation bytes of 0x80 and a last byte of 0 pad it)"""
    b = bytearray(put_byte_frugal(v))
    assert len(b) <= nbytes
    while len(b) < nbytes:
        b[-1] |= 0x80
        b.append(0)
    return bytes(b)


class Case:
    def __init__(self, name, cut, map_off, map_len, off_bytes, family, seed=None):
        self.name, self.cut, self.map_off, self.map_len, self.off_bytes = name, bytes(cut), bytes(map_off), bytes(map_len), off_bytes
        self.family, self.seed = family, seed
        self._ref = None

    @property
    def ref(self):
        """the referee's verdict: (bytes, M, from matches, deepest chain, minimum) or a refusal's reason"""
        if self._ref is None:
            self._ref = restore_bounded(self.cut, self.map_off, self.map_len, self.off_bytes)
        return self._ref

    @property
    def accepted(self):
        return not isinstance(self.ref, str)

    def label(self):
        return self.name if self.seed is None else "%s (seed %d)" % (self.name, self.seed)


class Build:
    """a cut stream written front to back: literals and matches, positions in restored coordinates"""

    def __init__(self, seed, min_len=0):
        self.rng = np.random.default_rng(seed)
        self.min_len, self.parts, self.matches, self.enc = min_len, [], [], []
        self.pos = self.cut_pos = 0

    def lit(self, n, data=None):
        assert n >= 0
        b = bytes(NOT_MARK[self.rng.integers(0, 255, n)]) if data is None else bytes(data)
        assert MARK not in b
        self.parts.append(b)
        self.pos += len(b)
        self.cut_pos += len(b)
        return self

    def lit_to(self, pos):
        return self.lit(pos - self.pos)

    def match(self, src, ln, nbytes=None):
        """nbytes: the length is written as a padded value of that many bytes"""
        assert src + ln <= self.pos and ln >= self.min_len, (src, ln, self.pos)
        self.parts.append(bytes([MARK]))
        self.matches.append((src, ln))
        self.enc.append(nbytes)
        self.pos += ln
        self.cut_pos += 1
        return self

    def maps(self, off_bytes=4, min_bytes=None):
        map_off = b"".join(int(s).to_bytes(off_bytes, "little") for s, _ in self.matches)
        enc = lambda v, k: put_byte_frugal(v) if k is None else padded(v, k)
        map_len = enc(self.min_len, min_bytes) + b"".join(enc(ln - self.min_len, k) for (_, ln), k in zip(self.matches, self.enc))
        return map_off, map_len

    def case(self, name, family, off_bytes=4, min_bytes=None):
        return Case(name, b"".join(self.parts), *self.maps(off_bytes, min_bytes), off_bytes=off_bytes, family=family)


# ---- constructed cases ---------------------------------------------------------------------------------------------------
def edges():
    """a match start, a match end and a source start at every offset -17..+17 around a lane edge and two tile edges"""
    out = []
    for e, edge in enumerate((2064, TILE, 2 * TILE)):
        for o in range(-17, 18):
            ml = MIN_LENS[(o + 17 + e) % 4]
            b = Build(1000 + 100 * e + o, ml).lit_to(edge + o).match(37, 300).lit(900)
            out.append(b.case("edge: a match starts at %d%+d" % (edge, o), "edges"))
            b = Build(2000 + 100 * e + o, ml).lit_to(edge + o - 300).match(edge // 2 - 300, 300).lit(900)
            out.append(b.case("edge: a match ends at %d%+d" % (edge, o), "edges"))
            b = Build(3000 + 100 * e + o, ml).lit_to(edge + 611).match(edge + o, 300).lit(333)
            out.append(b.case("edge: a source starts at %d%+d" % (edge, o), "edges"))
    b = Build(3500, 55).lit_to(2 * TILE + 100).match(100, 2 * TILE - 100).lit(500)   # [8292, 16384): ends on a tile edge
    out.append(b.case("edge: a match ends exactly with tile 3", "edges"))
    b = Build(3501, 200).lit_to(2 * TILE + 100).match(50, 2 * TILE + 1).lit(5000)    # [8292, 16485): tile 3 wholly inside it
    out.append(b.case("edge: tile 3 lies wholly inside one match", "edges"))
    b = Build(3502, 1).lit_to(4 * TILE + 9).match(3, 3 * TILE + 777).lit(41)         # a match longer than three tiles
    out.append(b.case("edge: a match longer than three tiles", "edges"))
    b = Build(3503, 0).lit_to(TILE).match(0, TILE).match(0, 2 * TILE).lit(1)      # matches that start and end on tile edges
    out.append(b.case("edge: matches from tile edge to tile edge", "edges"))
    for k in range(4):
        for r in (0, 1, 15, 16, 17):
            total = TILE * k + r
            if total >= 700:
                b = Build(3600 + total, MIN_LENS[(k + r) % 4]).lit_to(total - 300).match(11, 300)
                out.append(b.case("edge: %d bytes, the last of them a match's" % total, "edges"))
                b = Build(3700 + total, MIN_LENS[(k + r) % 4]).lit_to(300).match(0, 299).lit_to(total)
                out.append(b.case("edge: %d bytes, the last of them literals" % total, "edges"))
            else:
                b = Build(3800 + total).lit(total - total // 2).match(0, total // 2)
                out.append(b.case("edge: %d bytes, the last of them a match's" % total, "edges"))
                out.append(Build(3900 + total).lit(total).case("edge: %d bytes and no match" % total, "edges"))
    return out


def dense():
    out = []
    for r in range(1, 41):
        b = Build(4000 + r)
        lens = [int(x) for x in b.rng.choice([0, 0, 1, 3, 15, 16, 17, 40], r)]
        b.lit(TILE - r // 2 - (r % 3))                                          # the run of marks straddles cut position 4096
        for ln in lens:
            b.match(int(b.rng.integers(0, b.pos - ln + 1)), ln)
        b.lit_to(b.pos + 16 - b.pos % 16 + 300)
        b.lit_to(2 * TILE - (sum(lens[:r // 2])) - (r % 2))                      # ... and the next one the restored position 8192
        for ln in lens:
            b.match(int(b.rng.integers(0, b.pos - ln + 1)), ln)
        b.lit(100 + r)
        lane = b.pos + 16 - b.pos % 16
        b.lit_to(lane + 160 - r // 3)                                           # ... and a run of zero lengths a lane edge
        for _ in range(r):
            b.match(int(b.rng.integers(0, b.pos + 1)), 0)
        b.lit(77)
        out.append(b.case("dense: runs of %d adjacent marks" % r, "dense"))
    for zero in (True, False):
        b = Build(4100 + zero).lit(TILE + 32)                                    # cut position 4128: a lane's whole load is marks
        for j in range(16):
            b.match(j * 7, 0 if zero or j % 3 else 5 + j)
        b.lit(500)
        out.append(b.case("dense: sixteen marks in one load%s" % (", all of length 0" if zero else ""), "dense"))
    for k in (1, 16, 17, 5000):
        b = Build(4200 + k)
        for _ in range(k):
            b.match(0, 0)
        out.append(b.case("dense: %d marks and nothing else, 0 bytes restored" % k, "dense"))
    b = Build(4300).lit(64)
    for j in range(40):
        ln = b.pos if j < 8 else int(b.rng.integers(0, 700))
        b.match(int(b.rng.integers(0, b.pos - ln + 1)), ln)
    out.append(b.case("dense: all text in matches, literals only in the first 64 bytes", "dense"))
    b = Build(4301).lit(300)
    b.match(0, 0).match(300, 0).lit(20).match(320, 0).match(0, 320).match(640, 0).lit(5).match(645, 0)
    out.append(b.case("dense: zero lengths at the start of literals, matches and the end", "dense"))
    return out


def ladder(depth=LADDER_DEPTH, step=32, seed=5000):
    """every match copies the one before it: byte 0 of match j was copied through j + 1 matches. LADDER_DEPTH is the depth at
    which tests/rcrestore_emu.cpp still runs the case in a few seconds under AddressSanitizer (a byte costs a binary search per
    hop, so the case costs depth^2 searches per column of the ladder)."""
    b = Build(seed).lit(step)
    for j in range(depth):
        b.match(j * step, step)                                              # src + len == d exactly
    return b.lit(9).case("chain: a ladder of depth %d" % depth, "chains")


def chains():
    out = []
    b = Build(5100).lit(200)                                                  # the hand-built stream of test_gpu_rcrestore.py, all byte values
    b.match(0, 200).lit(7).match(150, 100).lit(3).match(210, 150).match(523, 101).match(665, 90).lit(21).match(771, 101).lit(5)
    b.match(3, 37).lit(40).match(1001, 33)
    out.append(b.case("chain: depths 1 to 5 by hand", "chains"))
    for depth in (1, 2, 3, 4):
        b = Build(5110 + depth, MIN_LENS[depth % 4]).lit(1000)
        for j in range(depth):
            b.lit(13 + j).match(b.pos - 613 - j, 600)                            # each copies most of the one before it
        out.append(b.lit(50).case("chain: depth %d" % depth, "chains"))
    b = Build(5120, 1).lit(100).match(10, 50).lit(30).match(120, 40).lit(25).match(5, 200).lit(60)
    b.match(90, b.pos - 90 - 60)                                                # from inside match 0 over matches 1 and 2 and the literals between
    b.lit(10).match(0, b.pos)                                                   # everything so far: src + len == d
    out.append(b.case("chain: a source over several matches and the literals between them", "chains"))
    out.append(ladder())
    out.append(ladder(64, 48, 5001))
    return out


def fastpaths():
    """both vector paths, their runs ending at p0 + 15, + 16, + 17 and everywhere else within a lane: a literal run ends where a
    match starts (path 1: the sweep of edges() around 2064 too); the source of 16 bytes of a match is a literal run that ends at
    an inner match, of length 0 or 5, at q: lane p0 = 1024 + 16 j of the match [1024, 1280) reads [s0, s0 + 16), s0 = 484 - 16 j."""
    out = []
    for q in range(300, 336):
        for inner in (0, 5):
            b = Build(6000 + 2 * q + inner).lit_to(q).match(40, inner).lit_to(1024).match(244, 256).lit(100)
            out.append(b.case("fast path 2: the source run ends at %d, an inner match of length %d" % (q, inner), "fastpaths"))
    for o in (15, 16, 17):
        b = Build(6100 + o).lit_to(2048 + o).match(100, 64).lit_to(2048 + 128 + o).match(7, 3).lit(200)
        out.append(b.case("fast path 1: a literal run ends at p0 + %d" % o, "fastpaths"))
        b = Build(6200 + o, 1).lit_to(2048 - 64 + o).match(100, 64).lit(300)
        out.append(b.case("fast path 2: a match ends at p0 + %d" % o, "fastpaths"))
        b = Build(6300 + o, 1).lit_to(1000).match(500 - o, o).lit_to(2048 + o)     # src + len == 500 == the next source's start
        b.match(500, 16 * 20).lit(99)
        out.append(b.case("fast path 2: the source starts where a match of %d bytes ends" % o, "fastpaths"))
    return out


def parity():
    every = bytes(NOT_MARK)                                                   # 127 and 0x80 .. 0xFF without the mark among them
    out = []
    for lead in (0, 7, 16):
        b = Build(7000 + lead).lit(lead).lit(255, every)
        b.match(lead, 255).match(lead + 255, 255).match(lead + 510, 255).lit(3)
        out.append(b.case("parity: every byte value through 1, 2 and 3 hops, %d bytes in" % lead, "parity"))
    b = Build(7100).lit(255, every).lit(9).match(0, 255).lit(9).match(264, 255).lit(9).match(528, 255).lit(9).match(792, 255)
    out.append(b.case("parity: every byte value through 1 to 4 hops, literals between", "parity"))
    b = Build(7101).lit(64, bytes([127]) * 64).match(0, 64).match(64, 64).match(128, 64).lit(5, bytes([127, 0, 255, 0x80, 0xA5]))
    out.append(b.case("parity: byte 127 alone", "parity"))
    return out


def varints():
    out = []
    for value in (0, 5, 127):
        b = Build(8000 + value).lit(2000)
        for k in range(1 if value < 128 else 2, 11):
            b.lit(3).match(k, value, nbytes=k)
        out.append(b.lit(20).case("varint: %d in 1 to 10 bytes" % value, "varints"))
        out.append(b.case("varint: %d in 1 to 10 bytes, the minimal length in 10" % value, "varints", min_bytes=10))
    b = Build(8100, 200).lit(600)
    while b.pos < 38400:
        b.match(0, b.pos)
    for delta in (127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 14 + 1, 0):
        b.lit(6).match(b.pos - (200 + delta) - 11, 200 + delta)
    out.append(b.case("varint: deltas of 127, 128, 2^14 - 1, 2^14, 2^14 + 1 over a minimal length of 200", "varints"))
    out.append(b.case("varint: the same, the minimal length in 3 bytes", "varints", min_bytes=3))
    b = Build(8101, 0).lit(1 << 16)
    while b.pos < (1 << 21):
        b.match(0, b.pos)
    b.lit(5).match(3, 1 << 21).lit(1)
    out.append(b.case("varint: a length of 2^21", "varints"))
    return out


def grid_stride():
    """a little over 32 MiB, cut and restored: 8192 tiles and a few more of both, so that the fill and the two mark kernels all
    take more than one tile per workgroup; some hundreds of marks; matches on both sides of restored tile 8192 and across its
    edge, marks on both sides of the cut stream's tile 8192 and on its edge"""
    edge = GRID_TILES * TILE
    b = Build(9000, 55).lit(1 << 20)
    while b.pos < edge - (1 << 18):
        ln = int(b.rng.integers(55, 1200))
        b.lit(int(b.rng.integers(60_000, 200_000))).match(int(b.rng.integers(0, b.pos - ln + 1)), ln)
    b.lit_to(edge - 9000).match(edge - 20000, 8000).lit(100)                     # ends 900 bytes before the edge
    b.match(12345, 5000)                                                        # across it
    b.lit_to(edge + 2 * TILE + 3).match(edge - 300, 303)                         # behind it, its source across it
    b.lit(2000).match(edge + 1, 2 * TILE + 5)
    assert b.cut_pos < edge - 1
    b.lit(edge - 1 - b.cut_pos).match(77, 60).match(edge - 5, 55).match(edge + 9, 300)   # cut positions edge - 1, edge, edge + 1
    b.lit(3 * TILE).match(b.pos - 5000, 4999).lit(7)
    return b.case("grid stride: %d tiles of cut stream, %d restored" % ((b.cut_pos + TILE - 1) // TILE, (b.pos + TILE - 1) // TILE), "grid")


def eight(c):
    m = len(c.map_off) // 4
    off8 = b"".join(c.map_off[4 * i:4 * i + 4] + b"\0\0\0\0" for i in range(m))
    return Case(c.name + " [8-byte offsets]", c.cut, off8, c.map_len, 8, c.family + "/8")


@functools.lru_cache(maxsize=None)
def constructed():
    four = edges() + dense() + chains() + fastpaths() + parity() + varints()
    return four + [eight(c) for c in four if c.cut.count(bytes([MARK]))] + [grid_stride()]


# ---- mutants -------------------------------------------------------------------------------------------------------------
def slack(seed, min_len, n_matches, off_bytes=4, alternate=False):
    """sources in the first 1500 bytes, the first match behind 4000: a length or the minimum may change by hundreds. alternate:
    every other length is the minimum and up to 3 more behind one of two bytes — where moving a continuation bit on by one byte
    gives two other lengths that still fit"""
    b = Build(seed, min_len).lit(4000 + seed % 50)
    for j in range(n_matches):
        ln = int(b.rng.integers(max(min_len, 1), 420))
        if alternate:
            ln = min_len + (int(b.rng.integers(0, 4)) if j % 2 else int(b.rng.integers(128, 420)))
        b.lit(int(b.rng.integers(0, 600))).match(int(b.rng.integers(0, 1000)), ln)
    b.lit(int(b.rng.integers(0, 300)))
    return b, off_bytes


def tight(seed, min_len, off_bytes=4):
    """matches that copy what lies right in front of them, chains of them"""
    b = Build(seed, min_len).lit(700)
    for j in range(30):
        ln = int(b.rng.integers(max(min_len, 1), min(b.pos, 900)))
        gap = int(b.rng.choice([0, 0, 1, 16, 200]))
        b.lit(int(b.rng.choice([0, 1, 15, 40]))).match(max(0, b.pos - ln - gap), ln)
    return b, off_bytes


@functools.lru_cache(maxsize=None)
def bases():
    """about a dozen accepted streams of 5 to 40 kB restored, as (Build, width of an offset)"""
    out = [slack(11, 0, 12), slack(12, 1, 25), slack(13, 55, 9), slack(14, 200, 6), slack(15, 0, 30, off_bytes=8), slack(16, 55, 20, alternate=True),
           slack(17, 0, 24, alternate=True), slack(18, 1, 16, alternate=True), tight(21, 0), tight(22, 1), tight(23, 55, off_bytes=8), tight(24, 200)]
    for b, w in out:
        assert 5000 <= b.pos <= 40000, b.pos
    return out


def mutate(cls, b, w, rng, grow):
    """one mutation of class cls of (cut, matches, min_len, map_off, map_len) -> the same, changed. grow: the classes that change
    a size add (or take away) in every mutation of a case, so that two of them do not cancel"""
    cut, matches, min_len, map_off, map_len = b
    m = len(matches)
    marks = [i for i, x in enumerate(cut) if x == MARK]
    ds, cum = [], 0
    for i, (s, ln) in enumerate(matches):
        ds.append((marks[i] if i < len(marks) else 0) - i + cum)                 # (the marks are those of the maps but for the mark classes)
        cum += ln
    i = int(rng.integers(0, m))
    s, ln = matches[i]
    if cls == "offset":
        how = int(rng.integers(0, 7 if w == 8 else 6))
        new = [s + 1, max(s - 1, 0), s + 16, max(s - 16, 0), ds[i] - ln + 1 if how % 2 else max(ds[i] - ln - 1, 0), ds[i] - ln,
               s | (1 << int(rng.integers(32, 64)))][how] if how != 5 or rng.integers(0, 2) else cum + len(cut) + int(rng.integers(0, 1 << 30))
        matches = matches[:i] + [(new, ln)] + matches[i + 1:]
    elif cls == "length":
        how = int(rng.integers(0, 6))
        new = [ln + 1, max(ln - 1, min_len), ds[i] - s + 1, max(ds[i] - s - 1, min_len), max(ds[i] - s, min_len),
               min_len + (1 << int(rng.choice([31, 40, 62, 63])))][how]
        matches = matches[:i] + [(s, new)] + matches[i + 1:]
    elif cls == "minlen":
        delta = int(rng.choice([1, -1, 2, 16, -16, 100, 1 << 32, (1 << 32) - 1 - min_len, 1 << 62]))
        new = max(min_len + delta, 0)
        matches = [(s, ln - min_len + new) for s, ln in matches]
        min_len = new
    if cls in ("offset", "length", "minlen"):
        bb = Build(0, min_len)
        bb.matches, bb.enc = matches, [None] * m
        map_off, map_len = bb.maps(w)
    elif cls == "mark-insert":
        at = int(rng.integers(0, len(cut) + 1))
        cut = cut[:at] + bytes([MARK]) + (cut[at:] if rng.integers(0, 2) or at == len(cut) else cut[at + 1:])
        if cut.count(bytes([MARK])) == m:                                       # (a mark written over a mark)
            cut = cut + bytes([MARK])
    elif cls == "mark-delete":
        at = marks[int(rng.integers(0, len(marks)))]
        cut = cut[:at] + (b"" if rng.integers(0, 2) else b"A") + cut[at + 1:]
    elif cls == "varint-byte":
        ml = bytearray(map_len)
        how = int(rng.integers(0, 10))
        two = [j for j in range(len(ml) - 2) if ml[j] >= 128 and ml[j + 1] < 128 and (j == 0 or ml[j - 1] < 128) and ml[j + 2] < 4]
        if how >= 2 and two:                                                    # a two-byte value and its successor become a one-byte value and a longer one
            j = two[int(rng.integers(0, len(two)))]
            ml[j] &= 127
            ml[j + 1] |= 128
        elif how == 0:
            ml.append(0x80)
        else:
            ml[int(rng.integers(0, len(ml)))] ^= 0x80
        map_len = bytes(ml)
    elif cls == "mapoff-size":
        k = int(rng.choice([1, 4, 8])) * (1 if grow else -1)
        at = int(rng.integers(0, len(map_off) + k + 1)) if k < 0 else len(map_off)   # (bytes taken out anywhere, added at the end)
        map_off = map_off[:at] + map_off[at - k:] if k < 0 else map_off + bytes(int(x) for x in rng.integers(0, 256, k))
    elif cls == "maplen-size":
        vals = _rcrestore.values_of(map_len)
        j = int(rng.integers(0, len(vals)))
        at = sum(k for _, k in vals[:j])
        map_len = map_len[:at] + map_len[at + vals[j][1]:] if not grow else map_len[:at] + put_byte_frugal(int(rng.integers(0, 300))) + map_len[at:]
    return cut, matches, min_len, map_off, map_len


@functools.lru_cache(maxsize=None)
def mutants(cls):
    """PER_CLASS cases: 1 to 3 mutations of the class on one of bases()"""
    out = []
    for k in range(PER_CLASS):
        seed = 100_000 + 1000 * CLASSES.index(cls) + k
        rng = np.random.default_rng(seed)
        b, w = bases()[k % len(bases())]
        if cls == "varint-byte" and k % 5 < 3:                                  # (the streams where a moved bit can still be accepted)
            b, w = bases()[5 + k % 3]
        state = (b"".join(b.parts), list(b.matches), b.min_len) + b.maps(w)
        for _ in range(1 + k % 3 if cls not in ("minlen",) else 1):
            state = mutate(cls, state, w, rng, k % 2 == 1)
        out.append(Case("%s #%d" % (cls, k), state[0], state[3], state[4], w, cls, seed))
    return out


def good():
    """the fixed good stream a handle restores after every refusal"""
    return constructed_by_name("chain: depths 1 to 5 by hand")


def constructed_by_name(name):
    return next(c for c in constructed() if c.name == name)


def everything():
    return constructed() + [c for cls in CLASSES for c in mutants(cls)]


def varint_streams():
    """[(bytes, [(value or None beyond 2^62, ends within 10 bytes)])]: values the item body of k_varint_decode is held to alone,
    those no accepted case can hold among them (2^28 and 2^35 as lengths would take gigabytes)"""
    vals = [0, 1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 14 + 1, 2 ** 21, 2 ** 28, 2 ** 35, 2 ** 62 - 1, 2 ** 62, 2 ** 62 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    streams = [b"".join(put_byte_frugal(v) for v in vals)]
    for v in (0, 5, 127, 128, 2 ** 35, 2 ** 62):
        streams.append(b"".join(padded(v, k) for k in range(len(put_byte_frugal(v)), 12)))
    streams.append(b"\x80" * 9 + b"\x01" + b"\xff" * 9 + b"\x00" + b"\xff" * 10 + b"\x00" + b"\x80" * 30 + b"\x05" + b"\x07")
    out = []
    for s in streams:
        want = [(v if v <= _rcrestore.CAP else None, k <= _rcrestore.MAX_VARINT) for v, k in _rcrestore.values_of(s)]
        out.append((s, want))
    return out


def write_corpus(path, cases):
    """the file tests/rcrestore_emu.cpp reads: the complement table, the varint streams, then every case with the referee's verdict"""
    u64 = lambda v: struct.pack("<Q", v)
    with open(path, "wb") as f:
        f.write(b"RCMUT1\0\0" + _rcrestore.LUT.tobytes())
        vs = varint_streams()
        f.write(u64(len(vs)))
        for s, want in vs:
            f.write(u64(len(s)) + s + u64(len(want)))
            for v, ok in want:
                f.write(u64((1 << 64) - 1 if v is None else v) + u64(ok))
        f.write(u64(len(cases)))
        for c in cases:
            name = c.label().encode()
            f.write(u64(len(name)) + name + u64(c.off_bytes) + u64(c.accepted))
            for blob in (c.cut, c.map_off, c.map_len):
                f.write(u64(len(blob)) + blob)
            if c.accepted:
                data, m, total, deep, min_len = c.ref
                f.write(u64(m) + u64(total) + u64(deep) + u64(min_len) + u64(len(data)) + data)
