"""A corpus of stream sets no encoder wrote, for the device decoder (mbgc_amd/csrc/swsem_decode.hip) and its referee, the bounded
form of the oracle's decoder (orc_decode_contig_bounded, oracle/decode_oracle.c). Built on the CPU alone.

Per parameter row (ROWS) a small collection is matched and emitted by the oracle; every case is the six streams of one of its
contigs after 1-3 token-level mutations of one named class (CLASSES), closed under the referee: if the referee decodes the
mutant, the five streams that are not the literals are cut where it stopped reading, and the case is ACCEPTED with the bytes,
destLen and unmatchedChars the referee gives on exactly those streams; otherwise it is REJECTED. A few accepted cases with one
byte appended to one stream are rejected for the byte left over (class "leftover"). The reference buffer is the oracle
matcher's, REF_MAX bytes of which some 340 kB are loaded; offsets point below the loaded length or at least 4096 bytes beyond the
device handle's buffer (its REF_MAX bytes and the slack behind them), and every case gives the same verdict with the buffer's
end moved across that slack (`slack_same`), so the slack decides nothing. Seeds are fixed: the corpus is the same everywhere."""
import functools
import struct

import numpy as np

import _driver
import _orc
from mbgc_amd import synth

REF_MAX = 1 << 20
DEVICE_SLACK = 256                  # what a matcher handle keeps behind its buffer (REF_SLACK, mbgc_amd/csrc/swsem_runtime_state.h)
FAR = REF_MAX + DEVICE_SLACK + 4096
MARK = 0xA5                         # MATCH_MARK, MBGC_Params.h:45
ORACLE_CAP = 1 << 18                # no accepted contig is longer
REJECT_CAP = 1 << 16                # destCap of a rejected case
LOCK_POS = 100_001
NAMES = _orc.STREAM_NAMES
LIT, OFF, OFF5, LEN, GAP, FLAGS = range(6)

ROWS = (("m0", dict(mode=0)), ("m1", dict(mode=1)), ("m2", dict(mode=2)), ("m1-eager", dict(mode=1, lazy=0)),
        ("m1-plainlen", dict(mode=1, flip_frugal=1)), ("m1-bit40", dict(mode=1, bit40=1)), ("m1-lock", dict(mode=1, lock=1)))
CLASSES = ("flag-flip", "flag-run", "literal", "length", "offset", "gapdelta", "mark", "refpoke")
PER_CLASS = 40
LEFTOVER = 12
PAD_OFFSETS = 512


class Case:
    __slots__ = ("row", "cls", "seed", "what", "streams", "accepted", "expect", "dest_len", "unmatched", "walk", "slack_same")

    def dest_cap(self):
        return self.dest_len + 16 if self.accepted else REJECT_CAP

    def label(self):
        return "row %s, class %s, seed %s (%s)" % (self.row, self.cls, self.seed, self.what)


class Row:
    pass


# ---- tokens -----------------------------------------------------------------------------------------------------------
def parse_lens(b, frugal):
    """decodeMapLenStream, MBGC_Decoder.cpp:966-986 (readUInt64Frugal, utils/helper.h:256-272)"""
    if not frugal:
        return list(struct.unpack("<%dI" % (len(b) // 4), b))
    out, i = [], 0
    while i < len(b):
        v = int.from_bytes(b[i:i + 2], "little"); i += 2
        if v == 0xFFFF:
            v = int.from_bytes(b[i:i + 4], "little"); i += 4
            if v == 0xFFFFFFFF:
                v = int.from_bytes(b[i:i + 8], "little"); i += 8
        out.append(v)
    return out


def put_lens(lens, frugal):
    return b"".join(_driver.frugal64(v) for v in lens) if frugal else struct.pack("<%dI" % len(lens), *lens)


class Tokens:
    def __init__(self, streams, frugal):
        self.frugal = frugal
        self.lit = bytearray(streams[LIT])
        self.offs = list(struct.unpack("<%dI" % (len(streams[OFF]) // 4), streams[OFF]))
        self.off5 = bytearray(streams[OFF5])
        self.lens = parse_lens(streams[LEN], frugal)
        self.gap = bytearray(streams[GAP])
        self.flags = bytearray(streams[FLAGS])

    def streams(self):
        return [bytes(self.lit), struct.pack("<%dI" % len(self.offs), *self.offs), bytes(self.off5), put_lens(self.lens, self.frugal),
                bytes(self.gap), bytes(self.flags)]


# ---- mutations: each returns a word on what it did, or None when the contig has no such token -----------------------------
def _pick(rng, n):
    return int(rng.integers(0, n)) if n else None


def mut_flag_flip(rng, t, row):
    i = _pick(rng, len(t.flags))
    if i is None:
        return None
    if getattr(t, "at_end", False):                   # (a mutant without padding: where the contig's last extensions read)
        i = len(t.flags) - 1 - int(rng.integers(0, min(48, len(t.flags))))
    t.flags[i] = 0 if t.flags[i] else 1
    return "flag %d -> %d" % (i, t.flags[i])


def mut_flag_run(rng, t, row):
    if len(t.flags) < 70:
        return None
    i = 64 * int(rng.integers(0, (len(t.flags) - 69) // 64 + 1)) + int(rng.integers(60, 69))
    n, v = int(rng.integers(1, 131)), int(rng.integers(0, 2))
    n = min(n, len(t.flags) - i)
    t.flags[i:i + n] = bytes([v]) * n
    return "flags [%d, +%d) = %d" % (i, n, v)


def mut_literal(rng, t, row, how=None):
    at = [i for i, c in enumerate(t.lit) if c != MARK]
    if not at:
        return None
    i = at[int(rng.integers(0, len(at)))]
    how = int(rng.integers(0, 3)) if how is None else how
    if how == 0:
        v = b"ACGTN"[int(rng.integers(0, 5))]
    elif how == 1:
        v = int(rng.integers(0, 5))
    else:
        v = int(rng.integers(5, 256))
        if v == MARK:
            v = 0xA6
    t.lit[i] = v
    return "literal %d = 0x%02x" % (i, v)


def mut_length(rng, t, row):
    i = _pick(rng, len(t.lens))
    if i is None:
        return None
    old = t.lens[i]
    v = (0, 1, 191, 192, 193, 65534, 65535, 65536, max(old - 1, 0), old + 1)[int(rng.integers(0, 10))]
    t.lens[i] = v
    return "length %d: %d -> %d" % (i, old, v)


def mut_offset(rng, t, row):
    """the encoder pairs nearly every match with the one in front of it (gapDelta) and writes a contig's first offset only: a
    gapDelta is cleared first, so that the match behind it takes the next offset (the first of the padding), and an offset that is
    read is moved"""
    if not len(t.gap) or not t.offs:
        return None
    g = int(rng.integers(0, len(t.gap)))
    t.gap[g] = 0
    t.unpaired = getattr(t, "unpaired", 0) + 1
    i = int(rng.integers(0, min(t.unpaired + 1, len(t.offs))))
    old = t.offs[i]
    targets = [old - 1, old + 1, old - 16, old + 16, 1, row.loaded - 1, FAR + int(rng.integers(0, 1 << 20))]
    if row.lock != _orc.NO_LOCK:
        targets += [row.lock, row.lock - 1, row.lock + 1] * 2
    v = targets[int(rng.integers(0, len(targets)))]
    if v < 0:
        v = 0
    elif v >= row.loaded:                             # (nothing between the loaded text and FAR)
        v = FAR + int(rng.integers(0, 1 << 20))
    t.offs[i] = v
    return "gapDelta %d = 0, offset %d: %d -> %d" % (g, i, old, v)


def mut_gapdelta(rng, t, row):
    i = _pick(rng, len(t.gap))
    if i is None:
        return None
    old, v = t.gap[i], int(rng.integers(0, 9))
    t.gap[i] = v
    return "gapDelta %d: %d -> %d" % (i, old, v)


def mut_mark(rng, t, row):
    marks = [i for i, c in enumerate(t.lit) if c == MARK]
    if marks and rng.integers(0, 2):
        i = marks[int(rng.integers(0, len(marks)))]
        del t.lit[i]
        return "mark at %d deleted" % i
    i = int(rng.integers(0, len(t.lit) + 1))
    t.lit.insert(i, MARK)
    return "mark inserted at %d" % i


MUTATORS = {"flag-flip": mut_flag_flip, "flag-run": mut_flag_run, "literal": mut_literal, "length": mut_length, "offset": mut_offset,
            "gapdelta": mut_gapdelta, "mark": mut_mark}


# ---- the base streams of a row ----------------------------------------------------------------------------------------
def _contigs(rng):
    """six contigs of 22-40 kB at divergence 0.01-0.05 (two of them with a same-length substitution: gaps), forward and reverse
    complemented, and two more (the last 40 kB of the genome) whose part of the reference belongs to the class "refpoke" alone"""
    base = synth.base_codes(170_000, 4242)
    g0 = synth.genome(base, 0, 0.0)
    out = []
    for i, (a, b, div, rc, sub) in enumerate(((0, 25_000, 0.01, 0, 0), (20_000, 50_000, 0.02, 1, 0), (45_000, 85_000, 0.03, 0, 250),
                                              (60_000, 82_000, 0.05, 1, 3000), (88_000, 128_000, 0.01, 0, 0), (95_000, 130_000, 0.02, 1, 0),
                                              (130_000, 150_000, 0.02, 0, 0), (150_000, 170_000, 0.03, 0, 0))):
        c = synth.genome(base, 1 + i, div)[a:b].copy()
        if sub:
            at = (b - a) // 3
            c[at:at + sub] = synth.ACGT[rng.integers(0, 4, sub)]
        out.append(_driver.revcomp(c) if rc else c)
    return g0, out


@functools.lru_cache(maxsize=None)
def row(name):
    opts = dict(ROWS)[name]
    r = Row()
    r.name, r.mode = name, opts["mode"]
    over = {}
    if "lazy" in opts:
        over["lazyDecompressionSupport"] = opts["lazy"]
    if opts.get("bit40"):
        over["enable40bitReference"] = 1
    r.params = _orc.emit_params(r.mode, **over)
    if opts.get("flip_frugal"):
        r.params.frugal64bitLenEncoding = 0 if r.params.frugal64bitLenEncoding else 1
    r.over = dict(over, frugal64bitLenEncoding=r.params.frugal64bitLenEncoding)
    r.frugal = bool(r.params.frugal64bitLenEncoding)
    rng = np.random.default_rng(77)
    g0, r.contigs = _contigs(rng)
    m = _orc.OracleMatcher(REF_MAX, skip_margin=24 if r.mode >= 2 else 16)
    m.load_ref(g0, load_rc=True)
    r.loaded = m.loaded_ref_length()
    loaded = [r.loaded]
    r.lock = _orc.NO_LOCK
    if opts.get("lock"):
        # the sliding window's end inside the loaded text (SlidingWindowSparseEMMatcher.cpp:361-378 on a buffer that has wrapped):
        # matches lie in [lock, loading position), a left extension stops at the lock
        m.set_sliding_window_size(2)
        m.set_position(REF_MAX // 2 + LOCK_POS - 1, 1)
        r.lock = m.acquire_lock()
        assert r.lock == LOCK_POS < r.loaded
    r.base = []
    for k, c in enumerate(r.contigs):
        rows = m.match(c, 32, r.lock)
        em = _orc.OracleEmitter(m, r.params)
        un = em.process(rows, c, r.lock, 128, 0, 0, loaded)
        assert un != _orc.SKIPPED
        r.base.append(([em.stream(i) for i in range(6)], int(un) & 0xFFFFFFFF, len(rows)))
    r.ref = np.zeros(REF_MAX + DEVICE_SLACK + 4096, dtype=np.uint8)       # (the oracle reads [0, REF_MAX) of it, `slack_same` a little more)
    r.ref[:REF_MAX] = m.ref(REF_MAX)
    r.clean_ref = r.ref.copy()
    m.close()
    _poke(r)
    return r


def referee(r, streams, ref_bytes=REF_MAX, trace=0, ref=None):
    return _orc.decode_contig_bounded(r.ref if ref is None else ref, ref_bytes, r.params, streams, r.lock, ORACLE_CAP, trace)


def _poke(r):
    """non-ACGTN bytes into the reference under the extensions of the last two contigs: under bytes an extension copies (contig 6)
    and under bytes it decodes from a literal code (contig 7: with the code turned into a byte >= 5, which is taken as it is,
    ContextAwareMismatchesCoder.cpp:72-77 — `fixed`; with a code below 5 the reference indexes its table out of range)"""
    r.pokes, r.fixes = [], []
    vals = (0, ord("R"), ord("n"), 0xFF, ord("-"), ord("a"))
    for k, coded, want in ((6, False, 12), (7, True, 8)):
        tr = referee(r, r.base[k][0], trace=1 << 17, ref=r.clean_ref)
        assert tr["unmatched"] >= 0
        reads = [(p, l) for p, l in tr["trace"] if (l != _orc.NO_LOCK) == coded]
        once = {}
        for p, l in tr["trace"]:
            once[p] = once.get(p, 0) + 1
        reads = [(p, l) for p, l in reads if once[p] == 1]
        assert len(reads) >= want, (r.name, k, len(reads))
        for j in range(want):
            p, l = reads[(2 * j + 1) * len(reads) // (2 * want)]
            r.ref[p] = vals[j % len(vals)]
            r.pokes.append(int(p))
            if coded:
                r.fixes.append((int(l), 5 + 31 * j))
    fixed = bytearray(r.base[7][0][LIT])
    for l, v in r.fixes:
        assert fixed[l] < 5 and v != MARK
        fixed[l] = v
    r.fixed = [bytes(fixed)] + list(r.base[7][0][1:])


# ---- cases ------------------------------------------------------------------------------------------------------------
def _pad(rng, t, r):
    """tokens behind the contig's own, so that a mutant that reads further than the contig did finds something there; what
    the referee does not read is cut off again"""
    t.flags += bytes((rng.random(8192) < 0.1).astype(np.uint8))
    t.offs += [int(x) for x in rng.integers(r.lock + 64 if r.lock != _orc.NO_LOCK else 64, r.loaded - 4096, PAD_OFFSETS)]
    t.off5 += bytes(PAD_OFFSETS)
    t.lens += [int(x) for x in rng.integers(20, 60, 64)]
    t.gap += bytes(64)


def close(r, streams):
    """-> (streams of the case, accepted, the referee's result on them)"""
    a = referee(r, streams)
    if a["unmatched"] < 0:
        return streams, False, a
    cut = [streams[0]] + [streams[i][:a["cur"][i]] for i in range(1, 6)]
    b = referee(r, cut)
    # (a left extension of a paired match looks ahead in the flags, :478-497: with the flags cut where reading stopped it may now run out)
    return cut, b["unmatched"] >= 0 and all(b["cur"][i] == len(cut[i]) for i in range(1, 6)), b


def _case(r, cls, seed, what, streams):
    streams, ok, res = close(r, streams)
    c = Case()
    c.row, c.cls, c.seed, c.what, c.streams, c.accepted = r.name, cls, seed, what, streams, ok
    c.expect = res["dest"] if ok else None
    c.dest_len, c.unmatched = (len(res["dest"]), res["unmatched"]) if ok else (0, -1)
    c.walk = res["walk"]
    wide = referee(r, streams, REF_MAX + DEVICE_SLACK)
    wide_ok = wide["unmatched"] >= 0 and all(wide["cur"][i] == len(streams[i]) for i in range(1, 6))
    c.slack_same = wide_ok == ok and (not ok or (wide["unmatched"] == c.unmatched and np.array_equal(wide["dest"], c.expect)))
    return c


@functools.lru_cache(maxsize=None)
def corpus(name):
    r = row(name)
    ri = [n for n, _ in ROWS].index(name)
    cases = []
    for ci, cls in enumerate(CLASSES):
        k = made = 0
        while made < PER_CLASS:
            seed = (ri, ci, k)
            rng = np.random.default_rng([ri, ci, k])
            k += 1
            assert k < 20 * PER_CLASS, (name, cls)
            if cls == "refpoke":
                # the two contigs over the poked bytes: as they are, with one repair undone (a code below 5 over a byte that is
                # none of ACGTN), with one more mutation elsewhere
                which = k % 4
                if which == 0:
                    t = Tokens(r.fixed, r.frugal)
                    l, v = r.fixes[int(rng.integers(0, len(r.fixes)))]
                    t.lit[l] = r.base[7][0][LIT][l]
                    what = ["contig 7, code %d as emitted" % l]
                else:
                    t = Tokens(r.base[6][0] if which & 1 else r.fixed, r.frugal)
                    what = ["contig %d" % (6 if which & 1 else 7)]
                    if k > 4:
                        what.append((mut_flag_flip, mut_literal, mut_length)[int(rng.integers(0, 3))](rng, t, r))
            else:
                t = Tokens(r.base[int(rng.integers(0, 6))][0], r.frugal)
                if cls == "offset":
                    _pad(rng, t, r)
                t.at_end = k % 4 == 0
                what = [MUTATORS[cls](rng, t, r) for _ in range(int(rng.integers(1, 4)))]
            if None in what:
                continue
            if cls != "offset" and k % 4:            # (one mutant in four stands alone: what reads further runs out)
                _pad(rng, t, r)
            c = _case(r, cls, seed, "; ".join(what), t.streams())
            if c.walk > 128:                          # (the device's own ring guard would have a say: not this corpus's subject)
                continue
            cases.append(c)
            made += 1
    acc = [c for c in cases if c.accepted and c.cls != "refpoke"]
    for k in range(LEFTOVER):
        rng = np.random.default_rng([ri, len(CLASSES), k])
        src = acc[int(rng.integers(0, len(acc)))]
        which = 1 + k % 5
        s = list(src.streams)
        s[which] = s[which] + bytes([int(rng.integers(0, 2))])
        c = Case()
        c.row, c.cls, c.seed, c.what, c.streams = name, "leftover", (ri, len(CLASSES), k), "%s; one byte behind %s" % (src.what, NAMES[which]), s
        res = referee(r, s)
        c.accepted = res["unmatched"] >= 0 and all(res["cur"][i] == len(s[i]) for i in range(1, 6))
        c.expect, c.dest_len, c.unmatched, c.walk, c.slack_same = (res["dest"] if c.accepted else None), (len(res["dest"]) if c.accepted else 0), \
            (res["unmatched"] if c.accepted else -1), res["walk"], True
        cases.append(c)
    return cases


def counts(cases):
    """{class: (accepted, rejected)}"""
    out = {}
    for c in cases:
        a, b = out.get(c.cls, (0, 0))
        out[c.cls] = (a + 1, b) if c.accepted else (a, b + 1)
    return out


def write_corpus(path):
    """every row and case for tests/decode_oracle_main.c: per row the emission parameters, the reference buffer, the lock position;
    per case the six streams, the verdict, destCap, destLen, unmatchedChars and the sum of the expected bytes"""
    import ctypes as C
    n = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(ROWS), C.sizeof(_orc.OrcEmitParams)))
        for name, _ in ROWS:
            r, cs = row(name), corpus(name)
            f.write(bytes(r.params))
            f.write(struct.pack("<QQI", REF_MAX, r.lock, len(cs)))
            f.write(r.ref[:REF_MAX].tobytes())
            for c in cs:
                f.write(struct.pack("<IqQQQ6Q", int(c.accepted), c.unmatched, c.dest_len, byte_sum(c.expect) if c.accepted else 0, c.dest_cap(),
                                    *[len(s) for s in c.streams]))
                for s in c.streams:
                    f.write(s)
                n += 1
    return n


def byte_sum(a):
    """position-weighted sum of the bytes (what the stand-alone program compares instead of the bytes themselves)"""
    a = np.asarray(a, dtype=np.uint64)
    return int((a * (np.arange(a.size, dtype=np.uint64) % np.uint64(65521) + np.uint64(1))).sum() & np.uint64(0xFFFFFFFFFFFFFFFF))
