"""The corpus of the decoder's size-picked fill paths and of its plan's register windows (tests/test_decode_size_classes_cpu.py
proves on the oracle that it is what it says, tests/test_gpu_decode_size_classes.py holds the device decoder to it). Pure numpy,
everything from fixed seeds; the reference is the 400 000 random bases of tests/_emitsizes.py, loaded without its reverse complement.

k_decode_fill (decode_fill_body, mbgc_amd/csrc/swsem_decode.hip) picks code by a size at three places, k_decode_plan (plan_contig)
reads every stream through a register window. The constants that decide, restated (the CPU test holds each to the sources):"""
import functools

import numpy as np

import _decmut
import _emitsizes as E

DEC_WIDE_MIN = 192       # swsem_decode.hip   plain <= / r.len <= / r.rightLen > DEC_WIDE_MIN: the thread's loop, beyond it the wave's
FILL_THREADS = 256       # swsem_decode.hip, swsem_runtime_decode.h   threads of a block of k_decode_fill: one record each, four waves
WAVE = 64                # swsem_device.h     lanes of a wave: a ballot window is 64 bytes of the literals (marks) or of the flags
DW_WINDOW = 256          # swsem_decode.hip   bytes of a dword window (4 * WAVE): mapLen, mapOff, mapOff5th, gapDelta
COPY_ROUND = 1024        # swsem_decode.hip   bytes of one round of the wave copy (16 * WAVE), 16 bytes per lane

MARK = _decmut.MARK
REF_MAX = 4_000_000      # what the handle and the oracle's matcher are made for
REF_LEN = E.REF_LEN
LIT, OFF, OFF5, LEN, GAP, FLAGS = range(6)
PLAIN_ALPHABET = np.frombuffer(b"ACGTNacgtnRYKMSW", dtype=np.uint8)   # what a run of plain literals may hold: anything but the mark


def ref_buffer():
    """the matcher's buffer after load_ref(reference, load_rc=False): the text from position 1 on (REF_SHIFT), zeros around it"""
    b = np.zeros(REF_MAX, dtype=np.uint8)
    b[1:1 + REF_LEN] = E.reference()
    return b


# ---- family A: written by hand ------------------------------------------------------------------------------------------------
# (name, overrides of mode 1's parameters with enableExtensionsWithMismatches = 0, flip frugal64bitLenEncoding)
A_SETS = (("m1", {}, False), ("m1-plainlen", {}, True), ("m1-bit40", {"enable40bitReference": 1}, False))
PLAIN_LONG = (1_023, 1_024, 1_025, 1_039, 1_040, 1_041, 2_047, 2_048, 2_049, 100_003)
MATCH_LONG = (1_023, 1_024, 1_025, 1_039, 1_040, 1_041, 2_047, 2_048, 2_049, 65_534, 65_535, 65_536, 70_001)
LEN_WINDOW_AT = (125, 126, 127, 128, 129)
LEN_WINDOW_RECORDS, LEN_WINDOW_LONG = 260, 70_001
LANES_RECORDS, LANES_WIDE = 520, (0, 63, 64, 65, 255, 256, 257, 511)
LANES_FULL_RECORDS, LANES_FULL_WIDE = 200, tuple(range(64, 128))
PAIRS_RECORDS = 1_200
TINY_TAILS = (0, 1, 192, 193, 5_000)
TINY_NREC = (2, 64, 65, 256, 257)


class Hand:
    """a contig written token by token: recs = [(plain bytes, src, len)], tail = the plain bytes behind the last match; paired =
    the records that take their source from the record in front (its gapDelta is 1) and have no offset in the streams"""

    def __init__(self, name, recs, tail, paired=()):
        self.name, self.recs, self.tail, self.paired = name, recs, tail, frozenset(paired)
        self.nrec = len(recs) + 1                                         # (the tail's pseudo-record)

    def unmatched(self):
        return sum(len(p) for p, _, _ in self.recs) + len(self.tail)

    def expect(self, ref):
        """concat(plain_i, ref[src_i : src_i + len_i]) + tail: numpy alone, no decoder"""
        parts = []
        for p, s, n in self.recs:
            parts += [np.frombuffer(p, dtype=np.uint8), ref[s:s + n]]
        parts.append(np.frombuffer(self.tail, dtype=np.uint8))
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)

    def streams(self, frugal, bit40):
        """the six streams as oracle/decode_oracle.c reads them with the extensions off: per match its plain literals and a mark, a
        4-byte offset (and its fifth byte), a mapLen entry and — for every match but the contig's last — a gapDelta: 0 (the next
        match reads an offset of its own) or 1 (the next match lies on this one's diagonal and reads none); no flags"""
        t = _decmut.Tokens([b""] * 6, frugal)
        start, at = [], 0
        for i, (p, s, n) in enumerate(self.recs):
            assert MARK not in p
            t.lit += p + bytes([MARK])
            at += len(p)
            start.append(at)
            at += n
            if i in self.paired:                                          # matchSrcPos = the pair's source - its place + this match's place
                assert i > 0 and s == self.recs[i - 1][1] + start[i] - start[i - 1]
            else:
                t.offs.append(s & 0xFFFFFFFF)
                if bit40:
                    t.off5.append(s >> 32)
            t.lens.append(n)
        assert MARK not in self.tail
        t.lit += self.tail
        t.gap += bytes(1 if i + 1 in self.paired else 0 for i in range(len(self.recs) - 1))
        return t.streams()


def _plain(rng, n):
    return PLAIN_ALPHABET[rng.integers(0, PLAIN_ALPHABET.size, n)].tobytes()


def _src(rng, n, mod16=None):
    """where a match of n bases starts in the buffer: inside the loaded text, src % 16 as asked"""
    s = int(rng.integers(1, REF_LEN - n - 32))
    if mod16 is not None:
        s += (mod16 - s) % 16
    assert 1 <= s and s + n <= 1 + REF_LEN
    return s


@functools.lru_cache(maxsize=None)
def hand_contigs():
    """name -> Hand, every contig of family A"""
    out = []
    rng = np.random.default_rng(30_001)
    dense = list(range(0, 261))
    for tag, order in (("fwd", dense), ("rev", dense[::-1])):             # the reverse order starts every run at another destination alignment
        out.append(Hand("plain_dense_" + tag, [(_plain(rng, n), _src(rng, 40), 40) for n in order], _plain(rng, 7)))
    out.append(Hand("plain_long", [(_plain(rng, n), _src(rng, 40), 40) for n in PLAIN_LONG[:-1]], _plain(rng, PLAIN_LONG[-1])))
    out.append(Hand("plain_long_rev", [(_plain(rng, n), _src(rng, 40), 40) for n in PLAIN_LONG[::-1][:-1]], _plain(rng, PLAIN_LONG[0])))
    lens = list(range(1, 261))
    out.append(Hand("match_dense_fwd", [(_plain(rng, 3), _src(rng, n, n % 16), n) for n in lens], _plain(rng, 3)))
    out.append(Hand("match_dense_rev", [(_plain(rng, 3), _src(rng, n, (7 * n + 3) % 16), n) for n in lens[::-1]], _plain(rng, 3)))
    out.append(Hand("match_long", [(_plain(rng, 3), _src(rng, n), n) for n in MATCH_LONG], _plain(rng, 3)))
    for at in LEN_WINDOW_AT:
        recs = [(_plain(rng, 2), _src(rng, 40), 40) for _ in range(LEN_WINDOW_RECORDS)]
        recs.insert(at, (_plain(rng, 2), _src(rng, LEN_WINDOW_LONG), LEN_WINDOW_LONG))
        out.append(Hand("len_window_%d" % at, recs, _plain(rng, 5)))
    out.append(Hand("lanes", [((_plain(rng, 1_000), _src(rng, 1_000), 1_000) if i in LANES_WIDE else (_plain(rng, 3), _src(rng, 40), 40))
                              for i in range(LANES_RECORDS)], _plain(rng, 3)))
    # every lane of the second wave has a wide run and a wide match, no two of a length (the ballot loop runs 64 times, twice)
    out.append(Hand("lanes_full", [((_plain(rng, 193 + 13 * (i - 64)), _src(rng, 193 + 29 * (i - 64)), 193 + 29 * (i - 64)) if i in LANES_FULL_WIDE
                                    else (_plain(rng, 3), _src(rng, 40), 40)) for i in range(LANES_FULL_RECORDS)], _plain(rng, 3)))
    # gapDelta bytes that differ from window to window: about half of the records continue the diagonal of the one in front
    recs, paired = [], set()
    for i in range(PAIRS_RECORDS):
        if i and i - 1 not in paired and (i == DW_WINDOW + 1 or (i != 1 and rng.integers(0, 2))) and recs[-1][1] + 43 + 40 <= REF_LEN:
            recs.append((_plain(rng, 3), recs[-1][1] + 40 + 3, 40))
            paired.add(i)
        else:
            recs.append((_plain(rng, 3), _src(rng, 40), 40))
    out.append(Hand("pairs", recs, _plain(rng, 3), paired))
    for n in TINY_TAILS:
        out.append(Hand("tiny_tail_%d" % n, [], _plain(rng, n)))
    for nrec in TINY_NREC:
        out.append(Hand("tiny_nrec_%d" % nrec, [(_plain(rng, 3), _src(rng, 40), 40) for _ in range(nrec - 1)], _plain(rng, 5)))
    assert len({h.name for h in out}) == len(out)
    return {h.name: h for h in out}


def a_params(factory, name):
    """the parameter structure of a family A set, made by either side's factory (_orc.emit_params / binding.emit_params)"""
    over, flip = {n: (o, f) for n, o, f in A_SETS}[name]
    p = factory(1, enableExtensionsWithMismatches=0, **over)
    if flip:
        p.frugal64bitLenEncoding = 0 if p.frugal64bitLenEncoding else 1
    return p


# ---- family B: written by the oracle's encoder ---------------------------------------------------------------------------------
B_SETS = (("m1", E.params_key(1, 1, 1)), ("m1-eager", E.params_key(1, 0, 1)), ("m0", E.params_key(0, 1, 1)))
PIECE = 200
STRETCH_LENGTHS = [150] + list(range(185, 261)) + [1_023, 1_024, 1_025, 3_000]
SINGLES = (1, 63, 64, 65, 127, 128, 129)
# pattern -> the further substituted offsets of a stretch of n bytes (0 and n - 1 are always substituted)
PATTERNS = [("none", lambda rng, n: []), ("every", lambda rng, n: range(n)), ("mod64", lambda rng, n: [k for k in range(n) if k % 64 in (0, 1, 63)])]
PATTERNS += [("single%d" % s, (lambda s: lambda rng, n: [s] if s < n else [])(s)) for s in SINGLES]
PATTERNS += [("rate%02d" % round(100 * r), (lambda r: lambda rng, n: _capped(rng, n, r))(r)) for r in (0.08, 0.25)]
DENSE_PATTERNS = ("every", "rate08", "rate25")       # no run of more than E.RUN_CAP kept bases: the matcher finds the pieces and nothing else
FOREIGN_LONG, FOREIGN_SHORT = 260, 40                # a planted piece of at least gapBreakingMatchMinLength (256) stays a match, a shorter one is removed
B_LANES_RECORDS, B_LANES_WIDE, B_LANES_WIDE_LEN = 260, (0, 63, 64, 255, 256), 1_000


def _capped(rng, n, rate):
    """offsets at `rate` and wherever a run of more than E.RUN_CAP kept bases would end (as _emitsizes._substituted)"""
    mask = rng.random(n) < rate
    last = -1
    for i in range(n):
        if mask[i]:
            last = i
        elif i - last > E.RUN_CAP:
            mask[i] = True
            last = i
    return [int(i) for i in np.flatnonzero(mask)]


class Gap:
    """a copy of one region of the reference with stretches substituted in place: pieces and stretches alternate, a piece in front
    and behind. rows: the pieces as matches (posSrcText in the buffer, length, posDestText) — what the emitter is given.
    stretches: (offset in the contig, length, the record in front of it) per stretch; planted: foreign pieces, by record index."""

    def __init__(self, name, contig, rows, stretches, planted=(), removed=0):
        self.name, self.contig, self.rows, self.stretches, self.planted, self.removed = name, contig, rows, stretches, tuple(planted), removed


def _substitute(rng, g, R, o, at, n, offsets):
    for k in sorted(set(offsets) | {0, n - 1}):
        g[at + k] = E._other(rng, R[o + at + k])


def gap_contig(name, lengths, pattern, seed, piece=PIECE):
    """piece, stretch, piece, ..., stretch, piece on one diagonal"""
    R = E.ref_codes()
    rng = np.random.default_rng([seed, 79])
    total = piece * (len(lengths) + 1) + int(sum(lengths))
    o = int(rng.integers(1, R.size - total - 1))
    g = R[o:o + total].copy()
    rows, stretches, at = [(1 + o, piece, 0)], [], piece
    for i, n in enumerate(lengths):
        _substitute(rng, g, R, o, at, int(n), pattern(rng, int(n)))
        stretches.append((at, int(n), i))
        at += int(n)
        rows.append((1 + o + at, piece, at))
        at += piece
    return Gap(name, E.ACGT[g], np.array(rows, dtype=np.uint64), stretches)


def planted_contig(name, lengths, foreign, seed, piece=PIECE):
    """the same with a foreign piece (cut elsewhere in the reference) in the middle of every stretch, lengths kept: stretch =
    part, foreign piece, part — both parts substituted at 8 % (run-capped), the bytes around the foreign piece differing from what
    the reference has around the place it was cut from. The records: piece, foreign, piece, foreign, ..."""
    R = E.ref_codes()
    rng = np.random.default_rng([seed, 80])
    total = piece * (len(lengths) + 1) + int(sum(lengths))
    o = int(rng.integers(1, R.size // 2 - total - 1))                     # (the region in the first half, the foreign pieces from the second)
    g = R[o:o + total].copy()
    rows, stretches, planted, at = [(1 + o, piece, 0)], [], [], piece
    for i, n in enumerate(lengths):
        n = int(n)
        a = (n - foreign) // 2
        b = n - foreign - a
        assert a >= 2 and b >= 2
        f = int(rng.integers(R.size // 2 + 1, R.size - foreign - 1))
        _substitute(rng, g, R, o, at, a, _capped(rng, a, 0.08))
        g[at + a - 1] = E._other(rng, R[o + at + a - 1], R[f - 1])
        g[at + a:at + a + foreign] = R[f:f + foreign]
        _substitute(rng, g, R, o, at + a + foreign, b, _capped(rng, b, 0.08))
        g[at + a + foreign] = E._other(rng, R[o + at + a + foreign], R[f + foreign])
        stretches.append((at, a, len(rows) - 1))
        planted.append(len(rows))
        rows.append((1 + f, foreign, at + a))
        stretches.append((at + a + foreign, b, len(rows) - 1))
        at += n
        rows.append((1 + o + at, piece, at))
        at += piece
    return Gap(name, E.ACGT[g], np.array(rows, dtype=np.uint64), stretches, planted, removed=len(planted) if foreign < 256 else 0)


@functools.lru_cache(maxsize=None)
def gap_contigs():
    """name -> Gap, every contig of family B"""
    out = []
    for k, (tag, pat) in enumerate(PATTERNS):
        out.append(gap_contig("gap_" + tag, STRETCH_LENGTHS, pat, 200 + k))
    # parts of (n - foreign) / 2 bytes on either side of a planted piece: both sides of DEC_WIDE_MIN, a round of the wave's 64, long
    lengths = [2 * a + FOREIGN_LONG for a in (150, 185, 190, 191, 192, 193, 194, 200, 255, 256, 257, 1_024, 3_000)]
    out.append(planted_contig("planted_long", lengths + [n + 1 for n in lengths], FOREIGN_LONG, 230))
    out.append(planted_contig("planted_short", [2 * a + FOREIGN_SHORT for a in (150, 191, 192, 193, 1_024)], FOREIGN_SHORT, 231))
    rate08 = dict(PATTERNS)["rate08"]
    out.append(gap_contig("gap_lanes", [B_LANES_WIDE_LEN if i in B_LANES_WIDE else 40 for i in range(B_LANES_RECORDS)], rate08, 232, piece=60))
    return {c.name: c for c in out}


class Referee(E.Referee):
    """the oracle on the reference; a contig's streams from rows that are given (the pieces), not matched"""

    def emit_rows(self, gap, key):
        import ctypes as C
        orc = self.orc
        k = ("rows", gap.name, key)
        if k not in self._out:
            oe = orc.OracleEmitter(self.o, E.params_of(orc.emit_params, key))
            a = np.ascontiguousarray(gap.contig, dtype=np.uint8)
            n = len(gap.rows)
            rows = np.zeros((n, 4), dtype=np.uint64)
            rows[:, :3] = gap.rows
            nn = C.c_uint64(n)
            ld = np.ascontiguousarray(self.loaded, dtype=np.uint64)
            un = orc.lib().orc_process_matches(self.o.h, C.byref(oe.p), C.cast(rows.ctypes.data_as(C.c_void_p), C.POINTER(orc.OrcMatch)),
                                               C.byref(nn), a.ctypes.data_as(C.c_void_p), a.size, orc.NO_LOCK, 128, 0, 0,
                                               ld.ctypes.data_as(C.c_void_p), ld.size, C.byref(oe.s))
            self._out[k] = dict(unmatched=int(un), streams=[oe.stream(i) for i in range(6)], counters=oe.counters(), rows=rows[:nn.value, :3].copy())
        return self._out[k]


@functools.lru_cache(maxsize=None)
def referee():
    return Referee(E.reference(), REF_MAX)
