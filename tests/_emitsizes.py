"""The corpus of the emission's size-picked write paths (tests/test_emit_size_classes_cpu.py proves on the oracle that it is what
it says, tests/test_gpu_emit_size_classes.py holds the device to the oracle on it). Pure numpy, everything from fixed seeds.

The second phase of the emission (k_emit_sizes, k_emit_write, k_emit_copy_long; launched by run_phase2b) picks device code by a
size alone at six places. The constants that decide, restated (the CPU test holds every one of them to the sources):"""
import functools

import numpy as np

EMIT_THIN_MAX = 512      # mbgc_amd/csrc/swsem_runtime_state.h:22   chunks up to which <4> (1024 threads, 16 tasks per wave) runs, beyond: <1>
CH = 256                 # mbgc_amd/csrc/swsem_emit.hip:140         gap tasks per chunk (chunk_task: gx * 256, swsem_emit.hip:1169)
LONG_COPY_CAP = 4096     # mbgc_amd/csrc/swsem_emit.hip:50          entries of the list k_emit_copy_long works off
LONG_COPY_MIN = 32768    # mbgc_amd/csrc/swsem_emit.hip:51          plain run from which it is listed (z[4] >= LONG_COPY_MIN, :1420)
EXT_WIDE_MIN = 192       # mbgc_amd/csrc/swsem_emit.hip:908         litLeft > EXT_WIDE_MIN: the wave's ext_right_wide / ext_left_wide (:1145, :1217, :1430)
PLAIN_INLINE = 48        # mbgc_amd/csrc/swsem_emit.hip:1389        z[4] <= PLAIN_INLINE: the thread's own byte loop (:1417)
PIECE = 16384            # mbgc_amd/csrc/swsem_emit.hip:1485        bytes of a listed run one block of k_emit_copy_long takes at a time
# (seven names: the five thresholds of the issue's table, the chunk size they are counted in and the copy's piece)

MIN_LEN = 32             # the matching length L of every case (match_batch_dev's minLen: rows are reserved per n / minLen)
REF_LEN = 400_000
BIG_REF_LEN = 4_400_000
RUN_CAP = 24             # a related stretch keeps no run of equal bases longer than this (K = 28 for L = 32): no match inside it


def chunks_of(n, min_len=MIN_LEN):
    """chunks of CH gap tasks a contig of n bases is given: rows nm = n / minLen + 2, cap = nm + 2, ceil(cap / CH)
    (emit_layout, mbgc_amd/csrc/swsem_runtime_emit.h:53-60)"""
    return (n // min_len + 4 + CH - 1) // CH


def expected_thin(contigs):
    """run_phase2b (mbgc_amd/csrc/swsem_runtime_loader.h:78): the batch's chunks, all contigs, against EMIT_THIN_MAX"""
    return sum(chunks_of(int(c.size)) for c in contigs) <= EMIT_THIN_MAX


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def ref_codes():
    return np.random.default_rng(20_001).integers(0, 4, REF_LEN).astype(np.uint8)


def reference():
    """400 000 random ACGT bases (loaded with load_rc=False, L = 32, everything else at its default)"""
    return ACGT[ref_codes()]


@functools.lru_cache(maxsize=None)
def big_ref_codes():
    """the reference of `beside_big`: the small one and 4 000 000 more bases behind it, so the positions of the small one stay"""
    return np.concatenate([ref_codes(), np.random.default_rng(20_002).integers(0, 4, BIG_REF_LEN - REF_LEN).astype(np.uint8)])


def big_reference():
    return ACGT[big_ref_codes()]


def _unrelated(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _substituted(rng, seg, rate):
    """seg (codes) with substitutions — always by another base — at `rate`, and at every position that would end a run of more
    than RUN_CAP kept bases"""
    out = seg.copy()
    mask = rng.random(seg.size) < rate
    last = -1
    for i in range(seg.size):
        if mask[i]:
            last = i
        elif i - last > RUN_CAP:
            mask[i] = True
            last = i
    out[mask] = (out[mask] + rng.integers(1, 4, int(mask.sum())).astype(np.uint8)) & 3
    return out


def _other(rng, *avoid):
    """a code that is none of `avoid` (at most two of them; None: no constraint)"""
    ok = [c for c in range(4) if c not in [int(a) for a in avoid if a is not None]]
    return ok[int(rng.integers(0, len(ok)))]


def _per_stretch(x, n):
    return list(x) if isinstance(x, (list, tuple)) else [x] * n


def ladder_contig(lengths, piece=200, related=None, seed=0, side="right", related_len=None):
    """stretch, piece, stretch, ..., piece, stretch: len(lengths) stretches of the given lengths around len(lengths) - 1 pieces of
    the reference (`piece` bases each, from scattered offsets in no particular order: no two neighbours on one diagonal).
    related=None: a stretch is unrelated random bases. related=rate (one, or one per stretch): it copies the reference's
    continuation of the piece in front (side="right"; "left": what the reference has in front of the piece behind) with that
    substitution rate, its first related_len bytes (one, or one per stretch; "left": its last) or all of it — so the extension
    into it runs long and may cross it whole. The first byte of every stretch differs from the reference's byte behind the piece in
    front, the last from the byte in front of the piece behind: the matches end exactly where the pieces do."""
    R = ref_codes()
    m = len(lengths)
    rates, rlens = _per_stretch(related, m), _per_stretch(related_len, m)
    margin = 3_100                                                     # a related part is at most this long
    slots = np.arange(margin, R.size - margin - piece, piece + 56)
    assert m - 1 <= slots.size
    for attempt in range(100):
        rng = np.random.default_rng([seed, attempt, 77])
        offs = [int(x) for x in rng.permutation(slots)[: m - 1]]
        if all(offs[i + 1] - offs[i] != piece + int(lengths[i + 1]) for i in range(m - 2)):
            break
    else:
        raise AssertionError("no placement without two neighbours on one diagonal")
    parts = []
    for i, n in enumerate(lengths):
        n = int(n)
        front = offs[i - 1] if i >= 1 else None                       # piece in front of the stretch, piece behind it
        behind = offs[i] if i < m - 1 else None
        s = _unrelated(rng, n)
        rl = n if rlens[i] is None else min(n, int(rlens[i]))
        assert rates[i] is None or rl <= margin
        if rates[i] is not None and side == "right" and front is not None:
            s[:rl] = _substituted(rng, R[front + piece: front + piece + rl], rates[i])
        if rates[i] is not None and side == "left" and behind is not None:
            s[n - rl:] = _substituted(rng, R[behind - rl: behind], rates[i])
        a = R[front + piece] if front is not None else None
        b = R[behind - 1] if behind is not None else None
        if n == 1:
            s[0] = _other(rng, a, b)
        elif n > 1:
            if a is not None and s[0] == a:
                s[0] = _other(rng, a)
            if b is not None and s[-1] == b:
                s[-1] = _other(rng, b)
        parts.append(s)
        if behind is not None:
            parts.append(R[behind: behind + piece])
    return ACGT[np.concatenate(parts)]


def gap_contig(lengths, piece=200, related=None, seed=0):
    """the same on one diagonal: piece, stretch, piece, ..., stretch, piece as a copy of one region of the reference with every
    stretch substituted in place, its length kept — consecutive matches pair into gaps (isGap)"""
    R = ref_codes()
    rng = np.random.default_rng([seed, 78])
    total = piece * (len(lengths) + 1) + int(sum(lengths))
    o = int(rng.integers(1, R.size - total - 1))
    g = R[o: o + total].copy()
    at = piece
    for n in lengths:
        n = int(n)
        orig = g[at: at + n].copy()
        s = _unrelated(rng, n) if related is None else _substituted(rng, orig, related)
        for k in {0, n - 1}:
            if s[k] == orig[k]:
                s[k] = _other(rng, orig[k])
        g[at: at + n] = s
        at += n + piece
    return ACGT[g]


# ---- the case sets -----------------------------------------------------------------------------------------------------------
# a run of plain literals on both sides of PLAIN_INLINE, of one and two vectors of 16 bytes with and without a byte tail, of a
# round of the wave copy (64 lanes x 16 bytes = 1 024), of PIECE and of LONG_COPY_MIN, LONG_COPY_MIN + PIECE, and two long ones
# whose length is no multiple of 16
PLAIN_LENGTHS = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1_023, 1_024, 1_039, 16_383, 16_384, 16_385, 32_767, 32_768, 32_769,
                 32_768 + 16_384 - 1, 32_768 + 16_384, 32_768 + 16_384 + 1, 49_153 + 15, 100_003]
DENSE_LOW = list(range(30, 121))
DENSE_HIGH = list(range(LONG_COPY_MIN - 96, LONG_COPY_MIN + 97))
DENSE_HIGH_PARTS = 3                                                   # (one contig of them all would not be thin by itself)
WIDE_LENGTHS = [150] + list(range(185, 261)) + [500, 3_000]
WIDE_RATES = (0.08, 0.25)
LANES_HARD = (15, 16, 17, 63, 64, 65, 255, 256, 257)                   # gap tasks: last lane of a <4> wave and first of the next, of a <1> wave, of a chunk
LANES_TASKS = 260
LANES_RELATED, LANES_UNRELATED = 3_000, 40_000
ZERO_LENGTHS = [1, 31, 48, 49, 32_767, 32_768, 32_769, 1_000_003]


def plain_contigs(seed=0):
    """PLAIN_EXACT / PLAIN_EXT: the list, and the list in reverse order (the runs then start at other offsets modulo 16)"""
    return {"plain_fwd_%d" % seed: ladder_contig(PLAIN_LENGTHS, seed=100 + 2 * seed),
            "plain_rev_%d" % seed: ladder_contig(PLAIN_LENGTHS[::-1], seed=101 + 2 * seed)}


def dense_contigs():
    """PLAIN_EXT: every stretch length around both thresholds, whatever the extensions take off the ends"""
    out = {"dense_low": ladder_contig(DENSE_LOW, seed=110)}
    for k in range(DENSE_HIGH_PARTS):
        out["dense_high_%d" % k] = ladder_contig(DENSE_HIGH[k::DENSE_HIGH_PARTS], seed=111 + k)
    return out


def wide_contigs(seed=0):
    """WIDE: per rate a ladder whose stretches continue the piece in front, one whose stretches lead up to the piece behind (the
    left extension's long walk) and a gap contig"""
    out = {}
    for r in WIDE_RATES:
        tag = "%03d_%d" % (round(100 * r), seed)
        out["wide_ladder_" + tag] = ladder_contig(WIDE_LENGTHS, related=r, seed=120 + 10 * seed)
        out["wide_left_" + tag] = ladder_contig(WIDE_LENGTHS, related=r, seed=121 + 10 * seed, side="left")
        out["wide_gap_" + tag] = gap_contig(WIDE_LENGTHS, related=r, seed=122 + 10 * seed)
    return out


def lanes_contig():
    """LANES: the hard stretches (3 000 bases related at 0.08, then 40 000 unrelated: a wide right extension, a wide left one and
    a listed run in one task) are gap tasks LANES_HARD by the count of pieces in front of them; every other stretch is 40 bases"""
    lengths = [LANES_RELATED + LANES_UNRELATED if t in LANES_HARD else 40 for t in range(LANES_TASKS)]
    rates = [0.08 if t in LANES_HARD else None for t in range(LANES_TASKS)]
    return {"lanes": ladder_contig(lengths, related=rates, related_len=LANES_RELATED, seed=130)}


def zero_contigs():
    """ZERO: unrelated bases, no match at all — one task whose plain run is the contig"""
    return {"zero_%d" % n: ACGT[_unrelated(np.random.default_rng([140, n]), n)] for n in ZERO_LENGTHS}


@functools.lru_cache(maxsize=None)
def hard_contigs():
    """name -> contig, every contig of PLAIN_*, WIDE, LANES and ZERO"""
    out = {}
    for part in (plain_contigs(), dense_contigs(), wide_contigs(), lanes_contig(), zero_contigs()):
        out.update(part)
    return out


def _mutant(codes, rate, seed):
    rng = np.random.default_rng(seed)
    out = codes.copy()
    mask = rng.random(codes.size) < rate
    out[mask] = (out[mask] + rng.integers(1, 4, int(mask.sum())).astype(np.uint8)) & 3
    return out


@functools.lru_cache(maxsize=None)
def fillers():
    """600 contigs of 40-300 bases cut from a 1 % mutant of the reference: a chunk each, more than EMIT_THIN_MAX by count"""
    rng = np.random.default_rng(150)
    mut = ACGT[_mutant(ref_codes(), 0.01, 151)]
    out = {}
    for i in range(600):
        n, a = int(rng.integers(40, 301)), int(rng.integers(0, REF_LEN - 300))
        out["filler_%d" % i] = mut[a: a + n].copy()
    return out


@functools.lru_cache(maxsize=None)
def big_contig():
    """4 400 000 bases 2 % from the large reference: more than EMIT_THIN_MAX chunks by itself"""
    return ACGT[_mutant(big_ref_codes(), 0.02, 152)]


ALONE = {"alone_plain": ("plain_", "dense_low"), "alone_dense_0": ("dense_high_0",), "alone_dense_1": ("dense_high_1",),
         "alone_dense_2": ("dense_high_2",), "alone_wide": ("wide_",), "alone_lanes": ("lanes",), "alone_zero": ("zero_",)}


def batches():
    """-> list of dict(name, kind, ref ("small" / "big"), names, contigs, expected_thin): every hard contig `alone` (by itself or
    a handful together: thin), in the `crowd` (scattered among the fillers: not thin by count) and `beside_big` (behind one
    contig that is not thin by itself, against the large reference: the hard contigs' blocks lie at chunk indices above
    EMIT_THIN_MAX)"""
    hard, fill = hard_contigs(), fillers()
    out = []

    def add(name, kind, ref, pairs):
        names, contigs = [p[0] for p in pairs], [p[1] for p in pairs]
        out.append(dict(name=name, kind=kind, ref=ref, names=names, contigs=contigs, expected_thin=expected_thin(contigs)))

    seen = set()
    for name, prefixes in ALONE.items():
        pairs = [(k, v) for k, v in hard.items() if k.startswith(prefixes)]
        seen.update(p[0] for p in pairs)
        add(name, "alone", "small", pairs)
    assert seen == set(hard), "a hard contig that is in no `alone` batch"
    rng = np.random.default_rng(160)
    pairs = list(fill.items())
    for k, v in hard.items():                                          # scattered: each at a place of its own among the fillers
        pairs.insert(int(rng.integers(0, len(pairs) + 1)), (k, v))
    add("crowd", "crowd", "small", pairs)
    add("beside_big", "beside_big", "big", [("big", big_contig())] + list(hard.items()))
    return out


OVERFLOW_RUNS = 4_300
OVERFLOW_MIXED = 20


def overflow_batch():
    """-> the same kind of dict: 4 300 contigs of unrelated bases, 32 768 + (i mod 37) long — more runs of at least LONG_COPY_MIN
    than the list holds in one emission — and twenty PLAIN and WIDE contigs (other seeds among them) at fixed positions; about
    141 MB of query. Which runs get listed is the atomic counter's choice and differs from run to run; the bytes may not."""
    mixed = {}
    for seed in (0, 1, 2, 3):
        mixed.update(plain_contigs(seed))
    for seed in (0, 1):
        mixed.update(wide_contigs(seed))
    mixed = list(mixed.items())[:OVERFLOW_MIXED]
    assert len(mixed) == OVERFLOW_MIXED
    lens = [LONG_COPY_MIN + i % 37 for i in range(OVERFLOW_RUNS)]
    pool = ACGT[_unrelated(np.random.default_rng(170), sum(lens))]
    pairs, at = [], 0
    for i, n in enumerate(lens):
        pairs.append(("run_%d" % i, pool[at: at + n]))
        at += n
        if i % 215 == 107:                                             # 20 fixed places
            pairs.append(mixed[i // 215])
    names, contigs = [p[0] for p in pairs], [p[1] for p in pairs]
    return dict(name="overflow", kind="overflow", ref="small", names=names, contigs=contigs, expected_thin=expected_thin(contigs))


# ---- the oracle on this corpus (the only part that is not numpy: tests/_orc.py, imported when asked for) -----------------------
PARAMS = ((1, 1, 1), (1, 0, 1), (0, 1, 1), (3, 1, 1), (1, 1, 0))      # (mode, lazyDecompressionSupport, enableExtensionsWithMismatches)
COUNTERS = ("extensionsMatchedChars", "extensionsMismatches", "totalMatched", "removedGapBreakingMatches")


def params_key(mode, lazy, ext, **over):
    """hashable (mode, overrides) of an emission's parameters; params_of makes the structure for either side"""
    over.update(lazyDecompressionSupport=int(lazy), enableExtensionsWithMismatches=int(ext))
    return int(mode), tuple(sorted(over.items()))


def params_of(factory, key):
    return factory(key[0], **dict(key[1]))


class Referee:
    """The oracle on one reference: a contig's rows once (matching does not depend on the emission's parameters) and its streams
    once per parameter set, shared by every test that asks and left unchanged."""

    def __init__(self, ref, max_ref_len, sliding_window=None):
        import _orc
        self.orc = _orc
        self.o = _orc.OracleMatcher(max_ref_len)
        if sliding_window is not None:
            self.o.set_sliding_window_size(sliding_window)
        self.o.load_ref(ref, load_rc=False)
        self.loaded = [self.o.loading_position()]
        self._rows, self._out = {}, {}

    def rows(self, name, contig, lock=None):
        lock = self.orc.NO_LOCK if lock is None else lock
        if (name, lock) not in self._rows:
            self._rows[name, lock] = self.o.match(contig, MIN_LEN, lock)
        return self._rows[name, lock]

    def emit(self, name, contig, key, lock=None):
        """-> dict(unmatched, streams (by name), counters, rows: the rows as processMatches left them — gap-breaking matches
        removed, their successors extended to the left)"""
        import ctypes as C
        orc = self.orc
        lock = orc.NO_LOCK if lock is None else lock
        if (name, key, lock) not in self._out:
            m = self.rows(name, contig, lock)
            oe = orc.OracleEmitter(self.o, params_of(orc.emit_params, key))
            a = np.ascontiguousarray(contig, dtype=np.uint8)
            n = len(m)
            rows = np.zeros((max(n, 1), 4), dtype=np.uint64)
            rows[:n, :3] = m
            nn = C.c_uint64(n)
            ld = np.ascontiguousarray(self.loaded, dtype=np.uint64)
            un = orc.lib().orc_process_matches(self.o.h, C.byref(oe.p), C.cast(rows.ctypes.data_as(C.c_void_p), C.POINTER(orc.OrcMatch)),
                                               C.byref(nn), a.ctypes.data_as(C.c_void_p), a.size, lock, 128, 0, 0,
                                               ld.ctypes.data_as(C.c_void_p), ld.size, C.byref(oe.s))
            self._out[name, key, lock] = dict(unmatched=int(un), streams=oe.streams(), counters=oe.counters(), rows=rows[: nn.value, :3].copy())
        return self._out[name, key, lock]


def stretches(rows, n):
    """what lies in front of, between and behind the rows of a contig of n bases: len(rows) + 1 lengths"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    ends = np.concatenate([[0], r[:, 2] + r[:, 1]])
    starts = np.concatenate([r[:, 2], [n]])
    return [int(x) for x in starts - ends]
