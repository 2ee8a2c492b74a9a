"""Schedules and probes for the batched finalize at piece edges (swsem_finalize_targets, the applied branch of
swsem_emit_batch_begin_spec). Test infrastructure only: no GPU, no library of its own.

A Schedule is the initial load_ref, a list of finalize calls (extensions as offsets into one staging buffer, lazy, add_sep,
sep, the locks the call releases) and the rule by which probes are cut. steps() runs it call by call on a backend of
tests/_spec.py — tests/_orc_backend.OracleDeviceMatcher on host tensors, mbgc_amd.binding on HBM tensors — through one of
three routes: "batched" (finalize_targets), "single" (load_ref_dev, load_separator, release_lock target by target) and
"spec" (emit_batch_begin_spec under a prediction that holds). The oracle's run yields, per call, the loader's state before
it; model_call() restates load_pieces / load_separator / processIgnoreCollisionsRef on those figures and gives the call's
pieces, separator bytes and sample positions, and is itself held to the oracle's getters after every call.

Probes. The table image (m.ht()) holds positions only; what a lookup does with an entry's fingerprint and epoch shows in
match rows alone, and only in rows that hang on ONE sample. So after every call, for every edge of the call — each piece's
first and last byte, each separator byte, REF_SHIFT after a wrap, the window's end — and every sample position s within
K + 2 k1 of it, L bytes are cut from the oracle's buffer so that s is the only sample whose K-mer lies inside them (k1 + K >
L: asserted), flanked by two bytes that differ from the buffer's, and all of a call's probes are matched as one batch, once
without a lock and once under the lock the next round would hold. A sample off the grid (1 + 16 n behind a wrap) counts
the same way; in random text its entry sends the lookup to 16 n, the bytes differ and there is no row, in a run of one
letter there is.

Low complexity. In the second variant of every schedule each extension gets a run of one letter (N or A, changing every two
calls) of 2 K bytes around each of its boundaries: its first byte, its last byte and every place where load_pieces cuts it
(the wrap, the window's end). The runs at a cut are truly straddled; the run at an extension's first byte continues the
previous extension's last run across the piece boundary where the call has no lazy separator and both belong to calls of
the same letter, and otherwise begins at the first byte (a separator or the other letter stands in front of it).

Two geometry classes the issue names "if reachable":

  two separator bytes inside one piece of a flush: NOT reachable. pendingBytes is fed from two places. load_pieces pushes
    the byte at swEnd - 1 when a piece's copy ends exactly on swEnd — that piece's last byte, once per window end (a second
    arrival has tmpLength 0 and sep_end_done). load_separator's deferred branch pushes the byte AT the loading position and
    moves on: it lies between pieces, never inside one, and a flush never laps itself while a window is set (the window
    [pos1, swEnd) is shorter than the buffer). load_separator AT the window's end flushes what is pending and writes at once
    (k_mark_stale, k_set_byte): that byte is never in a flush's list. So a piece holds at most one byte of its flush's
    separators, its last one, and the trimming's order of pendingBytes cannot matter. That one byte is covered ("sep_inside").
  copies of one flush that overlap (beside = false): reachable, with the sliding window disabled (swEnd = 0: loadRef is
    bounded by nothing, .cpp:412-417) and one extension longer than the buffer — schedule "overlap". It showed that the
    earlier piece's samples were hashed from the later piece's bytes (table entries the oracle has were missing); the loader
    now launches what is pending before such a step (flush_if_hit), and `beside = false` stays behind it as a safeguard.
"""
import functools

import numpy as np
import torch

import _orc
import _spec

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
L, K1 = 32, 16
K_L32 = 28                     # initParams' K for L = 32 (.cpp:74-104); every handle made here is asked for its own and must agree
REF_SHIFT = 1
ROUTES = ("batched", "single", "spec")
EDGE_KINDS = ("first", "last", "sep", "shift", "wend")
NZ_SEP = ord("#")


def lengths(K):
    STEP, B = 128 * K1, 4096
    return [0, 1, K - 1, K, K + 1, K1 - 1, K1, K1 + 1, K + K1 - 1, K + K1, STEP - 1, STEP, STEP + 1, STEP + K - 1, STEP + K, STEP + K + 1,
            B - 1, B, B + 1, B + 15, 2 * B + 1]


SRC_RES = (0, 1, 7, 15)
DST_RES = ((16, 0), (16, 1), (16, 15), (4096, 0), (4096, 4095))


# ------------------------------------------------------------------------------------------------------------ schedule
class Call:
    def __init__(self, targets, lazy, add_sep, sep, hold, tags):
        self.targets, self.lazy, self.add_sep, self.sep, self.hold, self.tags = targets, bool(lazy), bool(add_sep), int(sep), bool(hold), set(tags)


class Schedule:
    def __init__(self, name, cls, lowc, max_ref, sw_factor, text, load_rc):
        self.name, self.cls, self.lowc, self.max_ref, self.sw_factor, self.text, self.load_rc = name, cls, lowc, max_ref, sw_factor, text, load_rc
        self.calls, self.chunks, self.size = [], [], 0
        self.claims = {}            # wrap / clipped (total) / at_sw_end / offgrid_and_back / short_piece: what the schedule says of itself

    def __repr__(self):
        return self.name

    @property
    def staging(self):
        out = np.zeros(max(self.size, 1) + 16, dtype=np.uint8)
        for off, a in self.chunks:
            out[off:off + a.size] = a
        return out


def _trunc_div(a, b):
    return a // b if a >= 0 else -((-a) // b)


def sample_sets(sp, pos1, K):
    """processIgnoreCollisionsRef (.cpp:146-171) for a loader at pos1 with sampling position sp: -> (main, tail, new sp)"""
    STEP = 128 * K1
    E = pos1 - K
    main = range(0)
    if sp < E - STEP:
        blocks = ((E - STEP) - sp + STEP - 1) // STEP
        main = range(sp, sp + blocks * STEP, K1)
    T = K1 + _trunc_div(E - 1, STEP) * STEP
    tail = range(T, E + 1, K1) if T < E + 1 else range(0)
    return main, tail, T + len(tail) * K1


def model_call(pre, lens, lazy, add_sep, K):
    """load_pieces / load_separator (.cpp:402-451) for the targets of one call, from the state before it. -> dict: pieces
    [(lo, hi, target)], seps [positions written], wrapped, clipped (bytes given up), at_sw_end (the loader stood on swEnd),
    offgrid [sample positions off the grid], off_then_on (sampling left the grid and returned), covered [samples inside a piece
    whose K-mer holds the separator at that piece's last byte], declined (a speculative finalize of the call cannot be queued:
    its lazy separator overwrites the last loaded byte at the window's end), pos / sp after the call"""
    pos, sp, sw_end, max_ref = pre["pos"], pre["sp"], pre["sw_end"], pre["max_ref"]
    out = dict(pieces=[], seps=[], wrapped=False, clipped=0, at_sw_end=False, offgrid=[], off_then_on=False, covered=[], declined=False)
    was_off, sep_done = False, False          # sep_done: the byte in front of swEnd already is this call's separator (sep_end_done)

    def wrap():
        nonlocal pos, sp
        if pos == max_ref and sw_end != max_ref:
            pos, sp = REF_SHIFT, REF_SHIFT
            out["wrapped"] = True

    for t, n in enumerate(lens):
        while n:
            wrap()
            tmp_max = max_ref if sw_end < pos else sw_end
            take = min(n, tmp_max - pos)
            if take:
                out["pieces"].append((pos, pos + take, t))
            lo = pos
            sep_write = add_sep and pos + take == sw_end and not (take == 0 and sep_done)
            if sep_write:
                out["seps"].append(sw_end - 1)
                sep_done = True
            pos += take
            main, tail, sp = sample_sets(sp, pos, K)
            if sep_write and take:
                # samples of this step that lie in the piece and whose K-mer holds the separator: the reference hashes them with the
                # separator in place (.cpp:418-424), the copy's source still has the text's byte there (prepare_inserts trims)
                out["covered"] += [s for s in range(max(lo, sw_end - K), sw_end) if s in main or s in tail]
            if len(main) and main[0] % K1:
                out["offgrid"] += list(main)
                was_off = True
            if was_off and sp % K1 == 0:
                out["off_then_on"] = True
            if pos == sw_end:
                out["clipped"] += n - take
                out["at_sw_end"] = True
                n = 0
            else:
                n -= take
        if lazy:
            wrap()
            if pos == max_ref:
                pass
            elif pos == sw_end:
                out["at_sw_end"] = True
                if not sep_done:              # written at once over a byte already loaded: cannot be queued behind a gate
                    out["seps"].append(pos - 1)
                    out["declined"] = True
                    sep_done = True
            else:
                out["seps"].append(pos)
                pos += 1
    out["pos"], out["sp"] = pos, sp
    return out


def loader_state(o):
    return dict(pos=int(o.loading_position()), sp=int(o.sampling_position()), sw_end=int(o.sw_end()), max_ref=int(o.max_ref_length()),
                laps=int(o.laps()), dropped=int(o.dropped_bytes()))


# ------------------------------------------------------------------------------------------------------------- running
def _stage(backend, sched):
    """the staging buffer in the backend's memory, its first byte on a 16-byte boundary"""
    a = sched.staging
    t = backend.zeros(a.size + 16)
    shift = (-t.data_ptr()) % 16
    t[shift:shift + a.size] = backend.tensor(a)
    backend.sync()
    return t, t.data_ptr() + shift


def steps(sched, backend, route="batched"):
    """runs the schedule call by call: yields (call index, call, m, loaded-after array, state before the call or None, applied).
    The handle is closed when the generator ends."""
    m = backend.make(sched.max_ref)
    if sched.sw_factor:
        m.set_sliding_window_size(sched.sw_factor)
    else:
        m.disable_sliding_window()
    m.load_ref(sched.text, load_rc=sched.load_rc)
    keep, base = _stage(backend, sched)
    is_oracle = not backend.cuda
    rng = np.random.default_rng(5)
    loaded = [int(m.loading_position())]
    try:
        for ci, call in enumerate(sched.calls):
            n = len(call.targets)
            locks = [int(m.acquire_lock()) for _ in range(n + call.hold)]
            use = locks[call.hold:]
            pre = loader_state(m.o) if is_oracle and hasattr(m, "o") and hasattr(m.o, "sw_end") else None
            ptrs = [base + off if ln else 0 for off, ln in call.targets]
            lens = [ln for _, ln in call.targets]
            applied = None
            if route == "batched" or is_oracle:
                after = m.finalize_targets(ptrs, lens, use, lazy=call.lazy, add_sep=call.add_sep, sep=call.sep)
            elif route == "single":
                after = []
                for p, ln, lk in zip(ptrs, lens, use):
                    if ln:
                        m.load_ref_dev(p, ln, False, call.add_sep, call.sep)
                    if call.lazy:
                        m.load_separator(call.sep)
                    after.append(int(m.loaded_ref_length()))
                    assert m.release_lock(lk) == 0
            else:
                # a round whose contigs the reference knows nothing of: unmatchedChars = their length, the extension and its
                # reverse complement are both "proper" (x128, x8) and predicted so — the finalize is applied unless the library
                # finds it cannot be queued behind a gate (a separator over the last loaded byte at the window's end)
                contigs = ACGT[rng.integers(0, 4, (n, 64))].astype(np.uint8)
                q = backend.tensor(contigs.reshape(-1))
                offs = np.arange(n + 1, dtype=np.uint64) * 64
                backend.sync()
                m.match_batch_dev(q.data_ptr(), offs, L, use)
                applied, after = m.emit_batch_begin_spec(backend.params(), use, [_spec.EMIT_FACTOR] * n, [n] * n, list(range(n)), loaded, n, ptrs, lens,
                                                         use, [1] * n, [1] * n, 128, 8, lazy=call.lazy, add_sep=call.add_sep, sep=call.sep)
                un = [int(x) for x in m.emit_unmatched(n)]
                assert un == [64] * n, un
                if not applied:
                    after = m.finalize_targets(ptrs, lens, use, lazy=call.lazy, add_sep=call.add_sep, sep=call.sep)
                m.emit_batch_end()
            if call.hold:
                assert m.release_lock(locks[0]) == 0
            after = [int(x) for x in after]
            loaded += after
            yield ci, call, m, after, pre, applied
    finally:
        m.close()
        del keep


class Probe:
    __slots__ = ("kind", "edge", "s", "at", "offgrid", "text", "sampled")

    def __init__(self, kind, edge, s, at, offgrid, text, sampled):
        # sampled: False for a grid position whose K-mer spans the loading position — new bytes in front of it, the last lap's behind:
        # the loader's arithmetic has put no sample on THESE bytes yet (E = pos1 - K, .cpp:146-171). Such a probe is still matched
        # on both sides (a stale entry may sit there) but is no "sample position" of the statistics.
        self.kind, self.edge, self.s, self.at, self.offgrid, self.text, self.sampled = kind, edge, s, at, offgrid, text, sampled

    def __repr__(self):
        return "%s edge at %d, sample %d%s, probe cut at reference position %d" % (self.kind, self.edge, self.s, " (off the grid)" if self.offgrid else "", self.at)


def edges_of(model, pre):
    e = []
    for lo, hi, _ in model["pieces"]:
        e += [("first", lo), ("last", hi - 1)]
    e += [("sep", s) for s in model["seps"]]
    if model["wrapped"]:
        e.append(("shift", REF_SHIFT))
    if pre["sw_end"] and model["pos"] + K1 >= pre["sw_end"] >= model["pos"]:
        e.append(("wend", pre["sw_end"]))
    return e


def cut_probes(ref, ref_len, pos, edges, offgrid, K):
    """one probe per (edge kind, sample) near the call's edges, cut from the oracle's buffer `ref`"""
    assert K1 + K > L, "a window of L bytes could hold two samples' K-mers"
    D = K + 2 * K1
    seen, out = set(), []
    for kind, e in edges:
        for s in range(max(e - D, REF_SHIFT), e + D + 1):
            off = s % K1 != 0
            if (off and s not in offgrid) or s + K > ref_len or (kind, s) in seen:
                continue
            seen.add((kind, s))
            at = s if off else s - (s >> 4) % (L - K + 1)     # (off the grid: the slot's first byte, a grid position, stays outside)
            if not off and at + L > pos >= s + K:                    # the text ends inside the probe: cut it to end with the text
                at = max(pos - L, s - (L - K))
            at = max(at, 0)
            if at + L > ref_len:
                at = ref_len - L
            if not (at <= s and s + K <= at + L):
                continue
            left = ACGT[(np.searchsorted(ACGT, ref[at - 1]) + 1) & 3] if at > 0 else ACGT[0]
            nxt = ref[at + L] if at + L < ref.size else 0
            right = ACGT[(np.searchsorted(ACGT, nxt) + 1) & 3]
            if at > 0 and left == ref[at - 1]:
                left = ACGT[(np.searchsorted(ACGT, left) + 1) & 3]
            if right == nxt:
                right = ACGT[(np.searchsorted(ACGT, right) + 1) & 3]
            text = np.concatenate(([left], ref[at:at + L], [right])).astype(np.uint8)
            out.append(Probe(kind, e, s, at, off, text, not (pos - K < s < pos)))
    return out


def match_probes(backend, m, probes, lock):
    """all probes as short contigs of one match_batch_dev -> list of row arrays"""
    if not probes:
        return []
    q = backend.tensor(np.concatenate([p.text for p in probes]))
    offs = np.arange(len(probes) + 1, dtype=np.uint64) * (L + 2)
    backend.sync()
    m.match_batch_dev(q.data_ptr(), offs, L, None if lock is None else [lock] * len(probes))
    counts = m.batch_counts()
    return [np.asarray(m.batch_matches(i, counts[i]), dtype=np.uint64).reshape(-1, 3) for i in range(len(probes))]


def next_lock(m):
    lk = int(m.acquire_lock())
    assert m.release_lock(lk) == 0
    return lk


def has_exact_row(rows, p):
    return any(int(r[1]) == L for r in rows)       # (in a run of one letter the row may lie at another position of the run)


class OracleRun:
    """the oracle's run of a schedule, call by call, with the model, the edges and the probes of every call"""

    def __init__(self, sched):
        self.sched, self.backend = sched, _spec.OracleBackend()
        self.offgrid = set()

    def __iter__(self):
        K = None
        for ci, call, m, after, pre, _ in steps(self.sched, self.backend):
            K = K or int(m.K())
            model = model_call(pre, [ln for _, ln in call.targets], call.lazy, call.add_sep, K)
            post = loader_state(m.o)
            what = "%s call %d" % (self.sched.name, ci)
            assert (model["pos"], model["sp"]) == (post["pos"], post["sp"]), "%s: the model of the loader ends at %r, the oracle at %r" % (
                what, (model["pos"], model["sp"]), (post["pos"], post["sp"]))
            assert post["dropped"] - pre["dropped"] == model["clipped"], what
            self.offgrid.update(model["offgrid"])
            ref_len = int(m.ref_length())
            ref = m.ref(int(m.max_ref_length()))
            edges = edges_of(model, pre)
            probes = cut_probes(ref, ref_len, post["pos"], edges, self.offgrid, K)
            yield dict(ci=ci, call=call, m=m, after=after, pre=pre, post=post, model=model, edges=edges, probes=probes, K=K)


# ----------------------------------------------------------------------------------------------------------- building
class Builder:
    """builds a schedule against a live oracle, so that a call's lengths can be worked out from where the loader stands"""

    def __init__(self, name, cls, lowc, max_ref, sw_factor, init_len, seed, load_rc=False):
        self.rng = np.random.default_rng(seed)
        text = ACGT[self.rng.integers(0, 4, init_len)].astype(np.uint8)
        if lowc:
            text[-2 * K_L32 - 8:] = ord("N")
        self.s = Schedule(name + ("_lowc" if lowc else ""), cls, lowc, max_ref, sw_factor, text, load_rc)
        self.o = _orc.OracleMatcher(max_ref)
        if sw_factor:
            self.o.set_sliding_window_size(sw_factor)
        else:
            self.o.disable_sliding_window()
        self.o.load_ref(text, load_rc=load_rc)
        self.K = int(self.o.K())
        assert self.K == K_L32

    pos = property(lambda self: int(self.o.loading_position()))
    max_ref = property(lambda self: int(self.o.max_ref_length()))
    sw_size = property(lambda self: int(self.o.sliding_window_size()))

    def call(self, lens, lazy=1, add_sep=1, sep=0, hold=False, src_res=None, tags=()):
        """lens: a list, or f(pos, sw_end, max_ref) -> list, asked once the call's locks are held"""
        o, s = self.o, self.s
        probe = [int(o.acquire_lock())]
        at = self.pos
        if at == self.max_ref and int(o.sw_end()) != self.max_ref:
            at = REF_SHIFT                                    # (the first load of the call begins the next lap)
        lens = lens(at, int(o.sw_end()), self.max_ref) if callable(lens) else list(lens)
        n = len(lens)
        locks = probe + [int(o.acquire_lock()) for _ in range(n + bool(hold) - 1)]
        use = locks[bool(hold):]
        pre = loader_state(o)
        model = model_call(pre, lens, lazy, add_sep, self.K)
        letter = ord("N") if (len(s.calls) // 2) % 2 == 0 else ord("A")
        sep = letter if sep == "letter" else sep
        targets = []
        for t, ln in enumerate(lens):
            res = (src_res if src_res is not None else (0, 1, 7, 15)[(len(s.calls) + t) % 4]) if ln else 0
            off = s.size + (res - s.size) % 16
            a = ACGT[self.rng.integers(0, 4, ln)].astype(np.uint8)
            if s.lowc and ln:
                cuts, at = [0, ln], 0
                for lo, hi, tt in model["pieces"]:
                    if tt == t:
                        at += hi - lo
                        cuts.append(at)
                for c in cuts:
                    a[max(c - 2 * self.K, 0):c + 2 * self.K] = letter
            if ln:
                s.chunks.append((off, a))
                s.size = off + ln
            targets.append((off if ln else 0, ln))
            if ln:
                o.load_ref(a, False, bool(add_sep), sep)
            if lazy:
                o.load_separator(sep)
            assert o.release_lock(use[t]) == 0
        if hold:
            assert o.release_lock(locks[0]) == 0
        assert self.pos == model["pos"], (s.name, len(s.calls))
        s.calls.append(Call(targets, lazy, add_sep, sep, hold, tags))
        return model

    def fill_to(self, target, per_call=3):
        """filler calls (random text, no separators) until the loader stands at `target`, wrapping on the way if it lies behind"""
        guard = 0
        while self.pos != target:
            guard += 1
            assert guard < 200, (self.s.name, self.pos, target)

            def lens(pos, sw_end, max_ref):
                goal = target if target > pos else max_ref
                room = goal - pos
                if pos < sw_end:                              # the window's end lies ahead: stay short of it
                    room = min(room, sw_end - pos - 64)
                assert room > 0, (self.s.name, pos, sw_end, target)
                cut = [int(x) for x in sorted(self.rng.integers(0, room + 1, per_call - 1))]
                return [y - x for x, y in zip([0] + cut, cut + [room])]
            self.call(lens, lazy=0, add_sep=1, tags=("filler",))

    def done(self, **claims):
        self.s.claims.update(claims)
        self.o.close()
        return self.s


def _flags(i):
    """lazy, add_sep, sep cycling through all combinations"""
    return dict(lazy=i & 1, add_sep=(i >> 1) & 1, sep=NZ_SEP if (i >> 2) & 1 else 0)


def _build(lowc):
    out = []
    LENS = lengths(K_L32)

    # every length alone in a call / as the middle of three (lap 0 of a 2^18-byte buffer: the window ends on the buffer's end)
    b = Builder("lengths_alone", "alone", lowc, 1 << 18, 16, 5000, 11)
    for i, ln in enumerate(LENS):
        b.call([ln], tags=("alone:%d" % ln, "n:1"), **_flags(i))
    out.append(b.done(short_piece=True))
    b = Builder("lengths_middle", "alone", lowc, 1 << 18, 16, 3001, 12)
    for i, ln in enumerate(LENS):
        b.call([100 + 7 * i, ln, 333 - i], tags=("middle:%d" % ln,) + (("zero:middle",) if ln == 0 else ()), **_flags(i + 3))
    out.append(b.done(short_piece=True))

    # source and destination residues: a filler target in front moves the loading position
    b = Builder("alignment", "alone", lowc, 1 << 18, 16, 2000, 13)
    i = 0
    for sres in SRC_RES:
        for mod, dres in DST_RES:
            ln = (4096 + 15, 2049, 45, 4096)[i % 4]
            b.call(lambda pos, e, mx, mod=mod, dres=dres, ln=ln: [(dres - pos) % mod, ln], lazy=i & 1, add_sep=1, src_res=sres,
                   tags=("src:%d" % sres, "dst:%d/%d" % (dres, mod)))
            i += 1
    out.append(b.done())

    # one, two, five and 40 targets per call, zero-length extensions first, middle and last
    b = Builder("calls", "alone", lowc, 1 << 18, 16, 4000, 14)
    i = 0
    for n in (1, 2, 5, 40):
        for zero in (None, "first", "middle", "last"):
            if n == 1 and zero:
                continue
            lens = [int(x) for x in b.rng.integers(1, 3000 if n < 40 else 700, n)]
            lens[int(b.rng.integers(0, n))] = (27, 2049, 16, 4097)[i % 4]
            if zero:
                lens[{"first": 0, "middle": n // 2, "last": n - 1}[zero]] = 0
            fl = _flags(i)
            b.call(lens, tags=("n:%d" % n, "lazy:%d" % fl["lazy"], "add_sep:%d" % fl["add_sep"], "sep:%s" % ("nz" if fl["sep"] else "0")) +
                   (("zero:" + zero,) if zero else ()), **fl)
            i += 1
    out.append(b.done(short_piece=True))

    # the window's end (lap 1 of a 2^16-byte buffer, a window of a sixteenth): one byte short of swEnd, exactly on it, a byte over it;
    # the front lock released by the call's own targets, or held by somebody else through the call; a later target finds the window full
    b = Builder("window_end", "window_end", lowc, 1 << 16, 16, 40_000, 15)
    b.fill_to(b.max_ref)
    clipped = 0
    i = 0
    covered = []

    def align():
        # the window's end is the loading position + 4096 when the locks are taken: with the position at 12 modulo 16 the sample at
        # swEnd - K is on the grid, lies inside the piece that reaches swEnd and has the separator as its K-mer's last byte
        b.call(lambda pos, e, mx: [(12 - pos) % 16 + 16], lazy=0, tags=("filler",))
    for hold in (False, True):
        for delta in (-1, 0, 1):
            for lazy in (0, 1):
                align()

                def lens(pos, e, mx, delta=delta):
                    room = e - pos
                    return [500, room - 500 + delta, 77, 0, 1]
                m = b.call(lens, lazy=lazy, add_sep=1, sep=NZ_SEP if i % 3 == 0 else 0, hold=hold,
                           tags=("wend:%+d" % delta, "wend:held" if hold else "wend:released", "wend:full_later") +
                           (("sep_inside",) if delta >= 0 else ()))
                assert m["at_sw_end"] and m["clipped"] > 0          # (the 77 bytes of the third target at the least)
                assert m["covered"] or delta < 0, (delta, lazy)     # (delta -1 with a lazy separator behind the first target ends ON swEnd too)
                covered += m["covered"]
                clipped += m["clipped"]
                i += 1
    b.call(lambda pos, e, mx: [e - pos], lazy=1, add_sep=0, tags=("wend:+0", "sep_over_last_byte"))      # the lazy separator alone overwrites the last byte
    # the separator equals the letter of the run the piece ends in: in the low-complexity variant the sample at swEnd - K (an edge
    # run: its K-mer holds the separator) and the tail's sample at swEnd - K - k1 (hashed from the source) have the same K-mer, and
    # only the epoch of the edge run (the tail's: epoch + 1) lets the later one keep the bucket as it does in the reference
    # The piece that reaches swEnd is the call's LAST step. (Every step re-inserts the tail of its 2048-byte block from the buffer,
    # .cpp:157: in the calls above the targets that find the window full do, and put the sample at swEnd - K right whatever
    # the piece's own insertion did.) Its K-mer and the text's differ in the last byte only, which the hash folds above a 2^24-entry
    # table's index: same bucket, same position, another fingerprint — the table image cannot tell, a probe can, once the loader
    # has moved on (the reference's window refuses a candidate that ends on the loading position). The call behind it starts with
    # more than 2048 bytes, so its own tail begins in a later block and leaves that sample alone.
    align()
    m = b.call(lambda pos, e, mx: [500, e - pos - 500], lazy=0, add_sep=1, sep=NZ_SEP, tags=("wend:+0", "sep_inside", "sep_inside_last_step"))
    covered += m["covered"]
    assert m["covered"] == [b.pos - K_L32]
    b.call(lambda pos, e, mx: [2048 + (12 - pos) % 16 + 16], lazy=0, tags=("filler",))
    m = b.call(lambda pos, e, mx: [500, e - pos - 500], lazy=0, add_sep=1, sep="letter", tags=("wend:+0", "sep_inside", "epoch_decides"))
    covered += m["covered"]
    e = b.pos
    r = b.o.ref(b.max_ref)
    assert m["covered"] == [e - K_L32] and (not lowc or bytes(r[e - K_L32 - K1:e - K1]) == bytes(r[e - K_L32:e]))
    b.call([2100, 300], lazy=1, tags=("filler",))
    out.append(b.done(wrap=True, clipped=clipped, at_sw_end=True, covered=len(covered)))

    # the buffer's end: an extension that ends exactly on it (the next piece starts at REF_SHIFT and is short: sampling is on the
    # grid at once), then round again and one that straddles it (two pieces, the second long: off the grid, then back)
    b = Builder("buffer_end", "buffer_end", lowc, 1 << 16, 4, 50_000, 16)
    b.fill_to(b.max_ref - 5000)
    b.call(lambda pos, e, mx: [1000, mx - pos - 1000], lazy=0, tags=("bend:exact",))
    assert b.pos == b.max_ref
    b.call([300, 28, 1], lazy=1, tags=("bend:short_after",))
    b.fill_to(b.max_ref - 3000)
    m = b.call(lambda pos, e, mx: [500, mx - pos - 500 + 6000, 100], lazy=1, tags=("bend:straddle",))
    assert m["wrapped"] and m["offgrid"] and len([p for p in m["pieces"] if p[2] == 1]) == 2
    for _ in range(3):
        b.call([700, 0, 2049], lazy=1, tags=("bend:back_on_grid",))
    assert b.o.sampling_position() % K1 == 0
    out.append(b.done(wrap=True, offgrid_and_back=True, short_piece=True))

    # three times round the buffer
    b = Builder("three_laps", "buffer_end", lowc, 1 << 16, 4, 30_000, 17)
    for lap in range(3):
        b.fill_to(b.max_ref - 2000 - 100 * lap, per_call=5)
        b.call(lambda pos, e, mx, lap=lap: [mx - pos + (5000, 40, 2500)[lap], 10], lazy=lap & 1, sep=NZ_SEP if lap == 1 else 0, tags=("bend:straddle", "laps"))
        b.call([100, 3000], tags=("laps",))
    assert b.o.laps() == 3
    out.append(b.done(wrap=True, offgrid_and_back=True, laps=3))

    # copies of one flush that overlap: no sliding window, one extension longer than the buffer
    b = Builder("overlap", "overlap", lowc, 1 << 16, 0, 20_000, 18)
    b.call([70_000], lazy=1, tags=("overlap",))
    b.call([300, 66_000, 5], lazy=0, tags=("overlap",))
    b.fill_to(b.max_ref)
    b.call([300, 40], lazy=1, tags=("bend:short_after",))      # (a short piece at REF_SHIFT: its samples are on the grid)
    out.append(b.done(wrap=True))
    return out


@functools.lru_cache(maxsize=None)
def schedules():
    """every schedule by name, random text and the low-complexity variant of each (deterministic)"""
    S = {}
    for lowc in (False, True):
        for s in _build(lowc):
            assert s.name not in S
            S[s.name] = s
    return S


SPEC_SCHEDULES = ("lengths_alone", "window_end", "window_end_lowc", "buffer_end", "lengths_middle_lowc", "buffer_end_lowc")


# ------------------------------------------------------------------------------------------------- the device's side
def tag_invariant(m, what):
    """test_gpu_tag_summary.py's invariant: a block the summary calls uniform holds that tag in all of its slots"""
    if not (hasattr(m, "tag_summary") and hasattr(m, "tags")):
        return
    s, sh = m.tag_summary()
    if not s.size:
        return
    from test_gpu_tag_summary import check_invariant
    check_invariant(m, what)


def hold_to_oracle(sched, backend, route):
    """the schedule on `backend` through `route`, held to the oracle's run after every call -> (calls, probes, calls applied)"""
    n_probes, n_applied, n_calls, n_declined = 0, 0, 0, 0
    dev = steps(sched, backend, route)
    try:
        for rec, (ci, call, m, after, _, applied) in zip(OracleRun(sched), dev):
            what = "%s, call %d, route %s" % (sched.name, ci, route)
            o = rec["m"]
            a, b = _spec.snapshot(m), _spec.snapshot(o)
            for f in _spec.STATE_FIELDS:
                if a[f] is not None and b[f] is not None:
                    assert a[f] == b[f], "%s: %s is %r, the oracle's %r" % (what, f, a[f], b[f])
            sw = getattr(m, "sliding_window_size", None)
            if sw is not None and hasattr(o, "sliding_window_size"):
                assert int(sw()) == int(o.sliding_window_size()), what
            assert after == rec["after"], "%s: loaded-after %r, the oracle's %r" % (what, after, rec["after"])
            for f in ("ref", "ht"):
                # (the reference allocates its buffer without clearing it: what lies behind the loaded text is nobody's)
                n = a["ref_length"] if f == "ref" and backend.name == "reference" else a[f].size
                d = np.nonzero(a[f][:n] != b[f][:n])[0]
                assert d.size == 0, "%s: %s differs from the oracle's in %d places, the first at %d (%r, expected %r); pieces %r, separators %r" % (
                    what, f, d.size, d[0], a[f][d[0]], b[f][d[0]], rec["model"]["pieces"], rec["model"]["seps"])
            for lock in (None, a["next_lock"]):
                want = match_probes(_spec.OracleBackend(), o, rec["probes"], lock)
                got = match_probes(backend, m, rec["probes"], lock)
                for p, w, g in zip(rec["probes"], want, got):
                    assert np.array_equal(w, g), "%s, %s: %s: rows %r, the oracle's %r" % (
                        what, "no lock" if lock is None else "lock %d" % lock, p, g.tolist(), w.tolist())
            tag_invariant(m, what)
            n_probes += 2 * len(rec["probes"])
            n_applied += bool(applied)
            n_declined += rec["model"]["declined"]
            n_calls += 1
    finally:
        dev.close()
    assert n_calls == len(sched.calls)
    if route == "spec" and backend.cuda:
        # every call is applied but those the loader cannot queue behind a gate (the model knows them: load_separator over the
        # last loaded byte at the window's end); none of these schedules laps its own flush (flush_if_hit)
        assert n_applied == n_calls - n_declined, "%s: %d of %d calls applied, %d expected" % (sched.name, n_applied, n_calls, n_calls - n_declined)
    return n_calls, n_probes, n_applied
