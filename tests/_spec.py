"""Scenario driver for the speculative finalize (swsem_emit_batch_begin_spec, include/mbgc_swsem.h): the same round run
twice from identical starting state on two handles —

  plain        match_batch_dev, emit_batch_begin, emit_unmatched, finalize_targets
  speculative  match_batch_dev, emit_batch_begin_spec (and finalize_targets when it reports "not applied")

— with the state (the WHOLE reference buffer, the hash-table image, the loader's positions, the next lock) taken before
and after every step that may change it. The header's promise is what check() asserts: applied = the finalize has been
done, exactly as the plain one does it; not applied = nothing has changed, device or host. The verdict that is expected
is worked out here from the plain path's emit_unmatched alone, never from what the library says about its speculation.

A backend is the device (mbgc_amd.binding, torch tensors in HBM) or the CPU oracle behind the same surface
(tests/_orc_backend.py, torch tensors in host memory): the scenarios are proven on the second (test_spec_contract_cpu.py)
before the first is held to them (test_gpu_spec_finalize.py). Test infrastructure only."""
import contextlib
import functools

import numpy as np
import torch

import _orc
from mbgc_amd import synth

SKIPPED = 2 ** 64 - 1
MIN_LEN = 32
EMIT_FACTOR = 128          # unmatchedFractionFactor of processMatches (the dissimilarity early-out); the speculation's factors are the round's
STATE_FIELDS = ("ref_length", "loading_position", "loaded_ref_length", "dropped_bytes", "next_lock")


# ---------------------------------------------------------------------------------------------------------- backends
class OracleBackend:
    name, cuda = "oracle", False

    def make(self, max_ref):
        import _orc_backend
        return _orc_backend.OracleDeviceMatcher(max_ref)

    def params(self): return _orc.emit_params(1)
    def tensor(self, a): return torch.from_numpy(np.array(a, copy=True))
    def zeros(self, n, dtype=torch.uint8): return torch.zeros(n, dtype=dtype)
    def host_word(self): return torch.zeros(1, dtype=torch.int32)
    def sync(self): pass


class DeviceBackend:
    name, cuda = "device", True

    def __init__(self, binding):
        self.b = binding

    def make(self, max_ref): return self.b.SlidingWindowSparseEMMatcher(max_ref)
    def params(self): return self.b.emit_params(1)
    def tensor(self, a): return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")
    def zeros(self, n, dtype=torch.uint8): return torch.zeros(n, dtype=dtype, device="cuda:0")
    def host_word(self): return torch.zeros(1, dtype=torch.int32).pin_memory()
    def sync(self): torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- scenarios
class Decision:
    """what the caller hands to the speculative finalize for one round"""

    def __init__(self, pred_ext, pred_rc, factor, rc_factor):
        self.pred_ext, self.pred_rc, self.factor, self.rc_factor = [int(x) for x in pred_ext], [int(x) for x in pred_rc], int(factor), int(rc_factor)


class Round:
    """contigs: one per target. pred_ext / pred_rc: the caller's prediction per contig; the targets' extension strings follow
    from it (the contig, then its reverse complement: MGMP.cpp:393-398). processed: processedTargetsCount per contig — by
    default the number of targets, which keeps the dissimilarity early-out (MBGC_Encoder.cpp:203) away. exchange: None (one
    replica, no callbacks), "keep" (callbacks that leave the word alone) or "zero" (another replica said no). derive(un,
    lens) -> Decision replaces the static prediction where it has to follow from pass 1's own figures (the threshold)."""

    def __init__(self, contigs, pred_ext, pred_rc=None, factor=128, rc_factor=8, processed=None, veto=False, exchange=None, sep=0, derive=None):
        n = len(contigs)
        self.contigs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]
        self.lens = [int(c.size) for c in self.contigs]
        self.static = Decision(pred_ext, pred_rc if pred_rc is not None else [0] * n, factor, rc_factor)
        self.processed = [n] * n if processed is None else list(processed)
        self.target_idx = list(range(n))
        self.veto, self.exchange, self.sep, self.derive = veto, exchange, sep, derive

    def decide(self, un):
        return self.derive(un, self.lens) if self.derive is not None else self.static

    def expected(self, dec, un):
        """the verdict, from the plain path's unmatchedChars (Python integers: the products do not wrap)"""
        word = 0 if self.exchange == "zero" else 1
        return (not self.veto) and word != 0 and all(
            u != SKIPPED and (u * dec.factor > ln) == bool(pe) and (u * dec.rc_factor > ln) == bool(prc)
            for u, ln, pe, prc in zip(un, self.lens, dec.pred_ext, dec.pred_rc))


class Scenario:
    """ref: the first file (loaded with its reverse complement). max_ref: the buffer's size, or a function of the loading
    position the reference leaves behind. want: the verdict per round the scenario is built for (None = not prescribed).
    pipelined: a round's streams are taken after the next round's emission has begun (two in flight). facts(plain) asserts
    what the scenario claims about itself, from the plain path's results."""

    def __init__(self, name, ref, rounds, want, max_ref=1 << 21, sw_factor=16, pipelined=False, facts=None):
        self.name, self.ref, self.rounds, self.want = name, ref, rounds, list(want)
        self.max_ref, self.sw_factor, self.pipelined, self.facts = max_ref, sw_factor, pipelined, facts
        rng = np.random.default_rng(len(name) + 1000)
        last = rounds[-1].contigs
        self.probe = [mutate(last[0], 5, rng), mutate(last[-1], 3, rng), ref[1000:6000].copy()]

    def __repr__(self):
        return self.name

    def buffer_size(self, backend):
        if not callable(self.max_ref):
            return self.max_ref
        t = backend.make(4 * self.ref.size + (1 << 20))
        t.set_sliding_window_size(self.sw_factor)
        t.load_ref(self.ref, load_rc=True)
        pos0 = int(t.loading_position())
        t.close()
        return self.max_ref(pos0)


# ------------------------------------------------------------------------------------------------------------ driver
def snapshot(m, full=True):
    """full: every emission is waited for first (the gated copies run on a stream of their own; the debug hooks wait for the
    main stream, which the finalize joins them to). Not full (two emissions in flight): the main stream only."""
    m.synchronize()
    if full:
        m.emit_batch_end()
        m.synchronize()
    lk = int(m.acquire_lock())
    assert m.release_lock(lk) == 0
    dropped = getattr(m, "dropped_bytes", None)
    return dict(ref=m.ref(int(m.max_ref_length())), ht=m.ht(), ref_length=int(m.ref_length()), loading_position=int(m.loading_position()),
                loaded_ref_length=int(m.loaded_ref_length()), dropped_bytes=int(dropped()) if dropped is not None else None, next_lock=lk)


def assert_state_equal(a, b, what):
    for f in STATE_FIELDS:
        assert a[f] == b[f], "%s: %s is %r, expected %r" % (what, f, a[f], b[f])
    for f in ("ref", "ht"):
        d = np.nonzero(a[f] != b[f])[0]
        assert d.size == 0, "%s: %s differs in %d places, the first at %d (%r, expected %r)" % (what, f, d.size, d[0], a[f][d[0]], b[f][d[0]])


class Extensions:
    """the targets' extension strings in the backend's memory: the contig in place in the query buffer when only the forward
    strand is loaded, otherwise built in a buffer of their own (reverse complement by the handle's revcomp_dev)"""

    def __init__(self, backend, m, q, offs, rnd, dec):
        self.ptrs, self.lens = [], []
        need = sum(ln * (pe + prc) for ln, pe, prc in zip(rnd.lens, dec.pred_ext, dec.pred_rc) if prc)
        self.buf = backend.zeros(max(need, 1))
        at, rc_jobs = 0, []
        for k, (ln, pe, prc) in enumerate(zip(rnd.lens, dec.pred_ext, dec.pred_rc)):
            src = q.data_ptr() + int(offs[k])
            if not pe and not prc:
                self.ptrs.append(0), self.lens.append(0)
            elif not prc:
                self.ptrs.append(src), self.lens.append(ln)
            else:
                self.ptrs.append(self.buf.data_ptr() + at), self.lens.append(ln * (pe + prc))
                if pe:
                    self.buf[at:at + ln] = q[int(offs[k]):int(offs[k]) + ln]
                    at += ln
                rc_jobs.append((src, ln, self.buf.data_ptr() + at))
                at += ln
        backend.sync()
        for src, ln, dst in rc_jobs:
            m.revcomp_dev(src, ln, dst)
        m.synchronize()


class Exchange:
    """the callbacks of a caller with several replicas, after RoundRunner._reduce_gate: phase 0 queues the word's reduction
    on the stream it is given (here: nothing, or "another replica said no") and its copy to the host; phase 1 returns it"""

    def __init__(self, backend, m, mode):
        self.backend, self.m, self.mode = backend, m, mode
        self.gate, self.host, self.ev = backend.zeros(1, torch.int32), backend.host_word(), None
        self.phases, self.ref_at_phase0 = [], None

    def reduce(self, stream):
        self.phases.append(0)
        self.ref_at_phase0 = self.m.ref(int(self.m.max_ref_length()))          # nothing gated has been queued yet
        if not (self.backend.cuda and stream):
            if self.mode == "zero":
                self.gate.zero_()
            self.host.copy_(self.gate)
            return
        # The word changes on the handle's stream, between the check and the launches it gates. Its copy to the host is
        # ordered behind that by an event but runs on torch's own stream: torch's allocator of page-locked memory records an
        # event on every stream a block was used on when the block is freed, and the handle's stream is gone by then if the
        # handle was closed first.
        with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
            if self.mode == "zero":
                self.gate.zero_()
            reduced = torch.cuda.Event()
            reduced.record()
        cur = torch.cuda.current_stream()
        cur.wait_event(reduced)
        self.host.copy_(self.gate, non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(cur)

    def verdict(self):
        self.phases.append(1)
        if self.ev is not None:
            self.ev.synchronize()
        return int(self.host[0])

    def kwargs(self):
        return dict(gate=self.gate.data_ptr(), reduce=self.reduce, verdict=self.verdict)


class RoundResult:
    pass


class PathResult:
    def __init__(self, m):
        self.m, self.rounds, self.keep = m, [], []


def _fetch(m, n):
    return [m.emit_result(k)[:2] for k in range(n)]


def run_path(backend, scn, decisions=None):
    """decisions None: the plain path (and the rounds' decisions come out of it); otherwise the speculative path under them"""
    spec = decisions is not None
    m = backend.make(scn.buffer_size(backend))
    m.set_sliding_window_size(scn.sw_factor)
    m.load_ref(scn.ref, load_rc=True)
    p = backend.params()
    loaded = [int(m.loading_position())]
    out = PathResult(m)
    full = not scn.pipelined
    for r, rnd in enumerate(scn.rounds):
        n = len(rnd.contigs)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(rnd.lens)
        q = backend.tensor(np.concatenate(rnd.contigs))
        out.keep.append(q)
        backend.sync()
        locks = [int(m.acquire_lock()) for _ in range(n)]
        m.match_batch_dev(q.data_ptr(), offs, MIN_LEN, locks)
        rec = RoundResult()
        rec.exchange = None
        if not spec:
            m.emit_batch_begin(p, None, locks, [EMIT_FACTOR] * n, rnd.processed, rnd.target_idx, loaded, n=n)
            rec.un = [int(x) for x in m.emit_unmatched(n)]
            rec.decision = rnd.decide(rec.un)
            ext = Extensions(backend, m, q, offs, rnd, rec.decision)
            rec.before = snapshot(m, full)
            after = m.finalize_targets(ext.ptrs, ext.lens, locks, lazy=True, add_sep=True, sep=rnd.sep)
            rec.applied = None
        else:
            rec.decision = dec = decisions[r]
            ext = Extensions(backend, m, q, offs, rnd, dec)
            rec.before = snapshot(m, full)
            kw = {}
            if rnd.exchange is not None:
                rec.exchange = Exchange(backend, m, rnd.exchange)
                kw = rec.exchange.kwargs()
            rec.applied, after = m.emit_batch_begin_spec(p, locks, [EMIT_FACTOR] * n, rnd.processed, rnd.target_idx, loaded, n, ext.ptrs, ext.lens, locks,
                                                         dec.pred_ext, dec.pred_rc, dec.factor, dec.rc_factor, lazy=True, add_sep=True, sep=rnd.sep,
                                                         veto=rnd.veto, **kw)
            rec.un = [int(x) for x in m.emit_unmatched(n)]
            rec.after_call = snapshot(m, full)
            if not rec.applied:
                after = m.finalize_targets(ext.ptrs, ext.lens, locks, lazy=True, add_sep=True, sep=rnd.sep)
        out.keep.append(ext)
        rec.after = snapshot(m, full)
        rec.loaded_after = [int(x) for x in after]
        loaded += rec.loaded_after
        out.rounds.append(rec)
        if scn.pipelined:                                # the round before: its second phase ran beside all of the above
            if r > 0:
                m.emit_select(1)
                out.rounds[r - 1].streams = _fetch(m, len(scn.rounds[r - 1].contigs))
                m.emit_select(0)
        else:
            m.emit_batch_end()
            rec.streams = _fetch(m, n)
    if scn.pipelined:
        m.emit_batch_end()
        out.rounds[-1].streams = _fetch(m, len(scn.rounds[-1].contigs))
    # a further round, matched against what the rounds left behind
    offs = np.zeros(len(scn.probe) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([c.size for c in scn.probe])
    q = backend.tensor(np.concatenate(scn.probe))
    out.keep.append(q)
    backend.sync()
    m.match_batch_dev(q.data_ptr(), offs, MIN_LEN, None)
    counts = m.batch_counts()
    out.probe_rows = [np.asarray(m.batch_matches(i, counts[i])) for i in range(len(scn.probe))]
    out.probe_fp = tuple(int(x) for x in m.batch_fingerprint())
    return out


def check(scn, A, B):
    """the contract, for every round; -> the branch each round took ("applied" / "not applied")"""
    branches = []
    for r, (rnd, a, b) in enumerate(zip(scn.rounds, A.rounds, B.rounds)):
        what = "%s round %d" % (scn.name, r)
        expected = rnd.expected(a.decision, a.un)
        if scn.want[r] is not None:
            assert expected == scn.want[r], "%s: the scenario is built for %r, pass 1 makes it %r (unmatched %r)" % (what, scn.want[r], expected, a.un)
            assert b.applied == expected, "%s: applied is %r, the prediction's outcome is %r" % (what, b.applied, expected)
        assert_state_equal(b.before, a.before, what + ", before the finalize (both paths)")
        if b.applied:
            assert_state_equal(b.after_call, a.after, what + ", applied: the state after the call against the plain finalize's")
            assert b.loaded_after == a.loaded_after, what
        else:
            assert_state_equal(b.after_call, b.before, what + ", not applied: the state after the call against the state before it")
            assert_state_equal(b.after, a.after, what + ", not applied: after the ordinary finalize")
            assert b.loaded_after == a.loaded_after, what
        assert b.un == a.un, what
        for k, ((ua, sa), (ub, sb)) in enumerate(zip(a.streams, b.streams)):
            assert ua == ub, (what, k)
            for name in sa:
                assert bytes(sa[name]) == bytes(sb[name]), "%s: contig %d, stream %s differs" % (what, k, name)
        if b.exchange is not None:
            assert b.exchange.phases == [0, 1], "%s: the exchange was called in phases %r" % (what, b.exchange.phases)
            d = np.nonzero(b.exchange.ref_at_phase0 != b.before["ref"])[0]
            assert d.size == 0, "%s: %d reference bytes had changed when the exchange was asked to reduce the word" % (what, d.size)
        branches.append("applied" if b.applied else "not applied")
    assert B.probe_fp == A.probe_fp, scn.name
    for x, y in zip(A.probe_rows, B.probe_rows):
        assert np.array_equal(x, y), scn.name
    assert A.probe_fp[1] > 0, "%s: the further round found nothing" % scn.name
    return branches


def close(*paths):
    for p in paths:
        p.m.close()


# ------------------------------------------------------------------------------------------- contigs and their kinds
def mutate(c, k, rng):
    """c with k substitutions"""
    c = c.copy()
    at = rng.choice(c.size, size=k, replace=False)
    c[at] = synth.ACGT[(np.searchsorted(synth.ACGT, c[at]) + rng.integers(1, 4, k)) & 3]
    return c


def reference(seed, n=300_000):
    return synth.genome(synth.base_codes(n, seed), 0, 0.0)


def novel(ref, at, n, frac, rng):
    """ref[at:at+n] with a stretch of n*frac random bases in its middle: unmatchedChars comes out near n*frac.
    frac 1/20: proper for the extension (x128) but not for the reverse complement's (x8) and never dissimilar (x8);
    frac 2/5: proper for both, and dissimilar wherever the early-out is not kept away"""
    c = ref[at:at + n].copy()
    k = int(n * frac)
    lo = (n - k) // 2
    c[lo:lo + k] = synth.ACGT[rng.integers(0, 4, k)]
    return c


PLAIN, RC = 1 / 20, 2 / 5


@functools.lru_cache(maxsize=None)
def scenarios():
    """every scenario of the contract, by name (deterministic: fixed seeds, nothing read from anywhere)"""
    S = {}

    def add(s):
        assert s.name not in S
        S[s.name] = s

    ref = reference(101)
    rng = np.random.default_rng(2024)
    six = [novel(ref, 20_000 + 30_000 * i, n, PLAIN, rng) for i, n in enumerate((8_000, 20_001, 4_097, 12_345, 2_000, 16_384))]

    # a. every contig extends, predicted so
    def facts_a(A, scn):
        assert all(0 < u < ln // 8 and u * 128 > ln for u, ln in zip(A.rounds[0].un, scn.rounds[0].lens)), A.rounds[0].un
    add(Scenario("a_all_extend", ref, [Round(six, [1] * 6)], [True], facts=facts_a))

    # b. nothing extends: ext_len all 0, the lazy separators are still loaded
    near = [mutate(ref[40_000 * i + 500: 40_000 * i + 500 + n], 2, rng) for i, n in enumerate((9_000, 15_000, 3_001, 7_777, 2_048, 11_111))]

    def facts_b(A, scn):
        assert all(u * 128 <= ln for u, ln in zip(A.rounds[0].un, scn.rounds[0].lens)), A.rounds[0].un
        assert A.rounds[0].after["loaded_ref_length"] == A.rounds[0].before["loaded_ref_length"] + 6       # six separators
    add(Scenario("b_none_extends", ref, [Round(near, [0] * 6)], [True], facts=facts_b))

    # c. one contig mispredicted
    for i in (0, 3, 5):
        pred = [1] * 6
        pred[i] = 0
        add(Scenario("c_mispredicted_%d" % i, ref, [Round(six, pred)], [False], facts=facts_a))

    # d. more contigs than the check has threads
    many = [novel(ref, 997 * i, 2_000 - (i % 7), PLAIN, rng) for i in range(300)]

    def facts_d(A, scn):
        assert len(A.rounds[0].un) == 300
        assert all(0 < u and u * 8 <= ln < u * 128 for u, ln in zip(A.rounds[0].un, scn.rounds[0].lens)), A.rounds[0].un
    add(Scenario("d_300_contigs", ref, [Round(many, [1] * 300)], [True], facts=facts_d))
    for i in (255, 256, 299):
        pred = [1] * 300
        pred[i] = 0
        add(Scenario("d_300_contigs_mispredicted_%d" % i, ref, [Round(many, pred)], [False], facts=facts_d))

    # e. the threshold: f = len // un is the largest factor that says no
    T = 1
    thr = [near[0], novel(ref, 150_000, 10_000, PLAIN, rng), novel(ref, 200_000, 6_000, RC, rng)]
    for step, right in ((0, True), (0, False), (1, True), (1, False)):
        def derive(un, lens, step=step, right=right):
            f = lens[T] // un[T] + step
            pe = [int(u * f > ln) for u, ln in zip(un, lens)]
            prc = [int(u * 8 > ln) for u, ln in zip(un, lens)]
            if not right:
                pe[T] ^= 1
            return Decision(pe, prc, f, 8)

        def facts_e(A, scn, step=step, right=right):
            u, ln, dec = A.rounds[0].un[T], scn.rounds[0].lens[T], A.rounds[0].decision
            f = ln // u
            assert 0 < u < ln and u * f <= ln < u * (f + 1) and f > 1 and dec.factor == f + step
            assert dec.pred_ext[T] == (step if right else 1 - step)
            assert dec.pred_ext[0] == 0 and dec.pred_ext[2] == 1 and dec.pred_rc == [0, 0, 1]
        add(Scenario("e_threshold_f%s_%s" % ("+1" if step else "", "right" if right else "wrong"), ref,
                     [Round(thr, [0] * 3, derive=derive)], [right], facts=facts_e))
    # ... and equality: a contig the reference knows nothing of, un == len, under a factor of 1. The separator byte is 1 here:
    # a lazy separator of 0 written over the buffer's untouched zeros would not show.
    alien = [synth.ACGT[np.random.default_rng(77).integers(0, 4, 5_000)], near[1]]

    def facts_eq(A, scn):
        assert A.rounds[0].un[0] == scn.rounds[0].lens[0] and A.rounds[0].un[1] < scn.rounds[0].lens[1]
    add(Scenario("e_equality_factor_1", ref, [Round(alien, [0, 0], [0, 0], factor=1, rc_factor=1, sep=1)], [True], facts=facts_eq))
    add(Scenario("e_equality_rc_factor_1", ref, [Round(alien, [1, 0], [0, 0], factor=128, rc_factor=1)], [True], facts=facts_eq))

    # f. reverse-complement extensions
    tri = [six[0], novel(ref, 100_000, 9_000, RC, rng), six[2]]

    def facts_f(A, scn):
        u, ln = A.rounds[0].un[1], scn.rounds[0].lens[1]
        assert u != SKIPPED and u * 8 > ln
        assert all(u * 8 <= ln < u * 128 for u, ln in ((A.rounds[0].un[k], scn.rounds[0].lens[k]) for k in (0, 2)))
    add(Scenario("f_rc_predicted", ref, [Round(tri, [1, 1, 1], [0, 1, 0])], [True], facts=facts_f))
    add(Scenario("f_rc_not_predicted", ref, [Round(tri, [1, 1, 1], [0, 0, 0])], [False], facts=facts_f))
    mixed = [novel(ref, 10_000, 7_000, RC, rng), six[1], near[2], novel(ref, 250_000, 3_333, RC, rng), near[3], six[4]]

    def facts_mixed(A, scn):
        un, lens = A.rounds[0].un, scn.rounds[0].lens
        assert [int(u * 128 > ln) for u, ln in zip(un, lens)] == [1, 1, 0, 1, 0, 1] and [int(u * 8 > ln) for u, ln in zip(un, lens)] == [1, 0, 0, 1, 0, 0]
    add(Scenario("f_mixed", ref, [Round(mixed, [1, 1, 0, 1, 0, 1], [1, 0, 0, 1, 0, 0])], [True], facts=facts_mixed))

    # g. a contig given up as dissimilar: its unmatchedChars is 2^64 - 1, and its products wrap to values that CONFIRM this prediction
    gave_up = six[:3] + [novel(ref, 120_000, 9_000, RC, rng)] + six[4:]

    def facts_g(A, scn):
        assert A.rounds[0].un[3] == SKIPPED and all(u != SKIPPED for k, u in enumerate(A.rounds[0].un) if k != 3)
        ln = scn.rounds[0].lens[3]
        assert (SKIPPED * 128) % 2 ** 64 > ln and (SKIPPED * 8) % 2 ** 64 > ln
    add(Scenario("g_given_up", ref, [Round(gave_up, [1] * 6, [0, 0, 0, 1, 0, 0], processed=[0] * 6)], [False], facts=facts_g))

    # h. a veto, with and without the callbacks; i. the reduced word
    add(Scenario("h_veto", ref, [Round(six, [1] * 6, veto=True)], [False], facts=facts_a))
    add(Scenario("h_veto_with_callbacks", ref, [Round(six, [1] * 6, veto=True, exchange="keep")], [False], facts=facts_a))
    add(Scenario("i_another_replica_said_no", ref, [Round(six, [1] * 6, exchange="zero")], [False], facts=facts_a))
    add(Scenario("i_word_left_alone", ref, [Round(six, [1] * 6, exchange="keep")], [True], facts=facts_a))

    # j. two emissions in flight: applied, not applied, applied
    rounds = []
    for r in range(3):
        cs = [novel(ref, 15_000 + 60_000 * k + 9_000 * r, 7_000 + 501 * k, PLAIN, rng) for k in range(4)]
        pred = [1, 1, 0, 1] if r == 1 else [1] * 4
        rounds.append(Round(cs, pred))

    def facts_j(A, scn):
        for r in range(3):
            assert all(u * 8 <= ln < u * 128 for u, ln in zip(A.rounds[r].un, scn.rounds[r].lens))
    add(Scenario("j_two_in_flight", ref, rounds, [True, False, True], pipelined=True, facts=facts_j))

    # k. the round's loads cross the end of the circular buffer / stop exactly at it (every target's lock is held)
    small = reference(202, 200_000)
    # (taken from the reference's far half: the lock window of a round that wraps covers the buffer's beginning, where nothing is matched)
    five = [novel(small, 100_000 + 18_000 * i, 6_000, PLAIN, rng) for i in range(5)]
    total = sum(c.size + 1 for c in five)

    def facts_cross(A, scn):
        a, b = A.rounds[0].before, A.rounds[0].after
        assert b["loaded_ref_length"] - a["loaded_ref_length"] == total and b["loading_position"] < a["loading_position"]
        assert a["loading_position"] + total > len(a["ref"]) and b["dropped_bytes"] in (None, 0)
        assert a["next_lock"] < a["loading_position"] and all(u * 8 <= ln < u * 128 for u, ln in zip(A.rounds[0].un, scn.rounds[0].lens))
    add(Scenario("k_wrap_crosses_the_end", small, [Round(five, [1] * 5)], [None], max_ref=lambda pos0: pos0 + 15_000, sw_factor=4, facts=facts_cross))

    def facts_exact(A, scn):
        a, b = A.rounds[0].before, A.rounds[0].after
        assert b["loaded_ref_length"] - a["loaded_ref_length"] == total and a["loading_position"] + total == len(a["ref"])
        assert b["dropped_bytes"] in (None, 0)
        assert a["next_lock"] < a["loading_position"] and all(u * 8 <= ln < u * 128 for u, ln in zip(A.rounds[0].un, scn.rounds[0].lens))
    add(Scenario("k_wrap_stops_at_the_end", small, [Round(five, [1] * 5)], [None], max_ref=lambda pos0: pos0 + total, sw_factor=4, facts=facts_exact))
    return S
