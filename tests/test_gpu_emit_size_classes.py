"""The emission's second phase (k_emit_sizes, k_emit_write, k_emit_copy_long) picks device code by a size alone at six places:
<4> or <1> by the batch's chunks, a plain run's thread loop / wave copy / listed copy / wave copy again when the list is full, the
left and the right extension by one thread or by the wave. The corpus of tests/_emitsizes.py sits on every one of these edges
(tests/test_emit_size_classes_cpu.py shows that on the oracle); here every contig of it is emitted `alone` (thin: <4>), in a
`crowd` of 600 fillers and `beside_big` (not thin: <1>), and its six streams, unmatchedChars and four counters are held to the
oracle byte for byte — and to each other across the three settings, which holds <4> and <1> to each other directly.

Which path ran is not observed on the device: it follows from the restated rules the CPU test pins to the sources.

Shown by experiment (one device run each, kernels broken by hand in a scratch copy, every break leaving bytes unwritten only):
  the wave copy without its byte tail    45 of the 50 cases fail, first test_batch_equals_the_oracle[alone_plain-*]; all but alone_lanes
                                         (its runs are inline or listed, none is the wave's)
  k_emit_copy_long without the last piece 45 fail, first [alone_plain-*] and every batch with a run of LONG_COPY_MIN bytes: all but alone_wide
  a full list discards the run           test_emission_after_an_emission_that_filled_the_list alone fails (overflow / run_3761, all its bytes)
  k_emit_write<1> one lane on            the 15 cases that are not thin fail (crowd, beside_big, locks, 40-bit, overflow), every `alone` case passes
What a missed write leaves in the arena is what an earlier emission put there: it can be the right byte when the same batch was
emitted before with the same literals at the same place. Every batch's first emission lands on other bytes.

Not covered here: runs or extension stretches beyond 2^32 bytes (litLeft <= UINT32_MAX in right_task_wide), and the emission's
first phase (k_emit_p1_*, k_emit_meta_*), which tests/test_gpu_pairing_chain.py owns.

Wall times on one MI355X, observed, not asserted: the module's 50 cases 9.0 s. Of that the overflow case 4.8 s (6.0 s inside a
run of the whole suite) — 4.3 s its first
emission (145 MB of query; nearly all of it the oracle's match call on each of the 4 300 runs, which the second emission, 0.1 s,
does not repeat; the 4 320 results come down as one packed arena, emit_result only slices it), beside_big 0.4 s with its own
handle's set-up, the locks' case 0.4 s, every other case at most 0.15 s."""
import time

import numpy as np
import pytest

import _emitsizes as E
import _orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0
    return b


class Rig:
    """one device handle and the oracle on the same reference; what the device gave for a (batch, parameters), kept once"""

    def __init__(self, binding, ref, max_ref_len, sliding_window=None):
        self.b = binding
        self.h = binding.SlidingWindowSparseEMMatcher(max_ref_len)
        if sliding_window is not None:
            self.h.set_sliding_window_size(sliding_window)
        self.h.load_ref(ref, load_rc=False)
        self.ref = E.Referee(ref, max_ref_len, sliding_window)
        self.seen = {}

    def close(self):
        self.h.close()

    def emit(self, batch, key, locks=None):
        """upload, match_batch_dev, emit_batch; every contig's result against the oracle's. -> {name: (unmatched, streams, counters)}"""
        import torch
        contigs, names = batch["contigs"], batch["names"]
        n = len(contigs)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([c.size for c in contigs])
        buf = torch.from_numpy(np.concatenate(contigs)).to("cuda:0")
        torch.cuda.synchronize()
        h = self.h
        h.match_batch_dev(buf.data_ptr(), offs, E.MIN_LEN, locks)
        counts = h.batch_counts()
        loaded = [h.loading_position()]
        assert loaded == self.ref.loaded
        p = E.params_of(self.b.emit_params, key)
        if locks is None:
            h.emit_batch(p, loaded=loaded, n=n)
        else:
            assert h.emit_batch(p, locks=locks, factors=[128] * n, processed=[0] * n, target_idx=[0] * n, loaded=loaded) == n
        out = {}
        for i, (name, c) in enumerate(zip(names, contigs)):
            lock = None if locks is None else int(locks[i])
            rows = self.ref.rows(name, c, lock)
            assert counts[i] == len(rows), (batch["name"], name)
            if len(rows):
                assert np.array_equal(h.batch_matches(i, counts[i]), rows), (batch["name"], name)
            want = self.ref.emit(name, c, key, lock)
            un, streams, st = h.emit_result(i)
            where = "%s / %s %r" % (batch["name"], name, key)
            assert un == want["unmatched"], where
            for s in _orc.STREAM_NAMES:
                assert len(streams[s]) == len(want["streams"][s]), "%s: %s is %d bytes, the oracle's %d" % (where, s, len(streams[s]), len(want["streams"][s]))
                if streams[s] != want["streams"][s]:
                    a, b = np.frombuffer(streams[s], dtype=np.uint8), np.frombuffer(want["streams"][s], dtype=np.uint8)
                    first = int(np.nonzero(a != b)[0][0])
                    raise AssertionError("%s: %s differs from the oracle's at byte %d of %d (%d bytes differ)" % (where, s, first, a.size, int((a != b).sum())))
            counters = {k: int(getattr(st, k)) for k in E.COUNTERS}
            assert counters == {k: want["counters"][k] for k in E.COUNTERS}, where
            out[name] = (un, streams, counters)
        del buf
        return out

    def emit_once(self, batch, key):
        k = (batch["name"], key)
        if k not in self.seen:
            hard = E.hard_contigs()
            self.seen[k] = {n: v for n, v in self.emit(batch, key).items() if n in hard}
        return self.seen[k]


@pytest.fixture(scope="module")
def rig(binding):
    r = Rig(binding, E.reference(), 4_000_000)
    yield r
    r.close()


@pytest.fixture(scope="module")
def big_rig(binding):
    r = Rig(binding, E.big_reference(), 16_000_000)
    yield r
    r.close()


BATCHES = {b["name"]: b for b in E.batches()}
SMALL = [n for n, b in BATCHES.items() if b["ref"] == "small"]
KEYS = [E.params_key(*p) for p in E.PARAMS]
BIG_KEYS = [E.params_key(1, 1, 1), E.params_key(1, 1, 0)]             # (the one batch that needs a reference of its own: extensions on, and off)


def ids(keys):
    return ["m%d-lazy%d-ext%d" % (k[0], dict(k[1])["lazyDecompressionSupport"], dict(k[1])["enableExtensionsWithMismatches"]) for k in keys]


@pytest.mark.parametrize("key", KEYS, ids=ids(KEYS))
@pytest.mark.parametrize("name", SMALL)
def test_batch_equals_the_oracle(rig, name, key):
    """`alone` (thin: k_emit_sizes<4> / k_emit_write<4>) and `crowd` (not thin: <1>)"""
    b = BATCHES[name]
    assert b["expected_thin"] == (b["kind"] == "alone")
    got = rig.emit_once(b, key)
    assert set(got) == {n for n in b["names"] if n in E.hard_contigs()}


@pytest.mark.parametrize("key", BIG_KEYS, ids=ids(BIG_KEYS))
def test_beside_big_equals_the_oracle(big_rig, key):
    """<1>, the hard contigs' blocks at chunk indices beyond EMIT_THIN_MAX"""
    b = BATCHES["beside_big"]
    assert not b["expected_thin"] and E.chunks_of(b["contigs"][0].size) > E.EMIT_THIN_MAX
    big_rig.emit_once(b, key)


@pytest.mark.parametrize("key", KEYS, ids=ids(KEYS))
def test_streams_do_not_depend_on_the_batch_mates(rig, big_rig, key):
    """a contig's result from `alone`, from the `crowd` and from `beside_big` (its rows are the same against the large reference:
    the CPU test) — the device's own outputs against each other"""
    crowd = rig.emit_once(BATCHES["crowd"], key)
    beside = big_rig.emit_once(BATCHES["beside_big"], key) if key in BIG_KEYS else None
    hard = set(E.hard_contigs())
    done = set()
    for name in SMALL:
        if BATCHES[name]["kind"] != "alone":
            continue
        for n, got in rig.emit_once(BATCHES[name], key).items():
            assert got == crowd[n], "%s: alone (<4>) and in the crowd (<1>) differ" % n
            if beside is not None:
                assert got == beside[n], "%s: alone (<4>) and beside the big contig (<1>) differ" % n
            done.add(n)
    assert done == hard == set(crowd)


def test_40bit_offsets_and_plain_lengths_in_the_crowd(rig):
    """enable40bitReference = 1 (a fifth offset byte per match) with frugal64bitLenEncoding flipped (4-byte lengths): the other
    four streams' placement beside the same literal runs"""
    key = E.params_key(1, 1, 1, enable40bitReference=1, frugal64bitLenEncoding=0)
    got = rig.emit(BATCHES["crowd"], key)
    assert any(len(v[1]["mapOff5th"]) for v in got.values())


def test_crowd_with_per_contig_locks(binding):
    """every contig under a matching lock of its own, as the rounds acquire them"""
    r = Rig(binding, E.reference(), 8_000_000, sliding_window=16)
    try:
        b = BATCHES["crowd"]
        locks = [r.h.acquire_lock() for _ in b["contigs"]]
        assert locks == [r.ref.o.acquire_lock() for _ in b["contigs"]]
        assert all(x != _orc.NO_LOCK for x in locks)
        r.emit(b, E.params_key(1, 1, 1), locks)
    finally:
        r.close()


def test_emission_after_an_emission_that_filled_the_list(rig):
    """more runs of at least LONG_COPY_MIN bytes than the list has entries: the runs that find it full are copied by their own
    waves — which ones is the atomic counter's choice, so every one of the 4 320 results is compared, not a sample. Twice in a
    row on one handle, then a crowd and an `alone` batch: the list and its count start empty every time."""
    key = E.params_key(1, 1, 1)
    b = E.overflow_batch()
    assert not b["expected_thin"] and sum(c.size >= E.LONG_COPY_MIN for c in b["contigs"]) > E.LONG_COPY_CAP + 100
    times = []
    for what, batch in (("overflow", b), ("overflow again", b), ("crowd", BATCHES["crowd"]), ("alone_plain", BATCHES["alone_plain"]),
                        ("alone_zero", BATCHES["alone_zero"])):
        t = time.time()
        rig.emit(batch, key)
        times.append("%s %.1f s" % (what, time.time() - t))
    print("emission after emission: " + ", ".join(times))
