"""The hashed k-mer length K on the device. init_params derives K from the matching length L (12, 16, 20, 24, 28, 32, 36, 40, 44 or
56: every K the reference instantiates its hash for), and K is no passive parameter there: it is the trip count of the insertion's
and the lookups' hash loops, the size of a lookup window's loads, the choice between k_resolve_blocks4 (K <= K_MAX4 = 40) and
k_resolve_blocks, what a speculative block must have warmed up over, and what "too short to hold a K-mer" means in every kernel
that computes n - K + 1. One L per K (tests/_kmer.py), min_len = L throughout, everything bit-exact against the oracle, which
tests/test_oracle_vs_ref.py pins on the reference at the same ten L.

Which resolve kernel ran is not something batch_stats() or emit_stats() tell, so it is not asserted: by batch_layout's condition
the default run and SWSEM_CHAINS=1 are different kernels at L <= 62 and the same one above.

Every case asserts that the oracle alone finds at least 50 rows, one of them of length exactly L (_kmer.assert_covered).

Replay counters seen on an MI355X over test_stitch_and_replay (SWSEM_RB=1; an observation, only > 0 is asserted):
(replayed_blocks / replays_precomputed / candidates_refused, summed over the three queries of collection(L))
  L=16  K=12: SWSEM_OVERLAP=0 261 / 0 / 0, SWSEM_OVERLAP=64  62 / 10 / 0
  L=56  K=40: SWSEM_OVERLAP=0 206 / 0 / 0, SWSEM_OVERLAP=64  84 / 17 / 0
  L=64  K=44: SWSEM_OVERLAP=0 198 / 0 / 0, SWSEM_OVERLAP=64  95 / 18 / 0
  L=120 K=56: SWSEM_OVERLAP=0 174 / 0 / 0, SWSEM_OVERLAP=64 122 /  6 / 0

A skip margin above L (-k 16 -m 2: margin 24) is what this file found the ORACLE wrong about, not the device: a hit inside a match
whose left end was cut behind the hit's position has a negative lastDelta, which the reference's strcmplcp passes
(tests/test_oracle_vs_ref.py::test_a_skip_margin_above_the_matching_length pins the mended restatement on the reference);
test_a_skip_margin_above_the_matching_length here runs the device over the same drives."""
import functools

import numpy as np
import pytest

import _driver
import _kmer
import _orc

pytestmark = pytest.mark.gpu
NO_LOCK = _orc.NO_LOCK
LS, K_OF_L = _kmer.LS, _kmer.K_OF_L
LIM = 4_000_000


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    return b


def pair(binding, max_len, **kw):
    h, o = binding.SlidingWindowSparseEMMatcher(max_len, **kw), _orc.OracleMatcher(max_len, **kw)
    assert h.K() == o.K() == K_OF_L[kw["L"]] and h.hash_size() == o.hash_size()
    return h, o


def assert_same_state(h, o):
    assert h.loading_position() == o.loading_position()
    assert h.ref_length() == o.ref_length()
    assert h.loaded_ref_length() == o.loaded_ref_length()
    n = o.ref_length()
    assert np.array_equal(h.ref(n)[1:], o.ref(n)[1:])
    a, b = h.ht(), o.ht()
    assert np.array_equal(a, b), "HT image differs at %d buckets" % int((a != b).sum())


def collection(L):
    """three genomes 2 % from each other and one 10 % from them, 90 000 bases"""
    return _kmer.related(3, 90_000, 100 + L)


@functools.lru_cache(maxsize=None)
def expected_rows(L, k1=16):
    """the oracle's rows for every genome of collection(L) after the first, each loaded after it was matched (computed once)"""
    gs = collection(L)
    o = _orc.OracleMatcher(LIM, L=L, k1=k1)
    o.load_ref(gs[0], load_rc=True)
    rows = []
    for g in gs[1:]:
        rows.append(o.match(g, L))
        o.load_ref(g)
    end = o.loading_position()
    o.close()
    _kmer.assert_covered(rows, L, "collection k1=%d" % k1)
    return rows, end


# ---- rows, table image, loader state
ROW_CASES = [(L, 16) for L in LS] + [(16, 8), (56, 8), (20, 7), (120, 9)]       # k1 = 8 at K = 12 and 40, an odd one at K = 16 and 56


@pytest.mark.parametrize("L,k1", ROW_CASES)
def test_rows_table_and_loader_state(binding, L, k1):
    gs = collection(L)
    h, o = pair(binding, LIM, L=L, k1=k1)
    for m in (h, o):
        m.load_ref(gs[0], load_rc=True)
    assert_same_state(h, o)                                            # (the insertion alone, before any lookup)
    rows = []
    for i, g in enumerate(gs[1:]):
        a, b = h.match(g, L), o.match(g, L)
        assert np.array_equal(a, b), (L, k1, i)
        rows.append(b)
        for m in (h, o):
            m.load_ref(g)
    assert_same_state(h, o)
    _kmer.assert_covered(rows, L, "collection k1=%d" % k1)
    h.close(); o.close()


# ---- both block kernels and the sequential replay
@pytest.mark.parametrize("env", [{}, {"SWSEM_CHAINS": "1"}, {"SWSEM_RESOLVE": "seq"}], ids=["default", "chains1", "seq"])
@pytest.mark.parametrize("L", [16, 28, 56, 64, 120])
def test_block_kernels_and_the_sequential_replay(binding, monkeypatch, L, env):
    """K = 12, 24, 40 (the largest the four-chain kernel's 16-dword window holds), 44 and 56 (one chain per wave by K > K_MAX4)"""
    for k in ("SWSEM_CHAINS", "SWSEM_RESOLVE", "SWSEM_RB", "SWSEM_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    gs = collection(L)
    rows, end = expected_rows(L)
    h = binding.SlidingWindowSparseEMMatcher(LIM, L=L)
    h.load_ref(gs[0], load_rc=True)
    for i, (g, exp) in enumerate(zip(gs[1:], rows)):
        assert np.array_equal(h.match(g, L), exp), (L, env, i)
        h.load_ref(g)
    assert h.loading_position() == end
    h.close()


# ---- edges
def batch_against_oracle(h, o, contigs, L, lead=0):
    """the contigs back to back in one device buffer, `lead` bytes into it, through match_batch_dev; -> the oracle's rows"""
    import torch
    offs = np.zeros(len(contigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([c.size for c in contigs])
    buf = torch.from_numpy(np.concatenate([np.zeros(lead, dtype=np.uint8)] + list(contigs))).to("cuda:0")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    h.match_batch_dev(buf.data_ptr() + lead, offs, L, None)
    counts = h.batch_counts()
    exp = [o.match(c, L) for c in contigs]
    for i, e in enumerate(exp):
        assert counts[i] == len(e), (L, lead, i, contigs[i].size)
        assert np.array_equal(h.batch_matches(i, counts[i]), e), (L, lead, i)
    return exp


@pytest.mark.parametrize("L", LS)
def test_edges(binding, L):
    """in one batch beside a long contig: contigs of K - 1, K, K + 1, L - 1, L and L + 1 bases (the first holds no K-mer, the next four
    none long enough), the planted copies of L - 1 / L / L + 1 bases; the long contig shares a run of one letter longer than K + 64,
    a run of N and a lower-case stretch with the reference; then queries that start 1, 2, 3 and 5 bytes into their buffer (the
    misalignment `sh` of the window loads)"""
    K = K_OF_L[L]
    g0, g1 = _kmer.hard_pair(L, K, 200 + L)
    pref, pq = _kmer.planted(L)
    h, o = pair(binding, LIM, L=L)
    for m in (h, o):
        m.load_ref(g0, load_rc=True)
        m.load_ref(pref, load_rc=False)
    assert_same_state(h, o)
    shorts = _kmer.short_contigs(g0, L, K)
    exp = batch_against_oracle(h, o, [g1] + shorts + [pq], L)
    _kmer.assert_covered(exp, L, "edges")
    assert all(len(e) == 0 for e, c in zip(exp[1:-1], shorts) if c.size < L)
    assert sum(len(e) for e in exp[1:-1]) > 0                           # (the pieces of L and L + 1 bases that hold a sampled K-mer)
    planted_lens = exp[-1][:, 1]
    assert (planted_lens == L).any() and not (planted_lens == L - 1).any()
    run = exp[0][(exp[0][:, 2] < 5_000 + K + 64 + 37) & (exp[0][:, 2] + exp[0][:, 1] > 5_000)]
    assert len(run) > 0                                                 # the run of one letter was matched
    for lead in (1, 2, 3, 5):
        batch_against_oracle(h, o, [g1[lead:lead + 10_001], g1[40_000:40_000 + K + lead]], L, lead)
    h.close(); o.close()


def test_proteins_profile(binding):
    """the reference's proteins profile: k = 16 (K = 12), sequences over the 20-letter amino-acid alphabet, no reverse complements"""
    L = 16
    gs = _kmer.proteins(4, 80_000, 77)
    h, o = pair(binding, LIM, L=L)
    for m in (h, o):
        m.load_ref(gs[0], load_rc=False)
    rows = []
    for i, g in enumerate(gs[1:]):
        a, b = h.match(g, L), o.match(g, L)
        assert np.array_equal(a, b), i
        rows.append(b)
        for m in (h, o):
            m.load_ref(g, load_rc=False)
    assert_same_state(h, o)
    _kmer.assert_covered(rows, L, "proteins")
    h.close(); o.close()


# ---- a skip margin above the matching length
@pytest.mark.parametrize("env", [{}, {"SWSEM_RESOLVE": "seq"}], ids=["default", "seq"])
@pytest.mark.parametrize("L,margin,mode", [(16, 24, 2), (20, 24, 2), (16, 20, 1), (16, 40, 2), (32, 48, 1)])
def test_a_skip_margin_above_the_matching_length(binding, monkeypatch, L, margin, mode, env):
    """matches shorter than the margin send the scan on by one position, back inside a match cut at its left end: hits with a
    negative lastDelta (SlidingWindowSparseEMMatcher.cpp:264-270). Rows, streams and table through the sequential drive."""
    for k in ("SWSEM_CHAINS", "SWSEM_RESOLVE", "SWSEM_RB", "SWSEM_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    files = emit_files(L)[:5]
    lim, _ = _driver.ref_length_limit(len(files), 70_000)
    h = binding.SlidingWindowSparseEMMatcher(lim, L=L, skip_margin=margin)
    o = _orc.OracleMatcher(lim, L=L, skip_margin=margin)
    he = VerifiedHipEmitter(binding, h, binding.emit_params(mode))
    oe = _orc.OracleEmitter(o, _orc.emit_params(mode))
    pol = _driver.Policy(mode)
    a = _driver.encode_sequential(h, he, files, pol, min_len=L)
    b = _driver.encode_sequential(o, oe, files, pol, min_len=L)
    for i, (x, y) in enumerate(zip(a["matches"], b["matches"])):
        assert np.array_equal(x, y), (L, margin, i, len(x), len(y))
    assert a["locks"] == b["locks"] and a["refExtSize"] == b["refExtSize"]
    compare(he.streams(), oe.streams())
    assert_same_state(h, o)
    _kmer.assert_covered(b["matches"], L, "margin")
    h.close(); o.close()


# ---- stitch and replay
TOTALS = {}


@pytest.mark.parametrize("L", [16, 56, 64, 120])
def test_stitch_and_replay(binding, monkeypatch, L):
    """blocks of 1024 positions behind no warm-up at all and behind 64 positions: rejected blocks — replayed ahead of the walk by
    k_stitch_replay or in place — at K = 12, 40, 44 and 56; the rows are the oracle's"""
    monkeypatch.delenv("SWSEM_CHAINS", raising=False)
    monkeypatch.delenv("SWSEM_RESOLVE", raising=False)
    monkeypatch.setenv("SWSEM_RB", "1")
    gs = collection(L)
    rows, end = expected_rows(L)
    total = 0
    for overlap in (0, 64):
        monkeypatch.setenv("SWSEM_OVERLAP", str(overlap))
        h = binding.SlidingWindowSparseEMMatcher(LIM, L=L)
        h.load_ref(gs[0], load_rc=True)
        seen = dict(replayed_blocks=0, replays_precomputed=0, candidates_refused=0)
        for i, (g, exp) in enumerate(zip(gs[1:], rows)):
            assert np.array_equal(h.match(g, L), exp), (L, overlap, i)
            st = h.batch_stats()
            for k in seen:
                seen[k] += int(st[k])
            h.load_ref(g)
        assert h.loading_position() == end
        h.close()
        TOTALS[(L, overlap)] = seen
        print("stitch replay counters L=%d K=%d overlap=%d: %s" % (L, K_OF_L[L], overlap, seen))
        if overlap == 0:
            assert seen["replayed_blocks"] > 0, seen                    # (no warm-up rejects more than half of the blocks)
        total += seen["replayed_blocks"]
    assert total > 0


# ---- a buffer that has wrapped
@pytest.mark.parametrize("sequential", [True, False], ids=["sequential", "window"])
@pytest.mark.parametrize("L", [16, 56, 120])
def test_wrapped_buffer(binding, L, sequential):
    """the schedule of test_wrap_quirk_and_locks (a 100 000-byte buffer, 14 steps, reverse-complement loads, separators, locks
    with the sliding window) at K = 12, 40 and 56"""
    h, o = pair(binding, 100_000, L=L)
    if sequential:
        h.disable_sliding_window(); o.disable_sliding_window()
    rows = []
    for step, (g, rc, sep) in enumerate(_kmer.wrap_steps(L, 400 + L, steps=14)):
        lock = NO_LOCK
        if not sequential:
            lh, lo = h.acquire_lock(), o.acquire_lock()
            assert lh == lo
            lock = lo
        a, b = h.match(g, L, lock), o.match(g, L, lock)
        assert np.array_equal(a, b), (L, step)
        rows.append(b)
        for m in (h, o):
            m.load_ref(g, load_rc=rc, add_sep=True)
            if sep:
                m.load_separator(0)
        if not sequential:
            h.release_lock(lock); o.release_lock(lock)
        assert_same_state(h, o)
    assert o.loaded_ref_length() > 100_000                              # the loaded length passed the limit
    _kmer.assert_covered(rows, L, "wrap")
    h.close(); o.close()


# ---- emission, device verification, decoding
EMIT_LS = [16, 24, 60, 64, 120]                                         # K = 12, 20, 40, 44, 56
K_OF_EMIT = {16: 12, 24: 20, 60: 40, 64: 44, 120: 56}


class VerifiedHipEmitter:
    """_driver emitter over swsem_emit (tests/test_gpu_emit.py's) that has every emission checked by the device decoder"""

    def __init__(self, binding, matcher, params):
        self.b, self.m, self.p = binding, matcher, params
        self.s = {k: b"" for k in binding.STREAM_NAMES}
        self.verified = 0

    def process(self, m, contig, lock, factor, processed, target_idx, loaded):
        un, streams, st = self.m.emit(self.p, 0, lock, factor, processed, target_idx, loaded)
        assert self.m.emit_verify() == (0, -1, 2 ** 64 - 1)
        self.verified += 1
        if un != self.b.SKIPPED:
            for k in self.s:
                self.s[k] += streams[k]
        return un

    def put(self, which, data): self.s[self.b.STREAM_NAMES[which]] += bytes(data)
    def streams(self): return dict(self.s)


def compare(a, b):
    for k in b:
        assert a[k] == b[k], "%s differs (%d vs %d bytes)" % (k, len(a[k]), len(b[k]))


def emit_files(L):
    """five genomes of 70 000 bases 2 % from each other and one 10 % from them, two contigs each"""
    return [[g[:30_000], g[30_000:]] for g in _kmer.related(5, 70_000, 500 + L)]


def emit_pair(binding, L, mode, lim):
    margin = 24 if mode >= 2 else 16
    h = binding.SlidingWindowSparseEMMatcher(lim, L=L, skip_margin=margin)
    o = _orc.OracleMatcher(lim, L=L, skip_margin=margin)
    assert h.K() == o.K() == K_OF_EMIT[L]
    return h, o


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("L", EMIT_LS)
def test_emission_sequential(binding, L, mode):
    files = emit_files(L)[:5]
    lim, _ = _driver.ref_length_limit(len(files), 70_000)
    h, o = emit_pair(binding, L, mode, lim)
    he = VerifiedHipEmitter(binding, h, binding.emit_params(mode))
    oe = _orc.OracleEmitter(o, _orc.emit_params(mode))
    pol = _driver.Policy(mode)
    a = _driver.encode_sequential(h, he, files, pol, min_len=L)
    b = _driver.encode_sequential(o, oe, files, pol, min_len=L)
    assert a["locks"] == b["locks"] and a["refExtSize"] == b["refExtSize"] and a["loaded"] == b["loaded"]
    for x, y in zip(a["matches"], b["matches"]):
        assert np.array_equal(x, y)
    compare(he.streams(), oe.streams())
    assert_same_state(h, o)
    assert he.verified == sum(len(f) for f in files)
    _kmer.assert_covered(b["matches"], L, "sequential emission")
    h.close(); o.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("L", EMIT_LS)
def test_emission_rounds(binding, L, mode):
    files = emit_files(L)
    h, o = emit_pair(binding, L, mode, LIM)
    pol = _driver.Policy(mode)
    made = []

    def make_hip():
        made.append(VerifiedHipEmitter(binding, h, binding.emit_params(mode)))
        return made[-1]
    a = _driver.encode_rounds(h, make_hip, files[0], files[1:], 3, pol, min_len=L)
    b = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o, _orc.emit_params(mode)), files[0], files[1:], 3, pol, min_len=L)
    assert a["locks"] == b["locks"] and a["refExtSize"] == b["refExtSize"] and a["unmatched"] == b["unmatched"]
    for x, y in zip(a["matches"], b["matches"]):
        assert np.array_equal(x, y)
    compare(a["streams"], b["streams"])
    assert_same_state(h, o)
    assert sum(e.verified for e in made) >= len(b["matches"])
    _kmer.assert_covered(b["matches"], L, "emission in rounds")
    h.close(); o.close()


@pytest.mark.parametrize("L", EMIT_LS)
def test_emitted_streams_decode_on_the_device(binding, L):
    """test_gpu_decode.py's pass at other lengths: every emission verified on the device, and the same streams through
    swsem_decode_contigs_dev from buffers of their own — the contig, the byte count and the return value of the oracle's decoder"""
    import torch
    gs = _kmer.related(4, 70_000, 600 + L)[:4]
    p, po = binding.emit_params(1), _orc.emit_params(1)
    h, o = emit_pair(binding, L, 1, LIM)
    for m in (h, o):
        m.load_ref(gs[0], load_rc=True)
    loaded = [h.loaded_ref_length()]
    rows = []
    for t, g in enumerate(gs[1:]):
        for c in (g[:30_000], g[30_000:]):
            m_h, m_o = h.match(c, L), o.match(c, L)
            assert np.array_equal(m_h, m_o)
            rows.append(m_o)
            un, streams, _ = h.emit(p, 0, binding.NO_LOCK, 128, t, t, loaded)
            assert h.emit_verify() == (0, -1, 2 ** 64 - 1)
            oe = _orc.OracleEmitter(o, po)
            assert oe.process(m_o, c, NO_LOCK, 128, t, t, loaded) == un
            compare(streams, oe.streams())
            bufs = [torch.from_numpy(np.frombuffer(streams[k], dtype=np.uint8).copy()).to("cuda:0") if len(streams[k]) else
                    torch.empty(1, dtype=torch.uint8, device="cuda:0") for k in binding.STREAM_NAMES]
            dest = torch.zeros(c.size + 16, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            job = ([(b.data_ptr(), len(streams[k])) for b, k in zip(bufs, binding.STREAM_NAMES)], binding.NO_LOCK, dest.data_ptr(), c.size)
            dl, un2 = h.decode_contigs_dev(p, [job])
            back, un3 = _orc.decode_contig(h.ref(h.max_ref_length()), po, streams, NO_LOCK, c.size + 16)
            assert int(dl[0]) == c.size and np.array_equal(dest.cpu().numpy()[:c.size], c) and np.array_equal(back, c)
            assert int(un2[0]) == un3 == (un & 0xFFFFFFFF)
            for m in (h, o):
                m.load_ref(c)
                m.load_separator(0)
            loaded.append(h.loaded_ref_length())
    assert_same_state(h, o)
    _kmer.assert_covered(rows, L, "decode")
    h.close(); o.close()


@pytest.mark.parametrize("L", [16, 64])
def test_round_runner(binding, L):
    """mbgc_amd.rounds.RoundRunner with run_round(..., min_len=L) against the reference loop of tests/_driver.py on the oracle"""
    import torch
    from mbgc_amd.rounds import RoundRunner
    gs = _kmer.related(9, 70_000, 700 + L)[:9]
    h, o = emit_pair(binding, L, 1, LIM)
    R = 3
    b = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o), [gs[0]], [[g] for g in gs[1:]], R, min_len=L)
    _kmer.assert_covered(b["matches"], L, "round runner")
    h.set_sliding_window_size(16)
    h.load_ref(gs[0], load_rc=True)
    runner = RoundRunner(h, 0, 1, None, "cuda:0", lazy=True, emit_params=binding.emit_params(1))
    runner.start()
    for r0 in range(1, len(gs), R):
        chunk = gs[r0:r0 + R]
        buf = torch.from_numpy(np.concatenate(chunk)).to("cuda:0")
        offs = np.zeros(len(chunk) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([c.size for c in chunk])
        torch.cuda.synchronize()
        runner.run_round(buf, offs, min_len=L)
    runner.flush()
    for k in b["streams"]:
        assert bytes(runner.streams[k]) == b["streams"][k], k
    assert bytes(runner.locks_stream) == b["locks"] and bytes(runner.ref_ext_sizes) == b["refExtSize"]
    assert_same_state(h, o)
    h.close(); o.close()
