"""The source-region lookups of the pairing chain's lazy rule (getMatchLoadedPos and the upper_bound in refExtLoadedPosArr,
MBGC_Encoder.cpp:137-141,254-256) are made for every STITCHED row beside pass 1 (k_emit_regions_raw) and carried to the kept
rows by k_emit_p1_compact, for the first emission of a batch; a later emission of the same batch looks them up behind pass 1
as before (k_emit_meta_regions). What can go wrong is a raw row's value landing on another kept row, a left-extended row
keeping the value of where it used to start, and the two paths disagreeing. Six streams against the oracle, byte for byte."""
import functools

import numpy as np
import pytest

import _driver
import _orc
from mbgc_amd import synth
from test_gpu_emit import compare

pytestmark = pytest.mark.gpu
NO_LOCK = _orc.NO_LOCK
ACGT = synth.ACGT
CH, MSPAN = 256, 4096                                  # mbgc_amd/csrc/swsem_emit.hip: rows per chunk of pass 1, kept rows per span of the pairing chain


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0
    return b


def mutated(rng, x, rate):
    y = x.copy()
    idx = np.nonzero(rng.random(x.size) < rate)[0]
    y[idx] = ACGT[(np.searchsorted(ACGT, y[idx]) + rng.integers(1, 4, idx.size)) & 3]
    return y


def load_pieces(m, pieces, unlisted):
    """pieces loaded one by one, each followed by a separator (lazy decompression); -> refExtLoadedPosArr. The `unlisted` pieces
    are loaded behind the last listed position: a match whose source lies there has no region behind it (UINT64_MAX)."""
    m.disable_sliding_window()
    loaded = []
    for p in pieces:
        m.load_ref(p, load_rc=False, add_sep=True, sep=0)
        m.load_separator(0)
        loaded.append(m.loading_position())
    for p in unlisted:
        m.load_ref(p, load_rc=False, add_sep=True, sep=0)
        m.load_separator(0)
    return loaded


def device_batch(binding, h, contigs, params, loaded, processed=None, target_idx=None):
    import torch
    offs = np.zeros(len(contigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([c.size for c in contigs])
    buf = torch.from_numpy(np.concatenate(contigs)).to("cuda:0")
    torch.cuda.synchronize()
    h.match_batch_dev(buf.data_ptr(), offs, 32, None)
    n = h.emit_batch(params, factors=[128] * len(contigs), processed=processed or [0] * len(contigs),
                     target_idx=target_idx or [0] * len(contigs), loaded=loaded)
    assert n == len(contigs)
    return [h.emit_result(i)[:2] for i in range(n)]


def oracle_batch(o, contigs, params, loaded, processed=None, target_idx=None):
    out = []
    for i, c in enumerate(contigs):
        oe = _orc.OracleEmitter(o, params)
        rows = np.asarray(o.match(c, 32, NO_LOCK)).reshape(-1, 3)
        un = oe.process(rows, c, NO_LOCK, 128, (processed or [0] * len(contigs))[i], (target_idx or [0] * len(contigs))[i], loaded)
        out.append((un, oe.streams(), rows, oe.counters()))
    return out


def hold(binding, got, want):
    for (un, streams), w in zip(got, want):
        if w[0] == _orc.SKIPPED:
            assert un == binding.SKIPPED
            continue
        assert un == w[0]
        compare(streams, w[1])


# ---- 1. several loaded pieces, lazy decompression on and off

@functools.lru_cache(maxsize=None)
def pieces_case():
    rng = np.random.default_rng(4101)
    pieces = [ACGT[rng.integers(0, 4, 40_000)] for _ in range(7)]
    lim = 2_000_000
    o = _orc.OracleMatcher(lim)
    loaded = load_pieces(o, pieces[:6], pieces[6:])
    ref = o.ref(o.loaded_ref_length() + 1)
    seps = [x - 1 for x in loaded]                                   # the separator byte behind every listed piece
    contigs = []
    for k in range(3):
        parts = []
        for s in range(14):
            if s % 3 == 1:                                           # across a separator: one diagonal, two source regions
                at = seps[(s + k) % 6]
                seg = ref[at - 1_400: at + 1_400].copy()
                seg[seg == 0] = ACGT[0]
            else:
                p = (5 * s + k) % 7                                  # every piece, the unlisted last one among them
                a = int(rng.integers(1_000, 36_000))
                seg = pieces[p][a: a + 2_900].copy()
            parts.append(mutated(rng, seg, 0.01))
        contigs.append(np.concatenate(parts))
    res = {}
    for lazy in (1, 0):
        res[lazy] = oracle_batch(o, contigs, _orc.emit_params(1, lazyDecompressionSupport=lazy), loaded)
    o.close()
    return pieces, loaded, contigs, res, lim


@pytest.mark.parametrize("lazy", [1, 0])
def test_several_loaded_pieces_with_lazy_decompression_on_and_off(binding, lazy):
    pieces, loaded, contigs, res, lim = pieces_case()
    assert len(loaded) >= 5 and all(38_000 < c.size < 42_000 for c in contigs)
    for un, streams, rows, _ in res[1]:
        src = rows[:, 0]
        regions = np.searchsorted(np.asarray(loaded, dtype=np.uint64), src, side="right")
        assert len(set(regions.tolist())) >= 6                       # every listed region is a source: the search takes several steps
        assert (src >= loaded[-1]).any()                             # and the last, unlisted piece: no region behind it
    # the streams depend on the regions: the rule keeps pairs apart that the plain chain makes
    assert any(a[1][k] != b[1][k] for a, b in zip(res[1], res[0]) for k in a[1])
    h = binding.SlidingWindowSparseEMMatcher(lim)
    assert load_pieces(h, pieces[:6], pieces[6:]) == loaded
    got = device_batch(binding, h, contigs, binding.emit_params(1, lazyDecompressionSupport=lazy), loaded)
    hold(binding, got, res[lazy])
    h.close()


# ---- 2. pass 1 removes rows

def removed_rows(rows, min_len=256):
    """pass 1's removal restated (MBGC_Encoder.cpp:153-199): the locally computable predicate, removed alternately inside a run"""
    src, ln, dst = (rows[:, i].astype(np.int64) for i in range(3))
    n = len(rows)
    f = np.zeros(n, dtype=bool)
    d = src - dst
    f[1:n - 1] = (d[2:] == d[:-2]) & (d[1:-1] != d[:-2]) & (ln[1:-1] < min_len)
    rm = np.zeros(n, dtype=bool)
    for j in range(n):
        rm[j] = f[j] and not rm[j - 1] if j else False
    return rm


@functools.lru_cache(maxsize=None)
def removal_case():
    """Contigs that follow one diagonal of the reference and have a short foreign piece of the reference (36..60 bases, a match
    of its own, shorter than gapBreakingMatchMinLength) written over them every 80..150 bases: the foreign match breaks the gap
    between two matches of the main diagonal and is removed. Single substitutions split some main matches in two, so the removed
    rows fall on both parities of the row index."""
    rng = np.random.default_rng(4202)
    ref = ACGT[rng.integers(0, 4, 1_500_000)]
    lim = 4_000_000
    o = _orc.OracleMatcher(lim)
    loaded = load_pieces(o, [ref[:700_000], ref[700_000:]], [])
    contigs = []
    for k, (a, n) in enumerate([(10_000, 1_200_000), (720_000, 30_000), (300_000, 200_000)]):
        q = ref[a: a + n].copy()
        at = 70
        while at + 200 < n:
            w = int(rng.integers(36, 61))
            f = int(rng.integers(0, ref.size - 100))
            q[at: at + w] = ref[f: f + w]
            at += w + int(rng.integers(80, 150))
            if rng.random() < 0.3:                                   # a substitution inside the main stretch that follows
                q[at - 40] = ACGT[(int(np.searchsorted(ACGT, q[at - 40])) + 1) & 3]
        contigs.append(q)
    res = oracle_batch(o, contigs, _orc.emit_params(1), loaded)
    o.close()
    return ref, loaded, contigs, res, lim


def check_removal_case(res):
    rows_all = sum(len(r[2]) for r in res)
    removed_all = sum(r[3]["removedGapBreakingMatches"] for r in res)
    share = removed_all / rows_all
    assert share >= 0.05, share                                      # (the oracle's own count; this input: about 0.4)
    rows, cnt = res[0][2], res[0][3]
    rm = removed_rows(rows)
    assert int(rm.sum()) == cnt["removedGapBreakingMatches"]
    j = np.nonzero(rm)[0]
    kept_before = np.cumsum(~rm)[j]                                  # kept rows in front of every removed one
    assert int((~rm).sum()) > 2 * MSPAN                              # three spans of the pairing chain
    # removed rows at a chunk's first and last row and inside it; in front of a span's first kept row (= behind the last of the
    # span before), behind its first and in front of its last
    assert {0, CH - 1, 100} <= set((j % CH).tolist())
    assert {0, 1, MSPAN - 1, 2000} <= set((kept_before % MSPAN).tolist())
    # rows behind a removed one that abut it and are extended to the left: their source position moves
    src, ln, dst = (rows[:, i].astype(np.int64) for i in range(3))
    abut = rm[:-1] & (dst[:-1] + ln[:-1] == dst[1:])
    assert int(abut.sum()) > 100
    return share


def test_rows_removed_by_pass_1_keep_their_own_regions(binding):
    ref, loaded, contigs, res, lim = removal_case()
    check_removal_case(res)
    h = binding.SlidingWindowSparseEMMatcher(lim)
    assert load_pieces(h, [ref[:700_000], ref[700_000:]], []) == loaded
    hold(binding, device_batch(binding, h, contigs, binding.emit_params(1), loaded), res)
    h.close()


# ---- 6. the pairing chain's replays read the same values

def test_replayed_pairing_blocks_read_the_same_regions(binding, monkeypatch):
    monkeypatch.setenv("SWSEM_META_WARM", "0")                      # (read when the handle is made)
    ref, loaded, contigs, res, lim = removal_case()
    h = binding.SlidingWindowSparseEMMatcher(lim)
    assert load_pieces(h, [ref[:700_000], ref[700_000:]], []) == loaded
    hold(binding, device_batch(binding, h, contigs, binding.emit_params(1), loaded), res)
    st = h.emit_stats()
    assert st["blocks_not_accepted"] > 20 and st["groups_replayed"] > 10, st
    h.close()


# ---- 3. a ragged round

def test_ragged_round(binding):
    rng = np.random.default_rng(4303)
    base = ACGT[rng.integers(0, 4, 60_000)]
    lim = 2_000_000
    h, o = binding.SlidingWindowSparseEMMatcher(lim), _orc.OracleMatcher(lim)
    loaded = None
    for m in (h, o):
        ld = load_pieces(m, [base[:30_000], base[30_000:]], [])
        assert loaded is None or ld == loaded
        loaded = ld
    one_row = np.concatenate([ACGT[rng.integers(0, 4, 90)], base[41_000:41_050], ACGT[rng.integers(0, 4, 90)]])
    contigs = [mutated(rng, base[2_000:32_000], 0.01), base[100:120].copy(), one_row, mutated(rng, base[20_000:50_000], 0.01),
               ACGT[rng.integers(0, 4, 20_000)], mutated(rng, base[5_000:45_000], 0.012)]
    processed, target_idx = [0] * 6, [20 + k for k in range(6)]     # far enough ahead of the processed targets to be given up
    want = oracle_batch(o, contigs, _orc.emit_params(1), loaded, processed, target_idx)
    assert len(want[1][2]) == 0 and len(want[2][2]) == 1
    assert [w[0] == _orc.SKIPPED for w in want] == [False, False, False, False, True, False]
    hold(binding, device_batch(binding, h, contigs, binding.emit_params(1), loaded, processed, target_idx), want)
    h.close(); o.close()


# ---- 4. rounds through a wrapping buffer with locks; 5. an emission that is not the first of its batch

def rounds_on_device(binding, gs, lim, R):
    import torch
    from mbgc_amd.rounds import RoundRunner
    h = binding.SlidingWindowSparseEMMatcher(lim)
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
        runner.run_round(buf, offs)
    runner.flush()
    return h, runner


def hold_rounds(h, runner, o, b):
    for k in b["streams"]:
        assert bytes(runner.streams[k]) == b["streams"][k], k
    assert bytes(runner.locks_stream) == b["locks"] and bytes(runner.ref_ext_sizes) == b["refExtSize"]
    assert h.loaded_ref_length() == o.loaded_ref_length()
    assert np.array_equal(h.ht(), o.ht())


def test_wrapped_reference_and_locks(binding):
    """2.4 MB buffer, 41 genomes of 100 kB in rounds of 4: the buffer wraps, the matches' sources lie on both sides of the
    loading position and of the contigs' locks, and getMatchLoadedPos adds the buffer's length to the ones in front"""
    lim = 2_400_000
    base = synth.base_codes(100_000, 71)
    gs = [synth.genome(base, i, 0.01) for i in range(41)]
    o = _orc.OracleMatcher(lim)
    seen = []

    class Watch(_orc.OracleEmitter):
        def process(s, m, contig, lock, factor, processed, t, loaded):
            m = np.asarray(m).reshape(-1, 3)
            if len(m) and o.loaded_ref_length() > lim:
                src = m[:, 0]
                seen.append(((src < o.loading_position()).any(), (src > o.loading_position()).any(),
                             lock != NO_LOCK and (src < lock).any(), lock != NO_LOCK and (src > lock).any()))
            return super().process(m, contig, lock, factor, processed, t, loaded)
    b = _driver.encode_rounds(o, lambda: Watch(o), [gs[0]], [[g] for g in gs[1:]], 4)
    assert o.loaded_ref_length() > lim
    assert any(s[0] and s[1] for s in seen) and any(s[2] and s[3] for s in seen)
    h, runner = rounds_on_device(binding, gs, lim, 4)
    hold_rounds(h, runner, o, b)
    h.close(); o.close()


def test_a_later_emission_of_the_same_batch_keeps_the_lookups_behind_pass_1(binding):
    """one batch, emitted twice: all of its contigs (the first emission: lookups beside pass 1), then a retry pass over a subset
    in another order (not the first: k_emit_meta_regions behind pass 1, as before) — the rows pass 1 removes are in both"""
    import torch
    ref, loaded, contigs, res, lim = removal_case()
    h = binding.SlidingWindowSparseEMMatcher(lim)
    assert load_pieces(h, [ref[:700_000], ref[700_000:]], []) == loaded
    p = binding.emit_params(1)
    hold(binding, device_batch(binding, h, contigs, p, loaded), res)
    sub = [2, 0]
    n = h.emit_batch(p, contigs=sub, factors=[128] * 2, processed=[0] * 2, target_idx=[0] * 2, loaded=loaded)
    assert n == 2
    hold(binding, [h.emit_result(i)[:2] for i in range(2)], [res[c] for c in sub])
    h.close()
