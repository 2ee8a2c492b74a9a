"""The stitch's rejected blocks: replayed ahead of the walk by k_stitch_replay (one wave each, from the state the
predecessor's speculative chain ended in) and taken by k_stitch when that state was the true one, replayed in place
otherwise. Rows against the oracle on short blocks (SWSEM_RB=1 / 2: 1024 / 2048 positions) behind short warm-ups
(SWSEM_OVERLAP=64 / 128 / 256), which reject many blocks, some of them one after the other; both block kernels; a
buffer that has wrapped (the LAPS instantiations); several contigs in one batch. The counters must show both paths.

What the seeds below gave on an MI355X, summed over the 12 cases of test_short_blocks_behind_short_warmups: 2556 blocks rejected, 784 of them taken from k_stitch_replay, 16 of its replays
refused by the walk and redone in place (the other rejected blocks were no candidates: with an empty warm-up stack most
blocks look beneath it, which the quick test cannot decide)."""
import numpy as np
import pytest

import _orc
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
NO_LOCK = _orc.NO_LOCK

# (contigs, length, divergence, seed): the three of test_resolve_variants_agree_with_oracle and one of 300 000-base contigs
COLLECTIONS = [(4, 120_000, 0.01, 41), (4, 120_000, 0.0005, 42), (4, 120_000, 0.1, 43), (3, 300_000, 0.01, 44)]
TOTALS = {"replayed_blocks": 0, "replays_precomputed": 0, "candidates_unused": 0, "candidates_refused": 0, "cases": 0}


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    return b


_expected = {}


def collection(key):
    """the genomes of a collection and the oracle's rows for each of them after the first (computed once)"""
    if key not in _expected:
        n, length, div, seed = key
        base = synth.base_codes(length, seed)
        gs = [synth.genome(base, i, div) for i in range(n)]
        o = _orc.OracleMatcher(8_000_000)
        o.load_ref(gs[0], load_rc=True)
        rows = []
        for g in gs[1:]:
            rows.append(o.match(g))
            o.load_ref(g)
        o.close()
        _expected[key] = (gs, rows)
    return _expected[key]


def add_counts(h):
    st = h.batch_stats()
    for k in TOTALS:
        if k != "cases":
            TOTALS[k] += int(st[k])
    assert st["replays_precomputed"] + st["candidates_refused"] <= st["replayed_blocks"], st
    return st


def run_case(binding, monkeypatch, rb, overlap, chains):
    monkeypatch.setenv("SWSEM_RB", str(rb))
    monkeypatch.setenv("SWSEM_OVERLAP", str(overlap))
    if chains == 1:
        monkeypatch.setenv("SWSEM_CHAINS", "1")
    else:
        monkeypatch.delenv("SWSEM_CHAINS", raising=False)
    for key in COLLECTIONS:
        gs, rows = collection(key)
        h = binding.SlidingWindowSparseEMMatcher(8_000_000)
        h.load_ref(gs[0], load_rc=True)
        for g, exp in zip(gs[1:], rows):
            assert np.array_equal(h.match(g), exp), (rb, overlap, chains, key)
            add_counts(h)
            h.load_ref(g)
        h.close()
    TOTALS["cases"] += 1


CASES = [(rb, ov, ch) for ch in (4, 1) for rb in (1, 2) for ov in (64, 128, 256)]


@pytest.mark.parametrize("rb,overlap,chains", CASES)
def test_short_blocks_behind_short_warmups(binding, monkeypatch, rb, overlap, chains):
    run_case(binding, monkeypatch, rb, overlap, chains)


def test_wrapped_buffer(binding, monkeypatch):
    """a buffer of 500 000 bytes under 120 000-base genomes: from the third query on it has wrapped (LAPS = true)"""
    monkeypatch.setenv("SWSEM_RB", "1")
    monkeypatch.setenv("SWSEM_OVERLAP", "64")
    base = synth.base_codes(120_000, 45)
    gs = [synth.genome(base, i, 0.01) for i in range(7)]
    h, o = binding.SlidingWindowSparseEMMatcher(500_000), _orc.OracleMatcher(500_000)
    for m in (h, o):
        m.disable_sliding_window()
        m.load_ref(gs[0], load_rc=True)
    replayed = 0
    for i, g in enumerate(gs[1:]):
        assert np.array_equal(h.match(g), o.match(g)), i
        replayed += add_counts(h)["replayed_blocks"]
        for m in (h, o):
            m.load_ref(g)
    assert o.loaded_ref_length() > 500_000 and h.loading_position() == o.loading_position()
    assert replayed > 0
    h.close(); o.close()


def test_several_contigs_in_one_batch(binding, monkeypatch):
    """contigs of unequal length (one shorter than a block, one shorter than a K-mer) in one match_batch_dev call"""
    import torch
    monkeypatch.setenv("SWSEM_RB", "1")
    monkeypatch.setenv("SWSEM_OVERLAP", "64")
    gs, _ = collection(COLLECTIONS[0])
    h, o = binding.SlidingWindowSparseEMMatcher(8_000_000), _orc.OracleMatcher(8_000_000)
    for m in (h, o):
        m.load_ref(gs[0], load_rc=True)
    contigs = [gs[1], gs[2][:70_001], gs[2][70_001:], gs[3][:900], gs[3][900:913], gs[3][913:]]
    offs = np.zeros(len(contigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([c.size for c in contigs])
    buf = torch.from_numpy(np.concatenate(contigs)).to("cuda:0")
    torch.cuda.synchronize()
    h.match_batch_dev(buf.data_ptr(), offs, 32, None)
    counts = h.batch_counts()
    for i, c in enumerate(contigs):
        e = o.match(c)
        assert counts[i] == len(e), i
        assert np.array_equal(h.batch_matches(i, counts[i]), e), i
    st = add_counts(h)
    assert st["replayed_blocks"] > 0, st
    h.close(); o.close()


def test_both_replay_paths_were_taken(binding, monkeypatch):
    """over the parameter set: blocks taken from k_stitch_replay, and replays of it refused and redone in place"""
    if TOTALS["cases"] < len(CASES):                       # (run on its own: the parameter set first)
        for k in TOTALS:
            TOTALS[k] = 0
        for rb, ov, ch in CASES:
            run_case(binding, monkeypatch, rb, ov, ch)
    print("stitch replay counters over the parameter set:", TOTALS)
    assert TOTALS["replayed_blocks"] > 0, TOTALS
    assert TOTALS["replays_precomputed"] > 0, TOTALS
    assert TOTALS["candidates_refused"] > 0, TOTALS


def test_default_warmup_is_adapted_and_the_switch_fixes_it(binding, monkeypatch):
    """SWSEM_OVERLAP unset leaves a fresh handle's blocks accepted as before (the bound of test_speculation_mostly_accepted
    on a third of its input); SWSEM_OVERLAP=0 — no warm-up at all — rejects nearly every block and still gives the rows"""
    gs, rows = collection(COLLECTIONS[3])
    monkeypatch.delenv("SWSEM_OVERLAP", raising=False)
    monkeypatch.delenv("SWSEM_RB", raising=False)
    h = binding.SlidingWindowSparseEMMatcher(8_000_000)
    h.load_ref(gs[0], load_rc=True)
    assert np.array_equal(h.match(gs[1]), rows[0])
    nblocks = (300_000 - 27 + 2047) // 2048
    assert h.batch_stats()["replayed_blocks"] <= nblocks // 10, h.batch_stats()
    h.close()
    monkeypatch.setenv("SWSEM_OVERLAP", "0")
    h = binding.SlidingWindowSparseEMMatcher(8_000_000)
    h.load_ref(gs[0], load_rc=True)
    assert np.array_equal(h.match(gs[1]), rows[0])
    st = h.batch_stats()
    assert st["replayed_blocks"] > nblocks // 2, st
    h.close()

