"""The corpus of tests/_emitsizes.py is what it says it is — shown on the oracle alone, no device: a corpus that silently
matched nothing would pass empty on the device (tests/test_gpu_emit_size_classes.py). The constants it restates are the sources',
its plain runs have exactly the listed lengths, its related stretches sit on the wide extensions' threshold and are crossed by the
extensions, its hard tasks are the lanes it names, its batches are thin / not thin by the restated chunk rule — and the oracle,
sequential C without a threshold in it, decodes back to every contig at these shapes."""
import os
import re

import numpy as np
import pytest

import _emitsizes as E
import _orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbgc_amd", "csrc")
EXACT = E.params_key(1, 1, 0)                # enableExtensionsWithMismatches = 0: what lies between two matches is one plain run
EXT = E.params_key(1, 1, 1)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def has(src, text):
    """`text` stands in the source, whatever the white space"""
    return "".join(text.split()) in "".join(src.split())


@pytest.fixture(scope="module")
def small():
    return E.Referee(E.reference(), 4_000_000)


@pytest.fixture(scope="module")
def big():
    return E.Referee(E.big_reference(), 16_000_000)


@pytest.mark.parametrize("name", ["EMIT_THIN_MAX", "CH", "LONG_COPY_CAP", "LONG_COPY_MIN", "EXT_WIDE_MIN", "PLAIN_INLINE", "PIECE"])
def test_restated_constant_is_the_sources(name):
    src = source("swsem_emit.hip") + source("swsem_runtime_state.h")
    found = re.findall(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert len(found) == 1, "%s: defined %d times in swsem_emit.hip / swsem_runtime_state.h" % (name, len(found))
    assert int(found[0]) == getattr(E, name), "%s is %s in the sources, %d in tests/_emitsizes.py: the corpus no longer sits on it" % (
        name, found[0], getattr(E, name))


def test_restated_rules_are_the_sources():
    """the chunk rule, the choice between <4> and <1>, the tasks of a lane, and which side of every threshold takes which path"""
    emit_h, loader, emit = source("swsem_runtime_emit.h"), source("swsem_runtime_loader.h"), source("swsem_emit.hip")
    for src, text in [(emit_h, "const uint64_t nm = cg.n / (h->minLen ? h->minLen : 1) + 2;"),
                      (emit_h, "e.cap = (uint32_t) (nm + 2);"),
                      (emit_h, "E.chunkOwner.insert(E.chunkOwner.end(), (e.cap + CH - 1) / CH, (uint32_t) k);"),
                      (emit_h, "E.grid2b = (uint32_t) E.chunkOwner.size();"),
                      (loader, "const bool thin = E.grid2b <= EMIT_THIN_MAX;"),
                      (loader, "if (thin) k_emit_sizes<4><<<grid2, dim3(1024), 0, h->stream2>>>"),
                      (loader, "else k_emit_sizes<1><<<grid2, dim3(256), 0, h->stream2>>>"),
                      (loader, "if (thin) k_emit_write<4><<<grid2, dim3(1024), 0, h->stream2>>>"),
                      (loader, "else k_emit_write<1><<<grid2, dim3(256), 0, h->stream2>>>"),
                      (loader, "k_emit_copy_long<<<dim3(512), dim3(256), 0, h->stream2>>>"),
                      (emit, "return lane < (uint32_t) (WAVE / S) ? (int64_t) gx * 256 + wave * (WAVE / S) + lane : -1;"),
                      (emit, "if (z[4] <= PLAIN_INLINE)"),
                      (emit, "if (z[4] >= LONG_COPY_MIN) slot = atomicAdd(v.longCount, 1u);"),
                      (emit, "if (slot < LONG_COPY_CAP)"),
                      (emit, "k.litLeft > EXT_WIDE_MIN && k.litLeft <= UINT32_MAX"),
                      (emit, "wideL = litLeft > EXT_WIDE_MIN;"),
                      (emit, "wideL = leftLen > EXT_WIDE_MIN;")]:
        assert has(src, text), "the sources no longer say `%s`: restate the rule in tests/_emitsizes.py and move the corpus with it" % text
    assert re.search(r"constexpr\s+int\s+WAVE\s*=\s*64\s*;", source("swsem_device.h")), "a wave of 64 lanes is what LANES_HARD is laid out for"
    for n in (0, 1, 31, 32, 32 * 252 - 1, 32 * 252, 32 * 252 + 31, 32 * 252 + 32, 4_400_000):
        nm = n // 32 + 2
        cap = nm + 2
        assert E.chunks_of(n) == (cap + 255) // 256
    assert E.chunks_of(32 * 252 - 1) == 1 and E.chunks_of(32 * 253) == 2


def test_lanes_are_the_edges_of_a_wave_and_of_a_chunk():
    """chunk_task restated: <4> gives a wave 16 tasks, <1> 64, a block 256"""
    def lane_of(t, S):
        return (t % 256) // (64 // S), t % (64 // S), t // 256        # wave, lane, chunk
    assert [lane_of(t, 4) for t in (15, 16, 17)] == [(0, 15, 0), (1, 0, 0), (1, 1, 0)]
    assert [lane_of(t, 1) for t in (63, 64, 65)] == [(0, 63, 0), (1, 0, 0), (1, 1, 0)]
    for S in (4, 1):
        assert [lane_of(t, S)[2] for t in (255, 256, 257)] == [0, 1, 1]
        assert lane_of(255, S)[:2] == (256 * S // 64 - 1, 64 // S - 1) and lane_of(256, S)[:2] == (0, 0)
    assert set(E.LANES_HARD) == {15, 16, 17, 63, 64, 65, 255, 256, 257}


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plain_exact_stretches_are_the_listed_lengths(small, seed):
    for name, c in E.plain_contigs(seed).items():
        r = small.emit(name, c, EXACT)
        want = E.PLAIN_LENGTHS if "fwd" in name else E.PLAIN_LENGTHS[::-1]
        assert len(r["rows"]) == len(want) - 1 and r["counters"]["removedGapBreakingMatches"] == 0
        assert E.stretches(r["rows"], c.size) == want, name
        assert r["unmatched"] == sum(want)
        assert len(r["streams"]["literals"]) == sum(want) + len(r["rows"]) and r["streams"]["flags"] == b""    # plain runs and match marks only
    for n in (47, 48, 49, 32_767, 32_768, 32_769, 32_768 + 16_384 - 1, 32_768 + 16_384 + 1):
        assert n in E.PLAIN_LENGTHS
    assert E.PLAIN_INLINE + 1 in E.PLAIN_LENGTHS and E.LONG_COPY_MIN - 1 in E.PLAIN_LENGTHS and E.LONG_COPY_MIN + E.PIECE + 1 in E.PLAIN_LENGTHS
    assert any(n > E.LONG_COPY_MIN and n % 16 for n in E.PLAIN_LENGTHS) and any(E.PLAIN_INLINE < n < E.LONG_COPY_MIN and n % 16 for n in E.PLAIN_LENGTHS)
    # the two orders start the same run at other offsets modulo 16, in the query and in the literal stream
    starts = {}
    for name, c in E.plain_contigs(0).items():
        rows, at, lit = small.emit(name, c, EXACT)["rows"], 0, 0
        for t, n in enumerate(E.stretches(rows, c.size)):
            starts.setdefault(n, []).append((at % 16, lit % 16))
            at += n + (int(rows[t][1]) if t < len(rows) else 0)
            lit += n + 1
    assert sum(1 for n, v in starts.items() if v[0] != v[1]) >= len(starts) - 2


def test_dense_ladders_straddle_both_thresholds(small):
    """with the extensions on a stretch loses a few bytes at each end to them: the plain runs that are left still fall on both
    sides of PLAIN_INLINE and of LONG_COPY_MIN, since every stretch length around them is there and an extension into unrelated
    bases takes far less than the ladder's reach (96) — bounded here by what the oracle's counters say they took"""
    low = E.dense_contigs()["dense_low"]
    assert E.stretches(small.rows("dense_low", low), low.size) == E.DENSE_LOW
    assert min(E.DENSE_LOW) < E.PLAIN_INLINE - 10 and max(E.DENSE_LOW) > E.PLAIN_INLINE + 60
    got = []
    for k in range(E.DENSE_HIGH_PARTS):
        name = "dense_high_%d" % k
        c = E.dense_contigs()[name]
        want = E.DENSE_HIGH[k::E.DENSE_HIGH_PARTS]
        assert E.stretches(small.rows(name, c), c.size) == want
        got += want
        r = small.emit(name, c, EXT)
        taken = r["counters"]["extensionsMatchedChars"] + r["counters"]["extensionsMismatches"]
        assert 0 < taken < 60 * len(want), "the extensions took %d bytes off %d stretches" % (taken, len(want))    # (far from 96 each on average)
        assert min(want) < E.LONG_COPY_MIN - 90 and max(want) > E.LONG_COPY_MIN + 90
    assert sorted(got) == E.DENSE_HIGH


def test_zero_contigs_match_nothing(small):
    for name, c in E.zero_contigs().items():
        for key in (EXACT, EXT):
            r = small.emit(name, c, key)
            assert len(r["rows"]) == 0 and r["unmatched"] == c.size and r["streams"]["literals"] == c.tobytes()
    assert [c.size for c in E.zero_contigs().values()] == E.ZERO_LENGTHS


@pytest.mark.parametrize("seed", [0, 1])
def test_wide_stretches_sit_on_the_threshold_and_are_crossed(small, seed):
    for name, c in E.wide_contigs(seed).items():
        r = small.emit(name, c, EXT)
        assert r["counters"]["removedGapBreakingMatches"] == 0
        between = E.stretches(r["rows"], c.size)
        between = between[1:-1] if "gap" in name else between
        assert between == E.WIDE_LENGTHS, name                          # (no match inside a related stretch: RUN_CAP)
        for n in (191, 192, 193, 194):
            assert n in between
        assert r["counters"]["extensionsMatchedChars"] > 0
        if "_008_" in name:
            assert 2 * r["counters"]["extensionsMatchedChars"] >= sum(E.WIDE_LENGTHS), (name, r["counters"])
        if "gap" in name:                                               # every stretch is a gap: one flag per byte of it but the first, and the closing one
            assert len(r["streams"]["flags"]) >= sum(E.WIDE_LENGTHS) - len(E.WIDE_LENGTHS)


def test_lanes_hard_tasks_are_where_they_are_said_to_be(small):
    c = E.lanes_contig()["lanes"]
    for key in (EXT, EXACT):
        r = small.emit("lanes", c, key)
        assert r["counters"]["removedGapBreakingMatches"] == 0 and len(r["rows"]) == E.LANES_TASKS - 1
        between = E.stretches(r["rows"], c.size)
        assert [t for t, n in enumerate(between) if n > 1_000] == list(E.LANES_HARD)
        assert all(n == (E.LANES_RELATED + E.LANES_UNRELATED if t in E.LANES_HARD else 40) for t, n in enumerate(between))
    # the related part is crossed (a wide right extension), what is left is a wide left extension's and a listed run
    ext = small.emit("lanes", c, EXT)["counters"]
    assert ext["extensionsMatchedChars"] >= len(E.LANES_HARD) * E.LANES_RELATED // 2
    assert E.LANES_RELATED > E.EXT_WIDE_MIN and E.LANES_UNRELATED - 1_000 > E.LONG_COPY_MIN


def test_batches_are_thin_or_not_as_they_say():
    bs = E.batches()
    hard = set(E.hard_contigs())
    kinds = {}
    for b in bs:
        kinds.setdefault(b["kind"], set()).update(n for n in b["names"] if n in hard)
        nchunks = sum(E.chunks_of(c.size) for c in b["contigs"])
        assert b["expected_thin"] == (nchunks <= E.EMIT_THIN_MAX)
        assert b["expected_thin"] == (b["kind"] == "alone"), b["name"]
    assert kinds["alone"] == hard and kinds["crowd"] == hard and kinds["beside_big"] == hard
    crowd = [b for b in bs if b["kind"] == "crowd"][0]
    assert len(crowd["contigs"]) - len(hard) == 600 > E.EMIT_THIN_MAX
    where = [i for i, n in enumerate(crowd["names"]) if n in hard]
    assert where[0] > 0 and max(np.diff(where)) > 1                    # scattered among the fillers
    beside = [b for b in bs if b["kind"] == "beside_big"][0]
    assert beside["names"][0] == "big" and E.chunks_of(beside["contigs"][0].size) > E.EMIT_THIN_MAX


def test_overflow_batch_fills_the_list(small):
    b = E.overflow_batch()
    assert not b["expected_thin"]
    long_ones = [c for c in b["contigs"] if c.size >= E.LONG_COPY_MIN]
    assert len(long_ones) > E.LONG_COPY_CAP + 100
    assert len(b["contigs"]) == E.OVERFLOW_RUNS + E.OVERFLOW_MIXED
    assert 140e6 < sum(c.size for c in b["contigs"]) < 150e6
    runs = [(n, c) for n, c in zip(b["names"], b["contigs"]) if n.startswith("run_")]
    assert len(runs) == E.OVERFLOW_RUNS and {c.size - E.LONG_COPY_MIN for _, c in runs} == set(range(37))
    for n, c in runs[::43]:                                             # one run of plain == n each (the device test asks the oracle about all of them)
        assert len(small.rows(n, c)) == 0
    mixed = [n for n in b["names"] if not n.startswith("run_")]
    assert sum(n.startswith("plain_") for n in mixed) >= 4 and sum(n.startswith("wide_") for n in mixed) >= 4


def test_hard_contigs_have_the_same_rows_beside_the_big_contig(small, big):
    """the large reference keeps the small one in front: the hard contigs' rows are the same against either, so their streams
    from `beside_big` can be held to those from `alone`"""
    for name, c in E.hard_contigs().items():
        assert np.array_equal(small.rows(name, c), big.rows(name, c)), name
    c = E.big_contig()
    rows = big.rows("big", c)
    assert len(rows) > 20_000 and int(rows[:, 1].sum()) > c.size // 2


@pytest.mark.parametrize("mode", [1, 3])
def test_oracle_streams_decode_back_to_the_contig(small, mode):
    key = E.params_key(mode, 1, 1)
    po = E.params_of(_orc.emit_params, key)
    ref = small.o.ref(small.o.max_ref_length())
    everything = dict(E.hard_contigs())
    everything.update(E.fillers())
    for seed in (1, 2, 3):
        everything.update(E.plain_contigs(seed))
    everything.update(E.wide_contigs(1))
    for name, c in everything.items():
        r = small.emit(name, c, key)
        back, un = _orc.decode_contig(ref, po, r["streams"], _orc.NO_LOCK, c.size + 16)
        assert back.size == c.size and np.array_equal(back, c), name
        assert un == (r["unmatched"] & 0xFFFFFFFF)


def test_oracle_streams_of_the_big_contig_decode_back(big):
    key = E.params_key(1, 1, 1)
    po = E.params_of(_orc.emit_params, key)
    ref = big.o.ref(big.o.max_ref_length())
    c = E.big_contig()
    r = big.emit("big", c, key)
    back, un = _orc.decode_contig(ref, po, r["streams"], _orc.NO_LOCK, c.size + 16)
    assert back.size == c.size and np.array_equal(back, c)
