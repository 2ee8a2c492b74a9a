"""The corpus of tests/_decsizes.py is what it says it is — shown on the oracle alone, no device. The constants it restates are the
sources' (with the three comparison lines of k_decode_fill and the windows' reload conditions quoted). Family A, the streams
written by hand: the oracle's decoder (orc_decode_contig_bounded, sequential C without a threshold in it) reads every one of them to
the end of all six streams and gives exactly the numpy expectation — they are well-formed MBGC streams, not merely something the
device accepts — and its per-match trace shows the plain runs, match lengths and record indices the corpus names. Family B, written
by the oracle's encoder from the pieces as rows: the oracle's decoder gives the contig back, and its trace shows per match the right
extension's length and which of start / middle / end it carries, on both sides of DEC_WIDE_MIN.

A planted piece of 40 bases does not survive the encoder (processMatches removes a match shorter than gapBreakingMatchMinLength = 256
that breaks a gap): `planted_short` claims exactly that, `planted_long` (260 bases) is the contig whose gaps span a record of another
diagonal. With gapDepthMismatchesEncoding = 2, the value of every mode, a gap spans at most one such record, so REC_GAP_MIDDLE does
not occur in streams an encoder writes; no case claims it."""
import collections
import os
import re

import numpy as np
import pytest

import _decsizes as D
import _emitsizes as E
import _orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mbgc_amd", "csrc")
G, START, MIDDLE, END = _orc.REC_GAP, _orc.REC_GAP_START, _orc.REC_GAP_MIDDLE, _orc.REC_GAP_END


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def has(src, text):
    """`text` stands in the source, whatever the white space"""
    return "".join(text.split()) in "".join(src.split())


@pytest.fixture(scope="module")
def ref():
    return D.ref_buffer()


def test_restated_constants_and_rules_are_the_sources():
    dec, run, dev = source("swsem_decode.hip"), source("swsem_runtime_decode.h"), source("swsem_device.h")
    found = re.findall(r"constexpr\s+uint64_t\s+DEC_WIDE_MIN\s*=\s*(\d+)\s*;", dec)
    assert found == [str(D.DEC_WIDE_MIN)], "DEC_WIDE_MIN is %s in swsem_decode.hip, %d in tests/_decsizes.py: the corpus no longer sits on it" % (found, D.DEC_WIDE_MIN)
    assert re.search(r"constexpr\s+int\s+WAVE\s*=\s*%d\s*;" % D.WAVE, dev)
    assert D.DW_WINDOW == 4 * D.WAVE and D.COPY_ROUND == 16 * D.WAVE and D.FILL_THREADS == 4 * D.WAVE
    for src, text in [
            # the three choices of k_decode_fill
            (dec, "if (plain <= DEC_WIDE_MIN) for (uint64_t k = 0; k < plain; k++) t[k] = s[k];"),
            (dec, "else { copyLen[0] = plain; copySrc[0] = s; copyDst[0] = t; }"),
            (dec, "if (r.len <= DEC_WIDE_MIN) {"),
            (dec, "} else { copyLen[1] = r.len; copySrc[1] = s; copyDst[1] = t; }"),
            (dec, "wideRight = (r.flags & REC_GAP) != 0 && r.rightLen > DEC_WIDE_MIN;"),
            # the wave copy: 16 bytes per lane, a round of 16 * WAVE, a byte tail
            (dec, "for (uint64_t o = 16 * (uint64_t) lane; o < len; o += 16 * WAVE) {"),
            (dec, "if (o + 16 <= len) { const uint4 x = ld_u128(src + o); __builtin_memcpy(dst + o, &x, 16); }"),
            (dec, "else for (uint64_t k = o; k < len; k++) dst[k] = src[k];"),
            # the wave's right extension: 64 bytes per iteration from s0 on, the code's place by popcount and rank
            (dec, "const uint32_t s0 = (rl64d(r.flags, l) & REC_GAP_START) ? 1u : 0u;"),
            (dec, "for (uint64_t i0 = s0; i0 < n && !bad; i0 += WAVE) {"),
            (dec, "t.litPos = lit0 + rank + (uint64_t) __popcll(set & ((1ull << lane) - 1ull));"),
            (dec, "rank += (uint64_t) __popcll(set);"),
            # one thread per record, 256 of them, the grid by the longest contig; blocks beyond a contig's records return
            (dec, "__global__ void __launch_bounds__(256) k_decode_fill("),
            (dec, "if (plans[c].unmatched < 0 || (uint64_t) blockIdx.x * blockDim.x >= plans[c].nrec) return;"),
            (run, "k_decode_fill<<<dim3((unsigned) ((maxRec + 255) / 256), (unsigned) cn), dim3(256), 0, h->stream>>>"),
            # the plan's windows: 64 bytes as a ballot mask, 64 dwords
            (dec, "if (from - d.lit.base >= (uint64_t) WAVE) bw_load<true>(d.lit, from);"),
            (dec, "from = d.lit.base + WAVE;"),
            (dec, "if (i - d.fl.base >= (uint64_t) WAVE) bw_load<false>(d.fl, i);"),
            (dec, "if (d.flPos - d.fl.base >= (uint64_t) WAVE) bw_load<false>(d.fl, d.flPos);"),
            (dec, "const uint64_t o = pos + 4ull * (threadIdx.x & (WAVE - 1));"),
            (dec, "if (pos < w.base || pos + width > w.base + 4 * WAVE) dw_load(w, pos);"),
            (dec, "__global__ void __launch_bounds__(WAVE) k_decode_plan(")]:
        assert has(src, text), "the sources no longer say `%s`: restate the rule in tests/_decsizes.py and move the corpus with it" % text


def test_reference_buffer_is_the_matchers(ref):
    assert np.array_equal(D.referee().o.ref(D.REF_MAX), ref)


# ---- family A ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand_traces(ref):
    """{(set, contig): the oracle's result with its per-match trace}: once, for every test that asks"""
    out = {}
    for sname, _, _ in D.A_SETS:
        p = D.a_params(_orc.emit_params, sname)
        for name, h in D.hand_contigs().items():
            s = h.streams(bool(p.frugal64bitLenEncoding), bool(p.enable40bitReference))
            out[sname, name] = (s, _orc.decode_contig_bounded(ref, D.REF_MAX, p, s, _orc.NO_LOCK, h.expect(ref).size + 16, recs=h.nrec))
    return out


@pytest.mark.parametrize("sname", [n for n, _, _ in D.A_SETS])
def test_hand_written_streams_are_well_formed(ref, hand_traces, sname):
    p = D.a_params(_orc.emit_params, sname)
    assert p.enableExtensionsWithMismatches == 0 and p.gapDepthOffsetEncoding and p.lazyDecompressionSupport == 1
    d = _orc.emit_params(1)
    assert bool(p.frugal64bitLenEncoding) == (bool(d.frugal64bitLenEncoding) != (sname == "m1-plainlen")) and p.enable40bitReference == (sname == "m1-bit40")
    for name, h in D.hand_contigs().items():
        s, r = hand_traces[sname, name]
        want = h.expect(ref)
        assert r["unmatched"] == h.unmatched() == sum(len(x[0]) for x in h.recs) + len(h.tail), (sname, name)
        assert r["dest"].size == want.size and np.array_equal(r["dest"], want), (sname, name)
        assert r["cur"] == [len(x) for x in s], (sname, name)            # all six cursors at the streams' ends
        assert len(s[D.FLAGS]) == 0 and len(s[D.OFF]) == 4 * (len(h.recs) - len(h.paired)) and len(s[D.OFF5]) == (len(h.recs) - len(h.paired) if sname == "m1-bit40" else 0)
        assert [(x["plain"], x["src"], x["matchLen"], x["leftLen"], x["rightLen"], x["flags"], x["skipOffset"]) for x in r["recs"]] == \
               [(len(pl), src, n, 0, 0, 0, int(i in h.paired)) for i, (pl, src, n) in enumerate(h.recs)], (sname, name)
        # the decoder's own back-door: the same streams through the form the reference pins
        back, un = _orc.decode_contig(ref, p, dict(zip(_orc.STREAM_NAMES, s)), _orc.NO_LOCK, want.size + 16)
        assert np.array_equal(back, want) and un == h.unmatched()


def test_hand_written_contigs_sit_on_the_edges(hand_traces):
    H = D.hand_contigs()
    W = D.DEC_WIDE_MIN
    recs = lambda name: hand_traces["m1", name][1]["recs"]
    # plain runs: every length 0..260 once, in both orders; every mark at every place of a 64-byte window; every 16-byte tail on
    # both sides of the threshold; other destination alignments in the reverse order
    marks, aligns = set(), {}
    for tag in ("fwd", "rev"):
        r = recs("plain_dense_" + tag)
        assert sorted(x["plain"] for x in r) == list(range(261))
        lit = 0
        for x in r:
            lit += x["plain"]
            marks.add(lit % D.WAVE)
            aligns.setdefault(x["plain"], []).append(x["destAt"] % 16)
            lit += 1
    assert marks == set(range(D.WAVE))
    assert {n % 16 for n in range(W - 15, W + 1)} == {n % 16 for n in range(W + 1, W + 17)} == set(range(16))
    assert sum(1 for v in aligns.values() if v[0] != v[1]) >= 240
    assert {W - 1, W, W + 1} <= set(aligns)
    long_ = [x["plain"] for x in recs("plain_long")] + [len(H["plain_long"].tail)]
    assert long_ == list(D.PLAIN_LONG) and len(H["plain_long"].tail) == 100_003      # one of them is the tail record's
    for n in (D.COPY_ROUND - 1, D.COPY_ROUND, D.COPY_ROUND + 1, D.COPY_ROUND + 15, D.COPY_ROUND + 16, D.COPY_ROUND + 17, 2 * D.COPY_ROUND):
        assert n in D.PLAIN_LONG and n in D.MATCH_LONG
    # matches: every length 1..260, src % 16 over 0..15 on both sides of the threshold
    for tag in ("fwd", "rev"):
        r = recs("match_dense_" + tag)
        assert sorted(x["matchLen"] for x in r) == list(range(1, 261)) and all(x["plain"] == 3 for x in r)
        assert {x["src"] % 16 for x in r if W - 16 < x["matchLen"] <= W} == {x["src"] % 16 for x in r if W < x["matchLen"] <= W + 16} == set(range(16))
    assert [x["matchLen"] for x in recs("match_long")] == list(D.MATCH_LONG)
    s = hand_traces["m1", "match_long"][0][D.LEN]
    assert len(s) == 2 * 10 + 6 * 3 and s[18:20] == b"\xfe\xff" and s[20:22] == b"\xff\xff" and s[22:26] == (65_535).to_bytes(4, "little")   # the 0xFFFF + 4-byte form
    # the long record's mapLen entry on both sides of the dword window's end
    spans = {}
    for at in D.LEN_WINDOW_AT:
        name = "len_window_%d" % at
        r = recs(name)
        assert len(r) == D.LEN_WINDOW_RECORDS + 1 and [i for i, x in enumerate(r) if x["matchLen"] != 40] == [at] and r[at]["matchLen"] == D.LEN_WINDOW_LONG
        s = hand_traces["m1", name][0][D.LEN]
        assert s[2 * at:2 * at + 2] == b"\xff\xff" and int.from_bytes(s[2 * at + 2:2 * at + 6], "little") == D.LEN_WINDOW_LONG
        spans[at] = (2 * at, 2 * at + 2, 2 * at + 6)
        s4 = hand_traces["m1-plainlen", name][0][D.LEN]
        assert len(s4) == 4 * (D.LEN_WINDOW_RECORDS + 1) and int.from_bytes(s4[4 * at:4 * at + 4], "little") == D.LEN_WINDOW_LONG
        assert len(hand_traces["m1-bit40", name][0][D.OFF5]) == D.LEN_WINDOW_RECORDS + 1
    assert spans[125] == (250, 252, 256)                                   # the 4-byte read ends on the window's last byte
    assert spans[126][1] < D.DW_WINDOW < spans[126][2]                     # ... straddles its end
    assert spans[127][1] == D.DW_WINDOW                                    # the 2-byte read ends on it, the 4-byte read starts behind it
    assert spans[128][0] == D.DW_WINDOW and spans[129][0] == D.DW_WINDOW + 2
    # lanes: wide work at the edges of a wave and of a block, and a wave whose 64 lanes all have some
    r = recs("lanes")
    assert len(r) == D.LANES_RECORDS and [i for i, x in enumerate(r) if x["plain"] > W] == [i for i, x in enumerate(r) if x["matchLen"] > W] == list(D.LANES_WIDE)
    assert set(D.LANES_WIDE) == {0, D.WAVE - 1, D.WAVE, D.WAVE + 1, D.FILL_THREADS - 1, D.FILL_THREADS, D.FILL_THREADS + 1, 2 * D.FILL_THREADS - 1}
    assert all((x["plain"], x["matchLen"]) == ((1_000, 1_000) if i in D.LANES_WIDE else (3, 40)) for i, x in enumerate(r))
    r = recs("lanes_full")
    wide = [i for i, x in enumerate(r) if x["plain"] > W and x["matchLen"] > W]
    assert wide == list(range(D.WAVE, 2 * D.WAVE)) and len({x["plain"] for x in r[D.WAVE:2 * D.WAVE]}) == len({x["matchLen"] for x in r[D.WAVE:2 * D.WAVE]}) == D.WAVE
    assert all(x["plain"] <= W and x["matchLen"] <= W for i, x in enumerate(r) if i not in wide)
    # gapDelta bytes that differ across the dword window's end, wherever an earlier reload put the window's base
    gd = hand_traces["m1", "pairs"][0][D.GAP]
    assert len(gd) == D.PAIRS_RECORDS - 1 and set(gd) == {0, 1} and gd[0] == 0 and gd[D.DW_WINDOW] == 1
    assert all(sum(gd[k] != gd[k + D.DW_WINDOW] for k in range(b, len(gd) - D.DW_WINDOW, D.DW_WINDOW)) >= 2 for b in range(4))
    # tiny: record counts around a wave and a block, tails around the threshold
    assert [H["tiny_tail_%d" % n].nrec for n in D.TINY_TAILS] == [1] * 5 and [len(H["tiny_tail_%d" % n].tail) for n in D.TINY_TAILS] == [0, 1, W, W + 1, 5_000]
    assert [H["tiny_nrec_%d" % n].nrec for n in D.TINY_NREC] == [2, D.WAVE, D.WAVE + 1, D.FILL_THREADS, D.FILL_THREADS + 1]
    # contigs of very different record counts side by side: the grid is sized by the largest
    assert min(h.nrec for h in H.values()) == 1 and max(h.nrec for h in H.values()) > 2 * D.FILL_THREADS


# ---- family B ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gap_traces(ref):
    out = {}
    R = D.referee()
    for sname, key in D.B_SETS:
        po = E.params_of(_orc.emit_params, key)
        for name, g in D.gap_contigs().items():
            e = R.emit_rows(g, key)
            out[sname, name] = (e, _orc.decode_contig_bounded(ref, D.REF_MAX, po, e["streams"], _orc.NO_LOCK, g.contig.size + 16, recs=len(g.rows) + 1))
    return out


def test_gap_contigs_are_built_as_said(ref):
    """the rows are matches bounded by a mismatch on either side; first and last byte of every stretch differ from the reference;
    the patterns are the substitutions that were made; a dense pattern leaves the matcher nothing but the pieces"""
    R = D.referee()
    for name, g in D.gap_contigs().items():
        c = g.contig
        for k, (src, n, dst) in enumerate(g.rows.tolist()):
            assert np.array_equal(c[dst:dst + n], ref[src:src + n]), (name, k)
            assert dst == 0 or c[dst - 1] != ref[src - 1], (name, k)
            assert dst + n == c.size or c[dst + n] != ref[src + n], (name, k)
        diag = int(g.rows[0][0])
        for at, n, k in g.stretches:
            assert c[at] != ref[diag + at] and c[at + n - 1] != ref[diag + at + n - 1], (name, at)
    for tag, _ in D.PATTERNS:
        g = D.gap_contigs()["gap_" + tag]
        diag = int(g.rows[0][0])
        assert [n for _, n, _ in g.stretches] == D.STRETCH_LENGTHS
        for at, n, _ in g.stretches:
            sub = set(np.flatnonzero(g.contig[at:at + n] != ref[diag + at:diag + at + n]).tolist())
            if tag == "none":
                want = {0, n - 1}
            elif tag == "every":
                want = set(range(n))
            elif tag == "mod64":
                want = {k for k in range(n) if k % 64 in (0, 1, 63)} | {0, n - 1}
            elif tag.startswith("single"):
                want = {0, n - 1} | ({int(tag[6:])} if int(tag[6:]) < n else set())
            else:
                rate = len(sub) / n
                assert (0.06 < rate < 0.16 if tag == "rate08" else 0.2 < rate < 0.33) or n < 200, (tag, n, rate)
                kept = np.diff(np.array([-1] + sorted(sub) + [n])) - 1
                assert kept.max() <= E.RUN_CAP
                continue
            assert sub == want, (tag, at, n)
    assert {1, 63, 64, 65, 127, 128, 129} == set(D.SINGLES)
    for n in (150, 191, 192, 193, 194, 260, 1_023, 1_024, 1_025, 3_000):
        assert n in D.STRETCH_LENGTHS
    for name in ["gap_" + t for t in D.DENSE_PATTERNS] + ["gap_lanes", "planted_long"]:
        g = D.gap_contigs()[name]
        m = R.rows(name, g.contig)
        assert m.shape == g.rows.shape and np.array_equal(m, g.rows), "%s: the matcher's rows are not the pieces" % name


@pytest.mark.parametrize("sname", [n for n, _ in D.B_SETS])
def test_oracle_decodes_the_gap_contigs_back_in_the_claimed_shapes(gap_traces, sname):
    W = D.DEC_WIDE_MIN
    seen = collections.Counter()
    for name, g in D.gap_contigs().items():
        e, r = gap_traces[sname, name]
        assert r["unmatched"] == (e["unmatched"] & 0xFFFFFFFF) and r["cur"] == [len(s) for s in e["streams"]], (sname, name)
        assert r["dest"].size == g.contig.size and np.array_equal(r["dest"], g.contig), (sname, name)
        assert e["counters"]["removedGapBreakingMatches"] == g.removed, (sname, name)
        recs = r["recs"]
        for x in recs:
            assert x["plain"] == 0 and x["leftLen"] == 0, (sname, name, x)  # everything between two matches is a gap's right extension
            if x["rightLen"]:
                seen[x["flags"], x["rightLen"] > W] += 1
        if g.removed:
            # the planted pieces are gone: one record per piece of the region, each gap spans its whole stretch, planted piece included
            assert len(recs) == len(g.rows) - g.removed
            spans = [a + D.FOREIGN_SHORT + b for (_, a, _), (_, b, _) in zip(g.stretches[0::2], g.stretches[1::2])]
            assert [(x["flags"], x["rightLen"]) for x in recs[:-1]] == [(G | START | END, n) for n in spans] and min(spans) > W
            continue
        assert len(recs) == len(g.rows) and [(x["src"], x["matchLen"]) for x in recs] == [(s, n) for s, n, _ in g.rows.tolist()], (sname, name)
        assert (recs[-1]["flags"], recs[-1]["rightLen"]) == (0, 0)
        for at, n, k in g.stretches:
            x = recs[k]
            want = G | (END if k in g.planted else START) | (0 if g.planted else END)
            assert x["rightLen"] == n and x["flags"] == want and x["destAt"] + x["matchLen"] == at, (sname, name, k, x)
            assert x["skipOffset"] == (0 if k == 0 or k in g.planted else 1), (sname, name, k)   # the region's pieces pair with each other
        if name.startswith("gap_") and name != "gap_lanes":
            assert [recs[k]["rightLen"] for _, _, k in g.stretches] == D.STRETCH_LENGTHS
    # every claimed combination on either side of the threshold
    for flags in (G | START | END, G | START, G | END):
        assert seen[flags, False] > 0 and seen[flags, True] > 0, (sname, flags, dict(seen))
    assert not any(f & MIDDLE for f, _ in seen)
    # lengths W - 1 .. W + 2 for every combination; a wide extension with s0 = 0 that is no multiple of 64 and one beyond a round of 64
    for name, flagsets in (("gap_rate08", (G | START | END,)), ("planted_long", (G | START, G | END))):
        recs = gap_traces[sname, name][1]["recs"]
        for flags in flagsets:
            got = {x["rightLen"] for x in recs if x["flags"] == flags}
            assert {W - 1, W, W + 1, W + 2} <= got and max(got) >= 1_024, (sname, name, flags, sorted(got))
    # wide gap extensions at the edges of a wave and of a block
    g = D.gap_contigs()["gap_lanes"]
    recs = gap_traces[sname, "gap_lanes"][1]["recs"]
    assert [i for i, x in enumerate(recs) if x["rightLen"] > W] == list(D.B_LANES_WIDE) == [0, D.WAVE - 1, D.WAVE, D.FILL_THREADS - 1, D.FILL_THREADS]
    assert all(x["rightLen"] == (D.B_LANES_WIDE_LEN if i in D.B_LANES_WIDE else 40) for i, x in enumerate(recs[:-1]))
    # set flags at the window's edges: the flag stream of gap_mod64 has set flags at offsets 63, 64 and 65 of a stretch's walk
    fl = np.frombuffer(gap_traces[sname, "gap_mod64"][0]["streams"][D.FLAGS], dtype=np.uint8)
    assert fl.size >= sum(D.STRETCH_LENGTHS) - len(D.STRETCH_LENGTHS) and 0 < int((fl != 0).sum()) < fl.size // 8
    assert {int(i) % D.WAVE for i in np.flatnonzero(fl)} == set(range(D.WAVE))   # a set flag at every place of a 64-byte window, the last included
