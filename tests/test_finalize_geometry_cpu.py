"""The finalize-geometry schedules (tests/_finalgeom.py) on the CPU oracle alone: every schedule is what it says it is (from
the loader's getters), the probes hang on one sample each, every edge kind of every schedule has a probe the oracle answers
with a row of exactly L bytes, 80 % of the probes cut from random text have a row, and the lists of lengths, alignments, call
shapes and ends the schedules were written for are all hit. Where the reference itself has been built (oracle/_ref), one
schedule of each end class is held to it as well."""
import functools

import numpy as np
import pytest

import _finalgeom as G
import _orc_backend
import _refh
import _spec

SCHEDULES = G.schedules()
RANDOM_ROW_SHARE = 0.80


@functools.lru_cache(maxsize=None)
def facts(name):
    """one oracle run of the schedule -> what was seen (per-call models, probe statistics)"""
    sched = SCHEDULES[name]
    f = dict(wrapped=False, clipped=0, at_sw_end=False, off_then_on=False, short_piece=False, laps=0, tags=set(),
             kinds={}, covered=0, probes=0, rows=0, grid_probes=0, grid_rows=0, offgrid_probes=0, offgrid_rows=0, dst=set(), src=set())
    off, on_again = False, False
    for rec in G.OracleRun(sched):
        md, call, K, o = rec["model"], rec["call"], rec["K"], rec["m"]
        f["wrapped"] |= md["wrapped"]
        f["clipped"] += rec["post"]["dropped"] - rec["pre"]["dropped"]
        f["at_sw_end"] |= md["at_sw_end"] and rec["post"]["pos"] == rec["pre"]["sw_end"]
        off |= rec["post"]["sp"] % G.K1 != 0 or bool(md["offgrid"])
        on_again |= off and rec["post"]["sp"] % G.K1 == 0
        f["short_piece"] |= any(hi - lo < K for lo, hi, _ in md["pieces"])
        f["laps"] = rec["post"]["laps"]
        f["tags"] |= call.tags
        f["covered"] += len(md["covered"])
        assert K == G.K_L32
        for kind, _ in rec["edges"]:
            f["kinds"].setdefault(kind, False)
        for lo, hi, t in md["pieces"]:
            f["dst"].add((lo % 16, lo % 4096))
            f["src"].add(call.targets[t][0] % 16)
        for p in rec["probes"]:
            inside = [s for s in range(p.at, p.at + G.L - K + 1) if s % G.K1 == 0]        # grid samples whose K-mer lies inside the probe
            assert p.at <= p.s <= p.at + G.L - K and inside == ([] if p.offgrid else [p.s]), (name, rec["ci"], p)
        for lock in (None, G.next_lock(o)):
            rows = G.match_probes(_spec.OracleBackend(), o, rec["probes"], lock)
            for p, r in zip(rec["probes"], rows):
                hit = G.has_exact_row(r, p)
                if not p.sampled:
                    assert not hit, (name, rec["ci"], p)
                    continue
                f["probes"] += 1
                f["rows"] += hit
                f["offgrid_probes" if p.offgrid else "grid_probes"] += 1
                f["offgrid_rows" if p.offgrid else "grid_rows"] += hit
                f["kinds"][p.kind] = f["kinds"].get(p.kind, False) or hit
    f["off_then_on"] = on_again
    return f


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_a_schedule_is_what_it_says(name):
    sched, f = SCHEDULES[name], facts(name)
    c = sched.claims
    if c.get("wrap"):
        assert f["wrapped"] and f["laps"] >= 1
    if "clipped" in c:
        assert f["clipped"] == c["clipped"] > 0
    else:
        assert f["clipped"] == 0
    if c.get("at_sw_end"):
        assert f["at_sw_end"]
    if c.get("offgrid_and_back"):
        assert f["off_then_on"]
    if c.get("short_piece"):
        assert f["short_piece"]
    if "covered" in c:
        # samples inside a piece whose K-mer holds that piece's separator: what the trimming in prepare_inserts is for
        assert f["covered"] == c["covered"] > 0
    if "laps" in c:
        assert f["laps"] == c["laps"]
    assert f["probes"] > 0
    # every edge kind the schedule has: at least one probe the oracle answers with a row of exactly L bytes
    missing = [k for k, hit in f["kinds"].items() if not hit]
    print("%s: %d probes, %d with a row; on the grid %d / %d, off it %d / %d; edge kinds %r" % (
        name, f["probes"], f["rows"], f["grid_rows"], f["grid_probes"], f["offgrid_rows"], f["offgrid_probes"], sorted(f["kinds"])))
    assert not missing, "%s: no probe with a row of exactly L at the edge kinds %r" % (name, missing)


def test_most_probes_of_random_text_have_a_row():
    tot = rows = 0
    for name, s in SCHEDULES.items():
        if not s.lowc:
            tot += facts(name)["probes"]
            rows += facts(name)["rows"]
    print("random text: %d of %d probes have a row (%.3f)" % (rows, tot, rows / tot))
    assert rows >= RANDOM_ROW_SHARE * tot


def test_a_sample_off_the_grid_has_rows_in_low_complexity_only():
    rnd = sum(facts(n)["offgrid_rows"] for n, s in SCHEDULES.items() if not s.lowc)
    low = sum(facts(n)["offgrid_rows"] for n, s in SCHEDULES.items() if s.lowc)
    assert sum(facts(n)["offgrid_probes"] for n in SCHEDULES) > 0
    assert low > 0, "no probe of a sample off the grid has a row in the low-complexity schedules"
    print("probes of samples off the grid with a row: random text %d, low complexity %d" % (rnd, low))


def test_the_coverage_table_has_no_empty_class():
    K = G.K_L32
    want = ["alone:%d" % n for n in G.lengths(K)] + ["middle:%d" % n for n in G.lengths(K)]
    want += ["src:%d" % r for r in G.SRC_RES] + ["dst:%d/%d" % (r, m) for m, r in G.DST_RES]
    want += ["n:%d" % n for n in (1, 2, 5, 40)] + ["zero:first", "zero:middle", "zero:last", "lazy:0", "lazy:1", "add_sep:0", "add_sep:1", "sep:0", "sep:nz"]
    want += ["wend:-1", "wend:+0", "wend:+1", "wend:held", "wend:released", "wend:full_later", "sep_inside", "sep_over_last_byte", "epoch_decides", "sep_inside_last_step"]
    want += ["bend:exact", "bend:short_after", "bend:straddle", "bend:back_on_grid", "laps", "overlap"]
    for lowc in (False, True):
        table = {w: [n for n, s in SCHEDULES.items() if s.lowc == lowc and w in facts(n)["tags"]] for w in want}
        empty = [w for w, v in table.items() if not v]
        assert not empty, "no %s schedule hits %r" % ("low-complexity" if lowc else "random-text", empty)
        # the residues, from where the pieces really went
        dst = set().union(*[facts(n)["dst"] for n, s in SCHEDULES.items() if s.lowc == lowc])
        src = set().union(*[facts(n)["src"] for n, s in SCHEDULES.items() if s.lowc == lowc])
        assert {0, 1, 15} <= {a for a, _ in dst} and {0, 4095} <= {b for _, b in dst} and set(G.SRC_RES) <= src
    assert {s.cls for s in SCHEDULES.values()} >= {"alone", "window_end", "buffer_end", "overlap"}
    assert set(G.SPEC_SCHEDULES) <= set(SCHEDULES)


# ---- the reference itself, where it has been built
class _RefShim:
    def __init__(self, r):
        self.r = r

    def __getattr__(self, name):
        return getattr(self.r, name)

    def release_lock(self, v):
        self.r.release_lock(v)
        return 0


class RefDeviceMatcher(_orc_backend.OracleDeviceMatcher):
    def __init__(self, max_ref_len):
        self.o = _RefShim(_refh.RefMatcher(max_ref_len))
        self._contigs, self._locks, self._matches, self._em, self._em_prev, self._sel_prev = [], [], [], [], [], False


class RefBackend(_spec.OracleBackend):
    name = "reference"

    def make(self, max_ref):
        return RefDeviceMatcher(max_ref)


@pytest.mark.skipif(not _refh.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", ["window_end", "buffer_end", "buffer_end_lowc", "three_laps_lowc"])
def test_an_end_schedule_against_the_reference_itself(name):
    n_calls, n_probes, _ = G.hold_to_oracle(SCHEDULES[name], RefBackend(), "batched")
    assert n_calls == len(SCHEDULES[name].calls) and n_probes > 0
