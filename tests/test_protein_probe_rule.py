"""The protein-profile probe, restated (tests/_probe.py), against what the reference CLI decided for the same inputs
(tests/golden/proteins/rule_cases.json, written by tests/golden/make_proteins_golden.py from `mbgc-dev c`'s stderr)."""
import json
import os

import pytest

import _probe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proteins")
RECORDED = json.load(open(os.path.join(GOLDEN, "rule_cases.json")))
CASES = _probe.rule_cases()


def test_every_case_is_recorded():
    assert set(CASES) == set(RECORDED)
    for name, (records, opts, _) in CASES.items():
        assert RECORDED[name]["options"] == opts and RECORDED[name]["record_lengths"] == [len(r) for r in records], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_decides_as_the_reference(name):
    records, opts, sequential = CASES[name]
    switched, _ = _probe.switches(records, sequential, k=_probe.case_k(opts), uppercase="-U" in opts)
    assert switched == RECORDED[name]["switched"]


def test_recorded_flags_are_the_ones_the_cases_are_named_for():
    want = dict(pct10_of_256=False, pct11_of_256=True, running_count_over_1500=True, running_count_over_2000=False,
                running_count_sequential=False, dna_65536_then_protein=False, straddle_clipped_divisor=True,
                straddle_clipped_count=False, lowercase_n_15pct=True, lowercase_n_15pct_U=False, protein_k16=False, protein_k24=True)
    assert {k: v["switched"] for k, v in RECORDED.items()} == want
    for kind in ("t1", "m3"):
        assert json.load(open(os.path.join(GOLDEN, "expected_%s.json" % kind)))["switched"] is True


def test_where_and_on_what_the_probe_fires():
    records = CASES["running_count_over_1500"][0]
    assert _probe.probe_records(records) == (True, 1, (0, 200))             # at record 1, on the running count of record 0
    assert _probe.probe_records(CASES["running_count_over_2000"][0]) == (False, 0, (65536 - 2200, 200))
    # the clip: 65000 + 536 bases are probed, whatever the second record's length
    assert _probe.probe_records(CASES["straddle_clipped_count"][0]) == (False, 0, (0, 0))
    assert _probe.probe_records(CASES["straddle_clipped_divisor"][0]) == (True, 1, (0, 60))


def test_empty_record_and_carried_state():
    """the one deviation: an empty record changes nothing (the reference divides by zero); and the state goes from call to call"""
    prot = CASES["protein_k24"][0][0]
    assert _probe.probe_records([b"", prot[:300]]) == _probe.probe_records([prot[:300]])[:1] + (1,) + _probe.probe_records([prot[:300]])[2:]
    f1, _, st = _probe.probe_records([prot[:200]])
    assert not f1 and st[0] == 65536 - 200
    assert _probe.probe_records([prot[200:300]], st)[:2] == (True, 0)
    assert _probe.probe_records([prot], (0, 7)) == (False, 0, (0, 7))       # spent: nothing more is probed
