"""swsem_emit_batch_begin_spec against the plain finalize, at every verdict (scenarios and driver: tests/_spec.py; the
scenarios are proven on the CPU oracle in test_spec_contract_cpu.py). The device decides on its own whether the queued
copies, separators and table insertions run (k_spec_verify's word), the host comes to the same verdict a second time and
keeps or rolls back its bookkeeping: two handles run the same round, one through the plain calls and one through the
speculative one, and

  applied      the state after the call — the whole reference buffer, the hash-table image, the loader's positions, the
               next lock — is the plain finalize's, byte for byte, and so is loadedAfter
  not applied  the state after the call is the state before it, byte for byte, and the ordinary finalize that follows
               leaves the plain path's

with `applied` exactly the outcome of the prediction as Python integers work it out from the plain path's unmatchedChars.
Either way the six streams of every contig and a further round's match rows are the same on both handles, and the plain
handle's reference bytes and table equal the CPU oracle's for the same calls."""
import pytest

import _spec
from test_gpu_matcher import assert_same_state

pytestmark = pytest.mark.gpu
SCENARIOS = _spec.scenarios()


@pytest.fixture(scope="module")
def device():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    return _spec.DeviceBackend(b)


def run(device, name):
    scn = SCENARIOS[name]
    A = _spec.run_path(device, scn)
    decisions = [r.decision for r in A.rounds]
    B = _spec.run_path(device, scn, decisions)
    branches = _spec.check(scn, A, B)
    print("%s: %s" % (name, ", ".join(branches)))
    O = _spec.run_path(_spec.OracleBackend(), scn)
    for a, o in zip(A.rounds, O.rounds):
        assert a.un == o.un, name
    assert_same_state(A.m, O.m)
    assert A.probe_fp == O.probe_fp, name
    _spec.close(O)
    return scn, A, B, decisions, branches


@pytest.mark.parametrize("name", sorted(n for n in SCENARIOS if not n.startswith("k_")))
def test_speculative_finalize_keeps_its_contract(device, name):
    scn, A, B, _, branches = run(device, name)
    assert [b == "applied" for b in branches] == scn.want
    _spec.close(A, B)


@pytest.mark.parametrize("name", sorted(n for n in SCENARIOS if n.startswith("k_")))
def test_speculative_finalize_at_the_buffers_end(device, name):
    """the round's loads cross the end of the circular buffer, or stop exactly at it, with every target's lock held: the
    library may find that this finalize cannot be queued behind a gate and decline, so the verdict is not prescribed — only
    that whatever it reports is true, and that a second fresh handle given the same calls reports the same"""
    scn, A, B, decisions, branches = run(device, name)
    B2 = _spec.run_path(device, scn, decisions)
    assert [r.applied for r in B2.rounds] == [r.applied for r in B.rounds]
    _spec.check(scn, A, B2)
    print("%s took the branch: %s" % (name, ", ".join(branches)))
    _spec.close(A, B, B2)
