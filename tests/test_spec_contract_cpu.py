"""The speculative finalize's scenarios (tests/_spec.py) on the CPU oracle behind the device surface: every scenario is
what it claims to be — the "equality" contig really has un * factor == len, the given-up contig really returns 2^64 - 1,
the wrap really crosses the buffer's end — and comes to the verdict it is built for, before a GPU is held to it
(test_gpu_spec_finalize.py). The stand-in's emit_batch_begin_spec states the contract; check() holds it to it."""
import pytest

import _spec

SCENARIOS = _spec.scenarios()


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_is_what_it_claims(name):
    scn = SCENARIOS[name]
    backend = _spec.OracleBackend()
    A = _spec.run_path(backend, scn)
    B = _spec.run_path(backend, scn, [r.decision for r in A.rounds])
    for r, rec in enumerate(A.rounds):
        print("%s round %d: unmatched %r of %r, factors %d / %d" % (name, r, rec.un[:8], scn.rounds[r].lens[:8], rec.decision.factor, rec.decision.rc_factor))
    scn.facts(A, scn)
    branches = _spec.check(scn, A, B)
    print("%s: %s" % (name, ", ".join(branches)))
    for r, want in enumerate(scn.want):
        if want is not None:
            assert (branches[r] == "applied") == want
    _spec.close(A, B)
