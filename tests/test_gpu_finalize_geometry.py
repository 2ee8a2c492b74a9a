"""The batched finalize at piece edges (schedules and probes: tests/_finalgeom.py, proven on the oracle alone in
test_finalize_geometry_cpu.py). Every schedule runs on the device through three routes —

  batched   finalize_targets: all copies in one launch (k_copy_multi), all separators in one (k_set_bytes), the insertion
            beside the copies from their source (k_insert_multi<true>) and the edge runs behind them
  single    the same targets one by one through load_ref_dev, load_separator and release_lock: hipMemcpyAsync, k_insert,
            k_set_byte
  spec      emit_batch_begin_spec under a prediction that holds, so the gated launches run (one schedule per class; the
            verdicts themselves are test_gpu_spec_finalize.py's)

— and is held to the oracle's run of the same schedule after EVERY call: the whole reference buffer, the table image, the
loader's positions and counters, the next lock, the loaded-after array, and the rows of the single-sample probes at every
edge of the call (the table image shows positions; fingerprints and epochs show in those rows only). A failure names the
schedule, the call, the route, the edge and the probe's reference position."""
import time

import pytest

import _finalgeom as G
import _spec

pytestmark = pytest.mark.gpu
SCHEDULES = G.schedules()


@pytest.fixture(scope="module")
def device():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    return _spec.DeviceBackend(b)


def run(device, name, route):
    t0 = time.time()
    n_calls, n_probes, n_applied = G.hold_to_oracle(SCHEDULES[name], device, route)
    print("%s, route %s: %d calls, %d probes, %.2f s%s" % (name, route, n_calls, n_probes, time.time() - t0,
                                                           ", %d calls applied" % n_applied if route == "spec" else ""))
    return n_calls, n_probes, n_applied


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_the_batched_finalize_equals_the_oracle_after_every_call(device, name):
    run(device, name, "batched")


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_the_targets_one_by_one_equal_the_oracle_after_every_call(device, name):
    run(device, name, "single")


@pytest.mark.parametrize("name", G.SPEC_SCHEDULES)
def test_the_applied_speculative_finalize_equals_the_oracle_after_every_call(device, name):
    # (a call whose lazy separator has to overwrite the last loaded byte at the window's end cannot be queued behind a gate
    # and is declined: swsem_runtime_loader.h, load_separator. hold_to_oracle asserts that exactly those are, from the model.)
    n_calls, _, n_applied = run(device, name, "spec")
    assert n_applied > 0, "%s: no call was applied, the gated launches never ran" % name
