"""bench.py's host-side helpers (no GPU): what the container grants, and that the bench refuses to run without a device
instead of measuring something else."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_quota_is_none_or_a_positive_number_of_cpus():
    sys.path.insert(0, ROOT)
    import bench
    q = bench.cpu_quota()
    assert q is None or (isinstance(q, float) and 0 < q <= 4096)


def test_without_a_device_the_bench_fails_loudly():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a device is present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--cpu-sample", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert all(l["value"] is None and l["error"] for l in lines)                # nothing was measured, and the line (if any) says so


# ---- `bench.py --gpus N` outside a launcher: the spawner must not hang on a rank that dies
_CHILD = """
import os, sys, time, signal
r = int(os.environ["RANK"]); n = int(os.environ["WORLD_SIZE"])
open(os.path.join(os.environ["MBGC_BENCH_RUNDIR"], "rank%d.up" % r), "w").close()
mode = sys.argv[1]
if mode == "ok":
    time.sleep(0.3)
    if r == 0: print('{"metric": "m", "value": 1.0, "n_gpus": %d}' % n, flush=True)
elif mode == "kill3":
    if r == 3:
        time.sleep(1.0); os.kill(os.getpid(), signal.SIGKILL)
    time.sleep(600)                       # the others sit "inside a collective"
elif mode == "stuck":
    time.sleep(600)
elif mode == "exit7":
    if r == 1: sys.exit(7)
    time.sleep(600)
"""


def _spawn(mode, n, limit=None, grace=1.0):
    code = ("import sys; sys.path.insert(0, %r); import bench; bench.spawn_ranks(%d, argv=[sys.executable, '-c', %r, %r], grace=%r, limit=%r)"
            % (ROOT, n, _CHILD, mode, grace, limit))
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    return r, time.monotonic() - t0


def test_spawner_relays_rank_0s_line():
    r, dt = _spawn("ok", 4)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["value"] == 1.0 and lines[0]["n_gpus"] == 4


def test_spawner_ends_the_run_when_a_rank_is_killed():
    """8 ranks, rank 3 dies on SIGKILL a second in, the others would wait ten minutes: the spawner returns within seconds,
    non-zero, with a line that says value null, which rank, and how many ranks had come up"""
    r, dt = _spawn("kill3", 8)
    assert r.returncode != 0 and dt < 30, (r.returncode, dt)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["value"] is None and "rank 3" in lines[0]["error"] and "signal 9" in lines[0]["error"]
    assert lines[0]["rccl_ranks_seen"] == 8 and lines[0]["n_gpus"] == 8


def test_spawner_ends_the_run_when_a_rank_exits_with_an_error():
    r, dt = _spawn("exit7", 2)
    assert r.returncode == 7 and dt < 30
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines[0]["value"] is None and "rank 1" in lines[0]["error"] and "exit code 7" in lines[0]["error"]


def test_spawner_bounds_the_whole_run():
    r, dt = _spawn("stuck", 2, limit=2.0)
    assert r.returncode != 0 and dt < 30
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines[0]["value"] is None and "limit" in lines[0]["error"]


# ---- the lines bench.py adds beside the headline are put together from other programs' output: their format strings and regular
# expressions are exercised here with stand-ins for those programs (a percent sign in one of them cost a round-4 run its configs[1] line)
def _fake_tool(tmp_path, stdout, stderr):
    p = tmp_path / "fake-tool"
    p.write_text("#!/bin/sh\ncat <<'EOF_OUT'\n%s\nEOF_OUT\ncat >&2 <<'EOF_ERR'\n%s\nEOF_ERR\n" % (stdout, stderr))
    p.chmod(0o755)
    return str(p)


def test_the_lines_beside_the_headline_are_put_together(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    prof = ('kernel profile: {"load": {"ms": 7.0, "launches": 500}, "insert": {"ms": 12.0, "launches": 500}, "probe": {"ms": 0.0, "launches": 0}, '
            '"emit2": {"ms": 230.0, "launches": 500}, "resolve": {"ms": 140.0, "launches": 500}, "stitch": {"ms": 90.0, "launches": 500}, "emit": {"ms": 13.0, "launches": 500}}')
    out = "rounds of 28 targets; reference extension bytes dropped at the sliding window's end: 0\nfinal reference length: 1809744201\nexact matches total: 6954058\nswsMEM unmatched chars: 381336073\nfinal unmatched chars: 1"
    monkeypatch.setattr(bench, "TOOL", _fake_tool(tmp_path, out, "matching finished - 432 [ms]\n" + prof))
    (tmp_path / "meta.json").write_text(json.dumps({"genomes": 200, "bases": 909_000_000, "g0_bases": 5_000_000}))
    (tmp_path / "list.txt").write_text("")
    for rounds in (False, True):
        line = bench.config4_line(str(tmp_path), rounds=rounds)
        assert "error" not in line, line
        assert line["value"] == round(904_000_000 / 0.432 / 1e9, 4) and line["roofline"]["kernel"] == "k_resolve_blocks4"
        assert ("rounds of 28" in line["workload"]) == rounds and ("0.2-10 % divergence" in line["workload"]) != rounds
    # configs[1]: a child bench.py whose last line is the diagnostic line of `--no-emit`
    child = {"metric": "m", "value": 56.4, "unit": "Gbases/s", "ms_per_step": 1.4, "extension_bytes_dropped_per_step": 0.0,
             "config": {"max_ref_len": 1_280_000_000, "targets_per_step": 16}, "roofline": {"frac": 0.036}, "kernel_ms_per_launch": {"resolve": 0.92}}

    class R:
        returncode = 0
        stdout = json.dumps(child) + "\n"
        stderr = ""
    monkeypatch.setattr(bench.subprocess, "run", lambda *a, **k: R())
    line = bench.config1_line()
    assert "error" not in line, line
    assert line["value"] == 56.4 and "99% identity" in line["workload"] and "1.28e+09-byte" in line["workload"]


# ---- --dump-outputs: what the last timed step gave its caller, written from a stand-in for the handle's last emission
def test_dump_outputs_writes_the_last_steps_streams(tmp_path, monkeypatch):
    import ctypes
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from mbgc_amd import binding
    rng = np.random.default_rng(5)
    n = 3
    sizes = rng.integers(0, 400, (n, 6)).astype(np.uint64)
    sizes[1, 0] = 3000                                   # one stream longer than the cap below: sampled
    sizes[:, 2] = 0                                      # one stream empty in every contig (mapOff5th without 40-bit offsets): no file
    packed = rng.integers(0, 256, int(sizes.sum())).astype(np.uint8)
    counters = np.arange(n * 6, dtype=np.uint64)

    class FakeMatcher:
        h = None

        def emit_pack_sizes(self, k):
            assert k == n
            return sizes.copy(), int(sizes.sum())

        def emit_pack_dev(self, ptr, cap):
            assert cap >= packed.size
            ctypes.memmove(ptr, packed.ctypes.data, packed.size)
            return packed.size

    class FakeLib:
        @staticmethod
        def swsem_emit_counters(h, out):
            ctypes.memmove(out, counters.ctypes.data, counters.nbytes)
            return 0
    monkeypatch.setattr(binding, "lib", lambda: FakeLib)
    monkeypatch.setattr(bench, "DUMP_STREAM_CAP", 1000)
    d = tmp_path / "out"
    bench.dump_outputs(str(d), FakeMatcher(), np.array([7, 8, 9], dtype=np.uint64), True, "cpu")
    got = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))}
    assert set(got) == {"match_counts", "emit_counters", "stream_sizes", "stream_fingerprints"} | (set(binding.STREAM_NAMES) - {binding.STREAM_NAMES[2]})
    assert all(a.dtype in (np.float32, np.float64) and a.size for a in got.values())
    assert got["match_counts"].tolist() == [7, 8, 9] and got["emit_counters"].tolist() == counters.reshape(n, 6).tolist()
    assert np.array_equal(got["stream_sizes"], sizes.astype(np.float64))
    starts = np.concatenate([[0], np.cumsum(sizes.reshape(-1).astype(np.int64))])
    for st, name in enumerate(binding.STREAM_NAMES):
        whole = np.concatenate([packed[starts[k * 6 + st]: starts[k * 6 + st + 1]] for k in range(n)])
        if not whole.size:
            assert name not in got
        elif whole.size <= 1000:
            assert np.array_equal(got[name], whole.astype(np.float32)), name
        else:                                            # a fixed sample, the same in every run
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(whole.size, 1000, replace=False))
            assert np.array_equal(got[name], whole[idx].astype(np.float32)), name
        for k in range(n):
            seg = packed[starts[k * 6 + st]: starts[k * 6 + st + 1]].astype(np.int64)
            assert got["stream_fingerprints"][k, st, 0] == seg.sum()
            assert got["stream_fingerprints"][k, st, 1] == (seg * (np.arange(seg.size) + 1)).sum()


def test_a_plain_run_leaves_the_extras_to_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
