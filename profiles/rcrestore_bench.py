"""The inverse of the `-m3` reverse-complement pass against the forward pass, on the stream size of r02_rcmatch_bench.json: 256 MB
of literal-like stream (tests/_rcdata.literal_like) with 2.5 % of it planted as reverse-complement copies. Both directions are
timed at the C ABI (include/mbgc_copmem.h) from and to host memory: one warm-up call, then the median of RUNS calls.

    python profiles/rcrestore_bench.py [megabytes] [out.json] [libcopmem built with -DMBGC_RC_RESTORE_BYTEWISE]

The optional third argument times the fill kernel of a second build whose lanes never take the 16-byte path."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rcdata  # noqa: E402
from mbgc_amd import copmem  # noqa: E402

RUNS = 5


def declare(L):
    u64, vp, u32, P = C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER
    L.mbgc_copmem_create.argtypes = [P(vp), C.c_int]
    L.mbgc_copmem_destroy.argtypes = [vp]
    L.mbgc_copmem_last_error.restype = C.c_char_p
    L.mbgc_copmem_rc_restore_plan.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.c_int, P(u64), P(u64), P(C.c_double)]
    L.mbgc_copmem_rc_restore_fill.argtypes = [vp, vp, u64, vp, P(C.c_double), P(u64)]
    return L


def restore_runs(L, h, cut, map_off, map_len, out):
    rows = []
    for _ in range(RUNS + 1):
        org, pms, fms, deep = C.c_uint64(), C.c_double(), C.c_double(), C.c_uint64()
        st = (C.c_uint64 * 4)()
        t0 = time.perf_counter()
        r = L.mbgc_copmem_rc_restore_plan(h, cut.ctypes.data_as(C.c_void_p), cut.size, map_off, len(map_off), map_len, len(map_len), 0, C.byref(org), st, C.byref(pms))
        assert r == 0, L.mbgc_copmem_last_error()
        t1 = time.perf_counter()
        r = L.mbgc_copmem_rc_restore_fill(h, None, out.size, out.ctypes.data_as(C.c_void_p), C.byref(fms), C.byref(deep))
        assert r == 0, L.mbgc_copmem_last_error()
        t2 = time.perf_counter()
        rows.append({"whole_ms": (t2 - t0) * 1e3, "plan_call_ms": (t1 - t0) * 1e3, "fill_call_ms": (t2 - t1) * 1e3, "plan_device_ms": pms.value,
                     "fill_kernel_ms": fms.value, "deepest_chain": deep.value, "marks": st[0], "restored_from_matches": st[1], "restored_bytes": org.value})
    return rows[1:]


def med(rows, k):
    return round(statistics.median(r[k] for r in rows), 3)


def main():
    mb = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    n = mb * 1_000_000
    copies = max(1, int(n * 0.025 / 5000))                                   # lengths are uniform in [40, 10000): 2.5 % of the stream
    s = _rcdata.literal_like(n, 1, copies=copies, longest=10_000)
    s[(s == 0xA4) | (s == 127)] = ord("A")
    L = declare(copmem._lib())
    m = copmem.SimpleSequenceMatcher()
    fwd = []
    cut = map_off = map_len = None
    for _ in range(RUNS + 1):
        a = s.copy()
        new_len, no, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        off, ln = C.c_void_p(), C.c_void_p()
        st = (C.c_uint64 * 3)()
        t0 = time.perf_counter()
        r = L.mbgc_copmem_rc_match_sequence(m.h, a.ctypes.data_as(C.c_void_p), a.size, 55, 0xFFFFFFFF, C.byref(new_len), C.byref(off), C.byref(no), C.byref(ln), C.byref(nl), st)
        fwd.append((time.perf_counter() - t0) * 1e3)
        assert r == 0
        cut = a[:new_len.value].copy()
        map_off, map_len = C.string_at(off, no.value), C.string_at(ln, nl.value)
    fwd = fwd[1:]
    out = np.empty(n, dtype=np.uint8)
    rows = restore_runs(L, m.h, cut, map_off, map_len, out)
    identical = bool(np.array_equal(out, s))
    whole = med(rows, "whole_ms")
    res = {"sequence_bytes": n, "planted_copies": copies, "cut_bytes": int(cut.size), "marks": rows[0]["marks"], "restored_from_matches": rows[0]["restored_from_matches"],
           "deepest_chain": max(r["deepest_chain"] for r in rows), "runs": RUNS,
           "forward_rcMatchSequence_ms": round(statistics.median(fwd), 3), "forward_ms_min_max": [round(min(fwd), 3), round(max(fwd), 3)],
           "restore_whole_ms": whole, "restore_whole_ms_min_max": [round(min(r["whole_ms"] for r in rows), 3), round(max(r["whole_ms"] for r in rows), 3)],
           "restore_plan_call_ms": med(rows, "plan_call_ms"), "restore_fill_call_ms": med(rows, "fill_call_ms"), "restore_plan_device_ms": med(rows, "plan_device_ms"),
           "restore_fill_kernel_ms": med(rows, "fill_kernel_ms"), "restore_GB_per_s_whole": round(n / (whole * 1e-3) / 1e9, 3),
           "restore_GB_per_s_fill_kernel": round(n / (med(rows, "fill_kernel_ms") * 1e-3) / 1e9, 1), "identical_to_input": identical,
           "note": "both directions from and to pageable host memory through the C ABI; plan_call = upload of the cut stream and the maps + the plan's kernels, "
                   "fill_call = the fill kernel + the download of the restored stream"}
    if len(sys.argv) > 3:
        B = declare(C.CDLL(sys.argv[3]))
        h = C.c_void_p()
        assert B.mbgc_copmem_create(C.byref(h), 0) == 0
        out2 = np.empty(n, dtype=np.uint8)
        brows = restore_runs(B, h, cut, map_off, map_len, out2)
        res["bytewise_build_fill_kernel_ms"] = med(brows, "fill_kernel_ms")
        res["bytewise_build_identical"] = bool(np.array_equal(out2, s))
        B.mbgc_copmem_destroy(h)
    m.close()
    line = json.dumps(res, indent=1)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
    assert identical


if __name__ == "__main__":
    main()
