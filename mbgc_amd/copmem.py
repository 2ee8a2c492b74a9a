"""ctypes view of include/mbgc_copmem.h — the `-m3` reverse-complement pass over the literal stream
(SimpleSequenceMatcher::rcMatchSequence on CopMEMMatcher, matching/SimpleSequenceMatcher.cpp:165-176) and its inverse
(restoreRCMatchedSequence, :178-211)."""
import ctypes as C

import numpy as np

from . import binding

EXPORTS = """mbgc_copmem_create mbgc_copmem_destroy mbgc_copmem_last_error mbgc_copmem_rc_matches mbgc_copmem_rc_match_sequence
mbgc_copmem_rc_restore_plan mbgc_copmem_rc_restore_fill""".split()
DEFAULT = 0xFFFFFFFF
_ready = False


def _lib():
    global _ready
    L = binding.lib()
    if not _ready:
        u64, vp, u32, P = C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER
        L.mbgc_copmem_create.argtypes = [P(vp), C.c_int]
        L.mbgc_copmem_destroy.argtypes = [vp]
        L.mbgc_copmem_last_error.restype = C.c_char_p
        L.mbgc_copmem_rc_matches.argtypes = [vp, vp, u64, u32, u32, P(vp), P(u64), P(C.c_int)]
        L.mbgc_copmem_rc_match_sequence.argtypes = [vp, vp, u64, u32, u32, P(u64), P(vp), P(u64), P(vp), P(u64), P(u64)]
        L.mbgc_copmem_rc_restore_plan.argtypes = [vp, vp, u64, vp, u64, vp, u64, C.c_int, P(u64), P(u64), P(C.c_double)]
        L.mbgc_copmem_rc_restore_fill.argtypes = [vp, vp, u64, vp, P(C.c_double), P(u64)]
        _ready = True
    return L


class SimpleSequenceMatcher:
    """rcMatchSequence(sequence, rcMapOff, rcMapLen, targetMatchLength, minMatchLength) on the device."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        if _lib().mbgc_copmem_create(C.byref(self.h), device):
            raise binding.SwsemError(_lib().mbgc_copmem_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            _lib().mbgc_copmem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def rc_matches(self, seq, target=55, min_len=DEFAULT):
        """-> ((n, 3) uint64 rows in push order: posSrcText, length, posDestText in the reverse-complemented text; (K, k1, k2, log2 hash size))"""
        a = np.ascontiguousarray(seq, dtype=np.uint8)
        out, n = C.c_void_p(), C.c_uint64()
        params = (C.c_int * 4)()
        r = _lib().mbgc_copmem_rc_matches(self.h, a.ctypes.data_as(C.c_void_p), a.size, target, min_len, C.byref(out), C.byref(n), params)
        if r:
            raise binding.SwsemError("copmem error %d: %s" % (r, _lib().mbgc_copmem_last_error().decode()))
        rows = np.zeros((n.value, 3), dtype=np.uint64)
        if n.value:
            rows[:] = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(n.value, 3))
        return rows, tuple(params)

    def rc_match_sequence(self, seq, target=55, min_len=DEFAULT):
        """-> (rewritten sequence bytes, rcMapOff, rcMapLen, (unique matches, matched, overlapped))"""
        a = np.array(seq, dtype=np.uint8, copy=True)
        new_len, no, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        off, ln = C.c_void_p(), C.c_void_p()
        st = (C.c_uint64 * 3)()
        r = _lib().mbgc_copmem_rc_match_sequence(self.h, a.ctypes.data_as(C.c_void_p), a.size, target, min_len, C.byref(new_len),
                                                 C.byref(off), C.byref(no), C.byref(ln), C.byref(nl), st)
        if r:
            raise binding.SwsemError("copmem error %d: %s" % (r, _lib().mbgc_copmem_last_error().decode()))
        take = lambda p, k: bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(k,))) if k else b""
        return a[:new_len.value].tobytes(), take(off, no.value), take(ln, nl.value), tuple(st)

    def rc_restore_plan(self, cut, map_off, map_len, off_bytes=0):
        """uploads, plans and validates -> (restored length, (marks, bytes restored from matches, 0, minMatchLength), device ms);
        raises with the ABI's message on malformed maps (-4): nothing of them was used as an address"""
        a = np.ascontiguousarray(np.frombuffer(cut, dtype=np.uint8) if isinstance(cut, (bytes, bytearray)) else cut, dtype=np.uint8)
        mo, ml = bytes(map_off), bytes(map_len)
        org, ms = C.c_uint64(), C.c_double()
        st = (C.c_uint64 * 4)()
        r = _lib().mbgc_copmem_rc_restore_plan(self.h, a.ctypes.data_as(C.c_void_p), a.size, mo, len(mo), ml, len(ml), off_bytes,
                                               C.byref(org), st, C.byref(ms))
        if r:
            raise binding.SwsemError("copmem error %d: %s" % (r, _lib().mbgc_copmem_last_error().decode()))
        return org.value, tuple(st), ms.value

    def rc_restore_fill(self, org_len, cap=None, dst_dev=None):
        """the planned bytes -> (bytes, fill kernel ms, deepest chain); dst_dev: a device address of cap bytes to fill as well"""
        cap = org_len if cap is None else cap
        out = np.empty(max(cap, 1), dtype=np.uint8)
        ms, deep = C.c_double(), C.c_uint64()
        r = _lib().mbgc_copmem_rc_restore_fill(self.h, C.c_void_p(dst_dev), cap, out.ctypes.data_as(C.c_void_p), C.byref(ms), C.byref(deep))
        if r:
            raise binding.SwsemError("copmem error %d: %s" % (r, _lib().mbgc_copmem_last_error().decode()))
        return out[:org_len].tobytes(), ms.value, deep.value

    def rc_restore_sequence(self, cut, map_off, map_len, off_bytes=0):
        """restoreRCMatchedSequence -> (restored bytes, {"marks", "restored_from_matches", "max_chain", "min_match_length"})"""
        org, st, _ = self.rc_restore_plan(cut, map_off, map_len, off_bytes)
        data, _, deep = self.rc_restore_fill(org)
        return data, {"marks": st[0], "restored_from_matches": st[1], "max_chain": deep, "min_match_length": st[3]}


def rc_restore_sequence(cut, map_off, map_len, off_bytes=0, device=0):
    """one call on a handle of its own: see SimpleSequenceMatcher.rc_restore_sequence"""
    m = SimpleSequenceMatcher(device)
    try:
        return m.rc_restore_sequence(cut, map_off, map_len, off_bytes)
    finally:
        m.close()
