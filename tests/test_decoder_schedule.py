"""The decoder's load schedule (MBGC_Decoder::scheduleTarget / loadRef, mbgc_amd/host/mbgc_decoder.cpp) against a straight
transcription of the reference's MBGC_Decoder::loadRef and decodeTarget's load calls (mbgccoder/MBGC_Decoder.cpp:651-675,
:564-620), which moves real bytes; and <prefix>.meta written and parsed back. No device."""
import ctypes as C
import os

import numpy as np
import pytest

import _meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP, FROM_REF = -1, -2
COMP = {ord(a): ord(b) for a, b in zip("ACGTN", "TGCAN")}


def host():
    L = C.CDLL(os.path.join(ROOT, "mbgc_amd", "libmbgc_host.so"))
    P = C.POINTER(C.c_uint64)
    L.mbgc_decoder_schedule.argtypes = [P, P, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, P, P, C.c_int, C.c_int,
                                        C.POINTER(C.c_int64), C.c_uint64, P]
    L.mbgc_meta_roundtrip.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, P, C.c_char_p, C.c_uint64]
    return L


class RefDecoder:
    """the transcription: refStr, refPos, reachedRefLengthCount as the reference keeps them"""

    def __init__(self, total, lazy, ref_pos, ref):
        self.total, self.lazy, self.pos, self.laps = total, lazy, ref_pos, 0
        self.ref = ref

    def load_ref(self, text, lock, rc):                       # :651-675
        seq_len = len(text)
        at = 0
        while seq_len:
            if self.pos == self.total and lock != self.total:
                self.laps += 1
                self.pos = 1
            tmp = seq_len
            tmp_max = self.total if lock < self.pos else lock
            if self.pos + tmp > tmp_max:
                tmp = tmp_max - self.pos
            if rc:
                src = text[at + seq_len - tmp: at + seq_len]
                self.ref[self.pos: self.pos + tmp] = [COMP[c] for c in src[::-1]]
            else:
                self.ref[self.pos: self.pos + tmp] = text[at: at + tmp]
            self.pos += tmp
            at += 0 if rc else tmp
            seq_len = 0 if self.pos == lock else seq_len - tmp
            if self.lazy and self.pos == lock:
                self.ref[lock - 1] = 0

    def decode_target(self, contigs, unmatched, factor, rc_factor, rc_in_ref, individually, lock):   # :564-620
        start = self.pos
        for c, un in zip(contigs, unmatched):
            ext = c if un * factor > len(c) else c[:0]
            self.load_ref(ext, lock, False)
            if rc_in_ref and individually and un * rc_factor > len(c):
                self.load_ref(ext, lock, True)
        if rc_in_ref and not individually:
            if self.pos >= start:
                self.load_ref(bytes(self.ref[start: self.pos]), lock, True)
            else:
                self.load_ref(bytes(self.ref[1: self.pos]), lock, True)
                self.load_ref(bytes(self.ref[start: self.total]), lock, True)
        if self.lazy:
            self.load_ref(b"\0", lock, False)


def run_case(total, ref_pos, lock, lens, unmatched, lazy, factor=128, rc_factor=8, rc_in_ref=True, individually=True, seed=3):
    rng = np.random.default_rng(seed)
    contigs = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for n in lens]
    start = bytearray(bytes(np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, total + 8)]))   # (what was there before: lower case)
    want = RefDecoder(total, lazy, ref_pos, bytearray(start))
    want.decode_target(contigs, unmatched, factor, rc_factor, rc_in_ref, individually, lock)
    pos, laps, nsegs = C.c_uint64(ref_pos), C.c_uint64(0), C.c_uint64()
    segs = np.zeros((256, 5), dtype=np.int64)
    ln, un = np.asarray(lens, dtype=np.uint64), np.asarray(unmatched, dtype=np.uint64)
    P = C.POINTER(C.c_uint64)
    rc = host().mbgc_decoder_schedule(C.byref(pos), C.byref(laps), total, int(lazy), int(rc_in_ref), int(individually), lock, 10, len(lens),
                                      ln.ctypes.data_as(P), un.ctypes.data_as(P), factor, rc_factor, segs.ctypes.data_as(C.POINTER(C.c_int64)), 256,
                                      C.byref(nsegs))
    assert rc == 0
    got = bytearray(start)
    for contig, off, length, ref_at, is_rc in segs[: nsegs.value].tolist():
        assert 1 <= ref_at and ref_at + length <= total                               # never outside the buffer
        if contig == SEP:
            assert length == 1
            got[ref_at] = 0
            continue
        text = bytes(got) if contig == FROM_REF else contigs[contig - 10]
        src = text[off: off + length]
        assert len(src) == length
        got[ref_at: ref_at + length] = bytes(COMP[c] for c in src[::-1]) if is_rc else src
    assert bytes(got) == bytes(want.ref)
    assert (pos.value, laps.value) == (want.pos, want.laps)
    return segs[: nsegs.value], want


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("individually", [True, False])
def test_no_wrap(lazy, individually):
    segs, w = run_case(5000, 700, 5000, [300, 41, 500], [300, 0, 100], lazy, individually=individually)
    assert w.laps == 0 and w.pos > 700


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("individually", [True, False])
def test_wrap_to_ref_shift(lazy, individually):
    """the loads reach the buffer's end, the lock lies in front of the loading position: the rest goes on at REF_SHIFT"""
    segs, w = run_case(3000, 2500, 1800, [400, 350], [400, 350], lazy, individually=individually)
    assert w.laps == 1 and 1 < w.pos < 1800
    assert any(r[3] == 1 for r in segs.tolist())                                        # a segment that starts at REF_SHIFT


@pytest.mark.parametrize("lazy", [True, False])
@pytest.mark.parametrize("individually", [True, False])
def test_load_cut_at_the_lock(lazy, individually):
    """the lock lies behind the loading position and the loads reach it: cut there, the rest dropped, the separator at lock - 1"""
    segs, w = run_case(4000, 1000, 1500, [300, 300, 200], [300, 300, 200], lazy, individually=individually)
    assert w.pos == 1500 and w.laps == 0
    assert (SEP in [r[0] for r in segs.tolist()]) == lazy
    if lazy:
        assert w.ref[1499] == 0


def test_reverse_complement_cut_takes_the_texts_tail():
    """:665: a cut reverse-complement load takes the LAST tmpLength bytes of the text"""
    segs, w = run_case(4000, 1000, 1450, [300], [300], False)
    rows = segs.tolist()
    assert rows[0][:3] == [10, 0, 300] and rows[1] == [10, 150, 150, 1300, 1]


def test_wrap_twice_and_end_exactly_on_the_buffers_end():
    run_case(1200, 1100, 0, [500, 500, 500], [500, 500, 500], True, rc_factor=0)
    run_case(2000, 1700, 0, [300], [300], False, rc_factor=0)                            # ends at refTotalLength: the wrap waits for the next load


def test_contigs_that_load_nothing():
    segs, w = run_case(5000, 700, 5000, [300, 20], [1, 0], False)
    assert len(segs) == 0 and w.pos == 700


def sample_meta(index=True):
    return dict(version=1, mode=2, k=32, k1=15, g0_contigs=3, max_ref_length=1 << 33, sw_size=(1 << 33) // 16, final_ref_length=123456789012,
                laps=2, emit=[1, 1, 0, 1, 1, 64, 2, 256, 50, 50, 500, 125, 0, 1024, 2], targets=[(2, 128, 128), (0, 0, 8), (70000, 255, 1)],
                index=[[10, 0, 0, 0, 0, 0], [500, 40, 10, 20, 9, 77], [500, 40, 10, 20, 9, 78], [1 << 35, 44, 11, 26, 9, 1 << 34]] if index else [],
                sequential=False, rc_in_reference=True, contigs_individually_reversed=True, uppercase=True, single_fasta=False, rc_redundancy_removal=False)


@pytest.mark.parametrize("index", [True, False])
def test_meta_written_and_parsed_back_identically(index):
    m = sample_meta(index)
    b = _meta.build(m)
    assert _meta.parse(b) == m
    out, n, err = C.create_string_buffer(len(b) + 64), C.c_uint64(), C.create_string_buffer(256)
    assert host().mbgc_meta_roundtrip(b, len(b), out, len(b) + 64, C.byref(n), err, 256) == 0
    assert out.raw[: n.value] == b


@pytest.mark.parametrize("cut", [0, 7, 12, 40, 100, 190, 200, -1, "extra", "magic"])
def test_meta_malformed_is_refused(cut):
    b = _meta.build(sample_meta())
    bad = b + b"\0" if cut == "extra" else (b"X" + b[1:] if cut == "magic" else b[:cut])
    out, n, err = C.create_string_buffer(len(b) + 64), C.c_uint64(), C.create_string_buffer(256)
    assert host().mbgc_meta_roundtrip(bad, len(bad), out, len(b) + 64, C.byref(n), err, 256) == -1
    assert err.value.startswith(b"malformed .meta")
