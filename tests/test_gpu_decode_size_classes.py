"""The device decoder (k_decode_plan / k_decode_fill, mbgc_amd/csrc/swsem_decode.hip) on the corpus of tests/_decsizes.py, which
sits on every edge at which the fill picks code by a size (DEC_WIDE_MIN = 192 for a run of plain literals, for the match copy and
for the right extension across a gap; the wave copy's 16-byte vectors, byte tail and rounds of 1 024 bytes; record indices at the
edges of a wave and of a block; a wave whose 64 lanes all carry wide work) and at which the plan's register windows end (a mark or a
set flag at every place of a 64-byte window, a mapLen escape across the end of the 256-byte dword window).
tests/test_decode_size_classes_cpu.py shows on the oracle alone that the corpus is what it says.

Family A (streams written by hand, extensions off) is held to a numpy expectation that no decoder had a part in; family B (gap
contigs, streams written by the oracle's encoder) to the contig itself. All contigs of a parameter set are jobs of one
swsem_decode_contigs_dev call — record counts from 1 to 1 201 side by side, the grid sized by the largest. The streams lie in one
blob with 0xEE between them, every destination has 64 guard bytes in front and behind and destCap = destLen + 16. Per job destLen,
unmatchedChars and the bytes (the first differing byte named) are the expectation's, guard and spare bytes untouched. Family A runs
again with every stream pointer and every destination moved by 1, 5 and 15 bytes. Family B is also matched and emitted on the
device and verified there (swsem_emit_verify), which then has to name the contig and the byte of a change inside a wide gap extension.

Which path ran is not observed on the device: it follows from the restated rules the CPU test pins to the sources.

Shown by experiment (one device run each, swsem_decode.hip broken by hand in a scratch copy, every break leaving bytes unwritten or
wrong only, none committed) — the tests of this file that fail:
  the wave copy without its byte tail            all 18: every family A set (first plain_dense_fwd, the run of 193 bytes) and, through
                                                 the wide match copies of the pieces (200 bytes), every family B case
  r.len <= DEC_WIDE_MIN turned into <, the wave's
  copy taking lengths above it only              the 12 family A cases (match_dense_*, the match of 192 bases) and the 3 emission cases; the
                                                 3 oracle-written family B cases pass (no match of 192 bases in them)
  `rank` of the wideRight loop not advanced      the 6 family B cases (oracle-written and device-emitted); family A passes (no flags)
  s0 ignored                                     the same 6
  dw_get reloading at >= in place of >           none, and none can: the window is loaded one byte early, the program computes the same
  dw_get reloading one byte late (> ... + 1)     the 12 family A cases, at `pairs` (a gapDelta read behind the window's end; without `pairs`,
                                                 whose gapDelta bytes differ from window to window, nothing failed: mapLen and mapOff
                                                 reads keep an even distance to the window's base and never end one byte behind it)
  plan_find_mark stepping from = base + WAVE + 1 all 18 (a mark at a window's first byte is missed)
  plan_find_mark stepping from = base + WAVE - 1 not run: a window without a mark is then looked at again for ever, the wave never ends —
                                                 a hang, which no run on a shared machine may provoke; the step is quoted by the CPU test
What a missed write leaves is the 0xEE the destination was filled with, never the right byte.

Not covered here: the 8-byte mapLen escape (lengths from 2^32 - 1 on); mapOff5th bytes other than 0 (the reference is far below
2^32 bytes, so a fifth byte read from the wrong place is not seen; its window is dw_get's, as gapDelta's); left extensions and right extensions outside a gap, which
stay with their thread at any length (tests/test_gpu_decode.py, tests/test_gpu_decode_mutants.py); REC_GAP_MIDDLE, which no encoder
writes at gapDepthMismatchesEncoding = 2; the collection-level chain (k_decode_plan_chain, tests/test_gpu_decode_chain.py) and
d --region's masked fill (tests/test_gpu_decode_region_sweep.py), which share plan_contig and decode_fill_body with what runs here.

Wall times on one MI355X, observed, not asserted: the module's 18 cases 2.5 s, of that 2 s the first use of the device;
every case at most 0.1 s."""
import numpy as np
import pytest

import _decsizes as D
import _emitsizes as E
import _orc

pytestmark = pytest.mark.gpu
GUARD, FILL, SPARE = 64, 0xEE, 16


@pytest.fixture(scope="module")
def binding():
    from mbgc_amd import binding as b
    assert b.lib().swsem_device_count() > 0
    return b


@pytest.fixture(scope="module")
def handle(binding):
    h = binding.SlidingWindowSparseEMMatcher(D.REF_MAX)
    h.load_ref(E.reference(), load_rc=False)
    assert np.array_equal(h.ref(D.REF_LEN + 64), D.ref_buffer()[:D.REF_LEN + 64])
    yield h
    h.close()


def decode_jobs(h, p, cases, shift=0):
    """cases: (label, six streams, expected bytes, expected unmatchedChars). One swsem_decode_contigs_dev call; -> what is wrong, per job"""
    import torch
    parts, at, where = [], 0, []

    def pad_to(n):                                                         # at least 16 bytes of FILL, then up to address = shift (mod 16)
        return 16 + (shift - (n + 16)) % 16

    parts.append(bytes([FILL]) * (16 + shift))
    at = 16 + shift
    for _, streams, _, _ in cases:
        w = []
        for s in streams:
            assert at % 16 == shift
            w.append((at, len(s)))
            pad = pad_to(at + len(s))
            parts += [bytes(s), bytes([FILL]) * pad]
            at += len(s) + pad
        where.append(w)
    blob = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to("cuda:0")
    doff, total = [], 0
    for _, _, want, _ in cases:
        total += GUARD
        total += (shift - total) % 16
        doff.append(total)
        total += want.size + SPARE + GUARD
    dest = torch.full((total,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert blob.data_ptr() % 16 == 0 and dest.data_ptr() % 16 == 0
    jobs = [([(blob.data_ptr() + a, n) for a, n in w], _orc.NO_LOCK, dest.data_ptr() + o, c[2].size + SPARE) for c, w, o in zip(cases, where, doff)]
    dl, un = h.decode_contigs_dev(p, jobs)
    out = dest.cpu().numpy()
    wrong = []
    for k, ((label, _, want, unmatched), o) in enumerate(zip(cases, doff)):
        n = want.size
        got = out[o:o + n]
        why = None
        if int(dl[k]) != n or int(un[k]) != unmatched:
            why = "destLen %d, unmatchedChars %d; expected %d, %d" % (dl[k], un[k], n, unmatched)
        elif not np.array_equal(got, want):
            d = int(np.flatnonzero(got != want)[0])
            why = "byte %d of %d is 0x%02x, expected 0x%02x (%d bytes differ)" % (d, n, got[d], want[d], int((got != want).sum()))
        elif not (out[o - GUARD:o] == FILL).all() or not (out[o + n + SPARE:o + n + SPARE + GUARD] == FILL).all():
            why = "guard bytes overwritten"
        elif not (out[o + n:o + n + SPARE] == FILL).all():
            why = "the 16 spare bytes behind the contig overwritten"
        if why:
            wrong.append("%s: %s" % (label, why))
    return wrong


@pytest.mark.parametrize("shift", [0, 1, 5, 15])
@pytest.mark.parametrize("sname", [n for n, _, _ in D.A_SETS])
def test_hand_written_streams_give_the_numpy_expectation(binding, handle, sname, shift):
    p = D.a_params(binding.emit_params, sname)
    assert bytes(p) == bytes(D.a_params(_orc.emit_params, sname))
    ref = D.ref_buffer()
    cases = [("%s / %s, moved by %d" % (sname, name, shift), h.streams(bool(p.frugal64bitLenEncoding), bool(p.enable40bitReference)), h.expect(ref), h.unmatched())
             for name, h in D.hand_contigs().items()]
    wrong = decode_jobs(handle, p, cases, shift)
    print("%s, moved by %d: %d jobs, %d disagree" % (sname, shift, len(cases), len(wrong)))
    assert not wrong, "\n".join(wrong[:12])


@pytest.mark.parametrize("sname", [n for n, _ in D.B_SETS])
def test_oracle_written_gap_contigs_decode_back(binding, handle, sname):
    key = dict(D.B_SETS)[sname]
    p = E.params_of(binding.emit_params, key)
    assert bytes(p) == bytes(E.params_of(_orc.emit_params, key))
    R = D.referee()
    cases = []
    for name, g in D.gap_contigs().items():
        e = R.emit_rows(g, key)
        cases.append(("%s / %s" % (sname, name), e["streams"], g.contig, e["unmatched"] & 0xFFFFFFFF))
    wrong = decode_jobs(handle, p, cases)
    print("%s: %d jobs, %d disagree" % (sname, len(cases), len(wrong)))
    assert not wrong, "\n".join(wrong[:12])


@pytest.mark.parametrize("sname", [n for n, _ in D.B_SETS])
def test_device_emission_verifies_and_a_change_inside_a_wide_gap_is_named(binding, handle, sname):
    """the gap contigs matched and emitted on the device; where the matcher's rows are the pieces (the CPU test) the emission
    has the wide gap extensions of the corpus: a byte of the query changed inside one — a START|END extension behind its first
    64 bytes, an END-only one (s0 = 0) — is reported as that contig and that byte"""
    import torch
    key = dict(D.B_SETS)[sname]
    p = E.params_of(binding.emit_params, key)
    gaps = D.gap_contigs()
    names, contigs = list(gaps), [g.contig for g in gaps.values()]
    offs = np.zeros(len(contigs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([c.size for c in contigs])
    buf = torch.from_numpy(np.concatenate(contigs)).to("cuda:0")
    torch.cuda.synchronize()
    h = handle
    h.match_batch_dev(buf.data_ptr(), offs, E.MIN_LEN, None)
    counts = h.batch_counts()
    for name in ("gap_rate08", "planted_long", "gap_lanes"):
        i = names.index(name)
        assert counts[i] == len(gaps[name].rows) and np.array_equal(h.batch_matches(i, counts[i]), gaps[name].rows), name
    h.emit_batch(p, loaded=[h.loading_position()], n=len(contigs))
    assert h.emit_verify() == (0, -1, 2 ** 64 - 1)
    W = D.DEC_WIDE_MIN
    g = gaps["gap_rate08"]
    at, n, _ = [s for s in g.stretches if s[1] == 1_024][0]
    g2 = gaps["planted_long"]
    at2, n2, _ = [s for s in g2.stretches if s[2] in g2.planted and s[1] == W + 1][0]
    at3, n3, _ = [s for s in g2.stretches if s[2] in g2.planted and s[1] == 3_000][0]
    for name, pos in (("gap_rate08", at + 700), ("planted_long", at2 + W), ("planted_long", at3 + 2_000), ("gap_lanes", gaps["gap_lanes"].stretches[D.WAVE][0] + 999)):
        i = names.index(name)
        where = int(offs[i]) + pos
        old = int(buf[where])
        buf[where] = ord("N")
        torch.cuda.synchronize()
        assert h.emit_verify() == (1, i, pos), (name, pos)
        buf[where] = old
        torch.cuda.synchronize()
    assert h.emit_verify() == (0, -1, 2 ** 64 - 1)
