"""The device decoder (k_decode_plan / k_decode_fill, mbgc_amd/csrc/swsem_decode.hip) against a referee on streams no encoder
wrote: the mutant corpus of tests/_decmut.py, whose conditions tests/test_decode_mutants_cpu.py holds without a GPU. Per parameter
row every case is one job of a single swsem_decode_contigs_dev call against a handle that holds the oracle's buffer, the poked
bytes included. An accepted case must give the referee's unmatchedChars, destLen and bytes; a rejected one -1; and no job
writes outside its destination (64 guard bytes in front and behind, and for an accepted case the 16 spare bytes of destCap).
The streams lie in one buffer with bytes of 0xEE between them: a read past a stream's end would see set flags and marks' neighbours."""
import numpy as np
import pytest

import _decmut

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xEE


@pytest.mark.parametrize("name", [n for n, _ in _decmut.ROWS])
def test_device_decoder_agrees_with_the_referee(name):
    import torch
    from mbgc_amd import binding
    r, cases = _decmut.row(name), _decmut.corpus(name)
    p = binding.EmitParams.from_buffer_copy(bytes(r.params))
    assert bytes(p) == bytes(binding.emit_params(r.mode, **r.over))              # the row's parameters are the device's own for the mode
    h = binding.SlidingWindowSparseEMMatcher(_decmut.REF_MAX, skip_margin=24 if r.mode >= 2 else 16)
    assert h.max_ref_length() == _decmut.REF_MAX
    h.write_ref(0, r.ref[:_decmut.REF_MAX])
    # the streams of every case in one upload, the destinations in one allocation
    parts, at, where = [], 0, []
    for c in cases:
        w = []
        for s in c.streams:
            pad = 16 + (-(at + len(s)) % 16)
            w.append((at, len(s)))
            parts += [s, bytes([FILL]) * pad]
            at += len(s) + pad
        where.append(w)
    blob = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to("cuda:0")
    doff, total = [], 0
    for c in cases:
        doff.append(total + GUARD)
        total += GUARD + c.dest_cap() + GUARD
    dest = torch.full((total,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    jobs = [([(blob.data_ptr() + a, n) for a, n in w], r.lock, dest.data_ptr() + o, c.dest_cap()) for c, w, o in zip(cases, where, doff)]
    dl, un = h.decode_contigs_dev(p, jobs)
    out = dest.cpu().numpy()
    h.close()
    wrong = []
    for k, (c, o) in enumerate(zip(cases, doff)):
        cap = c.dest_cap()
        why = None
        if not (out[o - GUARD:o] == FILL).all() or not (out[o + cap:o + cap + GUARD] == FILL).all():
            why = "guard bytes overwritten"
        elif c.accepted:
            got = out[o:o + c.dest_len]
            if int(un[k]) != c.unmatched or int(dl[k]) != c.dest_len:
                why = "unmatched %d, destLen %d; the referee: %d, %d" % (un[k], dl[k], c.unmatched, c.dest_len)
            elif not np.array_equal(got, c.expect):
                d = int(np.flatnonzero(got != c.expect)[0])
                why = "byte %d of %d is 0x%02x, the referee's 0x%02x" % (d, c.dest_len, got[d], c.expect[d])
            elif not (out[o + c.dest_len:o + cap] == FILL).all():
                why = "bytes written behind the contig"
        elif int(un[k]) != -1:
            why = "decoded (unmatched %d, destLen %d) what the referee rejects" % (un[k], dl[k])
        if why:
            wrong.append("%s: %s" % (c.label(), why))
    print("row %s: %d jobs, %d accepted, %d disagree" % (name, len(cases), sum(c.accepted for c in cases), len(wrong)))
    assert not wrong, "\n".join(wrong[:12])
