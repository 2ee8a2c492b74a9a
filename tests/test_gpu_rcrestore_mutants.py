"""The device's inverse of the `-m3` reverse-complement pass (mbgc_copmem_rc_restore_plan / _fill, mbgc_amd/csrc/copmem_restore.h)
against a referee on cut streams and maps no encoder wrote: the corpus of tests/_rcmut.py, whose conditions
tests/test_rcrestore_mutants_cpu.py holds without a GPU and all of which went through tests/rcrestore_emu.cpp under the sanitizers
first. One handle serves the whole module, and within a test plans of very different sizes follow one another: the handle's
buffers only grow, and what a larger plan left behind the end of d, len and cum must not matter to a smaller one.

A case the referee refuses must fail in the plan with -4 and a message that says malformed, and the same handle must restore a
fixed good stream right after. A case it accepts must give the referee's length and stats from the plan; then the fill runs
twice on the one plan — into a device buffer at an address that is no multiple of 16, with 64 guard bytes on both sides, and into
the handle's own buffer and host memory — and both times the bytes and the deepest chain are the referee's and the guards are
whole. A case the plan accepts against the referee is reported and NOT filled."""
import time

import numpy as np
import pytest

import _rcmut

pytestmark = pytest.mark.gpu
GUARD, FILL, SKEW = 64, 0xEE, 5
FAMILIES = ("edges", "dense", "chains", "fastpaths", "parity", "varints")


@pytest.fixture(scope="module")
def ssm():
    from mbgc_amd import copmem
    m = copmem.SimpleSequenceMatcher()
    yield m
    m.close()


def in_turns(cases):
    """largest, smallest, second largest, ... by the number of marks and then the length of the cut stream"""
    by = sorted(cases, key=lambda c: (c.cut.count(bytes([_rcmut.MARK])), len(c.cut)))
    out = []
    while by:
        out.append(by.pop())
        if by:
            out.append(by.pop(0))
    return out


def run(ssm, cases):
    """-> what disagrees with the referee, one line per case; {name: restored bytes} of the accepted ones"""
    import torch
    from mbgc_amd import binding
    good = _rcmut.good()
    wrong, restored = [], {}
    for c in in_turns(cases):
        try:
            n, stats, _ = ssm.rc_restore_plan(c.cut, c.map_off, c.map_len, c.off_bytes)
        except binding.SwsemError as e:
            if c.accepted:
                wrong.append("%s: refused (%s) what the referee accepts" % (c.label(), e))
            else:
                if "copmem error -4: " not in str(e) or "malformed" not in str(e):
                    wrong.append("%s: refused with %r (the referee: %s)" % (c.label(), str(e), c.ref))
                if ssm.rc_restore_sequence(good.cut, good.map_off, good.map_len, good.off_bytes)[0] != good.ref[0]:
                    wrong.append("%s: the good stream does not come back after the refusal" % c.label())
            continue
        if not c.accepted:
            wrong.append("%s: planned (%d bytes) what the referee refuses: %s" % (c.label(), n, c.ref))
            continue                                                            # (and is not filled)
        want, m, total, deep, min_len = c.ref
        if n != len(want) or tuple(stats) != (m, total, 0, min_len):
            wrong.append("%s: length %d, stats %s; the referee: %d, %s" % (c.label(), n, tuple(stats), len(want), (m, total, 0, min_len)))
            continue
        buf = torch.full((GUARD + SKEW + n + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        at = GUARD + SKEW
        assert (buf.data_ptr() + at) % 16
        host1, _, deep1 = ssm.rc_restore_fill(n, cap=n, dst_dev=buf.data_ptr() + at)
        dev = buf.cpu().numpy()
        host2, _, deep2 = ssm.rc_restore_fill(n)
        why = None
        if not (dev[:at] == FILL).all() or not (dev[at + n:] == FILL).all():
            why = "guard bytes overwritten"
        elif dev[at:at + n].tobytes() != want or host1 != want or host2 != want:
            got = next(g for g in (dev[at:at + n].tobytes(), host1, host2) if g != want)
            d = int(np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))[0])
            why = "byte %d of %d is 0x%02x, the referee's 0x%02x" % (d, n, got[d], want[d])
        elif (deep1, deep2) != (deep, deep):
            why = "deepest chain %d and %d, the referee's %d" % (deep1, deep2, deep)
        if why:
            wrong.append("%s: %s" % (c.label(), why))
        restored[c.name] = want if why is None else None
    return wrong, restored


@pytest.mark.parametrize("family", FAMILIES)
def test_constructed_cases(ssm, family):
    """both widths of an offset in one run: the 8-byte form of a case gives the bytes of its 4-byte form"""
    cases = [c for c in _rcmut.constructed() if c.family in (family, family + "/8")]
    assert cases and all(c.accepted for c in cases)
    wrong, restored = run(ssm, cases)
    print("%s: %d cases, %d disagree" % (family, len(cases), len(wrong)))
    assert not wrong, "\n".join(wrong[:12])
    eights = [c for c in cases if c.off_bytes == 8]
    assert eights and all(restored[c.name] == restored[c.name[:-len(" [8-byte offsets]")]] for c in eights)


@pytest.mark.parametrize("cls", _rcmut.CLASSES)
def test_mutants(ssm, cls):
    cases = _rcmut.mutants(cls)
    wrong, _ = run(ssm, cases)
    print("%s: %d cases, %d accepted, %d disagree" % (cls, len(cases), sum(c.accepted for c in cases), len(wrong)))
    assert not wrong, "\n".join(wrong[:12])


def test_grid_stride(ssm):
    """a little over 32 MiB restored: the fill, k_mark_count and k_mark_write take more than one tile per workgroup. Its own time
    limit: the device's work on the one case, two fills and three copies of 32 MiB included, within 30 s"""
    cases = [c for c in _rcmut.constructed() if c.family == "grid"]
    assert len(cases) == 1 and len(cases[0].cut) > _rcmut.GRID_TILES * 128 and len(cases[0].ref[0]) > _rcmut.GRID_TILES * _rcmut.TILE
    small = _rcmut.constructed_by_name("edge: 17 bytes, the last of them a match's")
    t0 = time.time()
    wrong, _ = run(ssm, [cases[0], small])
    took = time.time() - t0
    print("grid stride: %.2f s" % took)
    assert not wrong, "\n".join(wrong)
    assert took < 30
