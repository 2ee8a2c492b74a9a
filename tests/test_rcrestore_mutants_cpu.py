"""The corpus of tests/_rcmut.py without a GPU: the referee (tests/_rcrestore.py, restore_bounded) against the unbounded
restatement of the reference's loop; the conditions the corpus must meet so that the device test (tests/test_gpu_rcrestore_mutants.py)
means something; and the whole corpus through tests/rcrestore_emu.cpp — what one item or lane of the device's kernels does
(mbgc_amd/csrc/copmem_restore_lane.h) as plain C++ under AddressSanitizer and UBSan against exactly sized buffers, with and without
the vector paths. A class of cases that this program cannot show to be in bounds does not go to the device."""
import os
import subprocess

import pytest

import _rcmut
import _rcrestore

HERE = os.path.dirname(os.path.abspath(__file__))


def small(c):
    return len(c.cut) < 1 << 20


def test_the_referee_equals_the_restatement_where_it_accepts():
    seen = 0
    for c in _rcmut.everything():
        if c.accepted and small(c):
            assert _rcrestore.restore(c.cut, c.map_off, c.map_len, c.off_bytes) == c.ref[0], c.label()
            seen += 1
    assert seen > 700


def test_a_refused_source_is_the_references_throw_or_truncation():
    seen = {"throw": 0, "short": 0}
    for c in _rcmut.everything():
        if not c.accepted and c.ref.startswith("source"):
            vals = _rcrestore.values_of(c.map_len)
            promised = len(c.cut) - (len(vals) - 1) + sum(v for v, _ in vals[1:]) + (len(vals) - 1) * vals[0][0]
            if promised > 1 << 32:                                               # (a huge length: the restatement would build it)
                continue
            try:
                got = _rcrestore.restore(c.cut, c.map_off, c.map_len, c.off_bytes)
            except IndexError:
                seen["throw"] += 1
                continue
            assert len(got) < promised, c.label()
            seen["short"] += 1
    assert seen["throw"] >= 5 and seen["short"] >= 5, seen


def test_constructed_cases_are_accepted():
    cases = _rcmut.constructed()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.accepted, (c.label(), c.ref)
    by = lambda name: _rcmut.constructed_by_name(name).ref
    assert by("chain: a ladder of depth %d" % _rcmut.LADDER_DEPTH)[3] == _rcmut.LADDER_DEPTH
    assert [by("chain: depth %d" % k)[3] for k in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert by("chain: depths 1 to 5 by hand")[3] == 5
    assert by("dense: 5000 marks and nothing else, 0 bytes restored")[:2] == (b"", 5000)
    g = _rcmut.constructed_by_name(next(c.name for c in cases if c.family == "grid"))
    assert _rcmut.GRID_TILES * _rcmut.TILE < len(g.cut) < len(g.ref[0]) < (_rcmut.GRID_TILES + 64) * _rcmut.TILE and 200 <= g.ref[1] <= 1000
    for c in cases:
        if c.off_bytes == 8:                                                     # the same bytes as the 4-byte run of the case
            assert c.ref == by(c.name[:-len(" [8-byte offsets]")]), c.name


def counts():
    return {cls: (sum(c.accepted for c in _rcmut.mutants(cls)), sum(not c.accepted for c in _rcmut.mutants(cls))) for cls in _rcmut.CLASSES}


def test_every_class_of_mutants_has_its_share():
    n = counts()
    print("mutants accepted / refused per class: %s" % n)
    for cls in _rcmut.CLASSES:
        acc, ref = n[cls]
        assert acc + ref == _rcmut.PER_CLASS
        assert len({(c.cut, c.map_off, c.map_len) for c in _rcmut.mutants(cls)}) >= _rcmut.PER_CLASS - 4, cls
        if cls in _rcmut.MAY_BE_ACCEPTED:
            assert 4 * acc >= _rcmut.PER_CLASS and ref >= 5, (cls, acc, ref)
        else:
            assert acc == 0, (cls, acc)
    for b, _ in _rcmut.bases():
        assert 5000 <= b.pos <= 40000
    assert any("beyond 32 bits" in c.ref for c in _rcmut.mutants("minlen") if not c.accepted)
    assert any("2^62" in c.ref for c in _rcmut.mutants("length") + _rcmut.mutants("minlen") if not c.accepted)
    assert any(c.off_bytes == 8 and int.from_bytes(c.map_off[8 * i + 4:8 * i + 8], "little") for c in _rcmut.mutants("offset")
               for i in range(len(c.map_off) // 8))                              # a high half that is not zero


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rcmut") / "corpus.bin")
    _rcmut.write_corpus(path, _rcmut.everything())
    return path


@pytest.mark.parametrize("form", ["vector paths", "bytewise"])
def test_the_lane_and_item_bodies_under_the_sanitizers(corpus_file, tmp_path, form):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas"] +
                   (["-DMBGC_RC_RESTORE_BYTEWISE"] if form == "bytewise" else []) +
                   ["-o", exe, os.path.join(HERE, "rcrestore_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, corpus_file], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-6000:]
    cases = _rcmut.everything()
    acc = sum(c.accepted for c in cases)
    assert r.stdout.strip().splitlines()[-1] == "ok: %d values, %d cases, %d accepted, %d refused, deepest chain %d" % (
        sum(len(w) for _, w in _rcmut.varint_streams()), len(cases), acc, len(cases) - acc, _rcmut.LADDER_DEPTH)
