"""The mutant corpus of tests/_decmut.py and its referee, without a GPU: the corpus is what tests/test_gpu_decode_mutants.py
takes it for (enough cases, enough of them accepted, every class on both sides, nothing decided by the device's ring guard or
by the slack behind a handle's buffer), the bounded decoder is the reference-pinned one on everything an encoder wrote, and it
stays inside its buffers on everything else (tests/decode_oracle_main.c under AddressSanitizer and UBSan, a program of its own)."""
import os
import subprocess

import numpy as np
import pytest

import _decmut
import _orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_NAMES = [n for n, _ in _decmut.ROWS]


@pytest.mark.parametrize("name", ROW_NAMES)
def test_corpus_meets_its_conditions(name):
    cases = _decmut.corpus(name)
    cnt = _decmut.counts(cases)
    print("row %s: %d cases, %d accepted" % (name, len(cases), sum(c.accepted for c in cases)))
    for cls in _decmut.CLASSES + ("leftover",):
        print("  %-10s accepted %3d  rejected %3d" % ((cls,) + cnt.get(cls, (0, 0))))
    assert len(cases) >= 300 and 2 * sum(c.accepted for c in cases) >= len(cases)
    assert len({c.seed for c in cases}) == len(cases)
    for cls in _decmut.CLASSES:
        assert cnt[cls][0] > 0, cls
    assert cnt["leftover"] == (0, _decmut.LEFTOVER)
    for c in cases:
        assert c.walk <= 128, c.label()                                  # the device's 4 x 128 guard never decides
        assert c.slack_same, c.label()                                   # nor do the bytes behind a handle's buffer
        if c.accepted:
            assert c.unmatched >= 0 and c.expect.size == c.dest_len <= _decmut.ORACLE_CAP - 16
        else:
            assert c.unmatched == -1


def test_every_class_rejects_somewhere():
    """(a flipped flag only rejects where the flags then run out: a few cases of the whole corpus, not of every row)"""
    total = {}
    for name in ROW_NAMES:
        for cls, (a, b) in _decmut.counts(_decmut.corpus(name)).items():
            total[cls] = total.get(cls, 0) + b
    assert all(total[cls] > 0 for cls in _decmut.CLASSES), total


@pytest.mark.parametrize("name", ROW_NAMES)
def test_bounded_decoder_is_the_pinned_one_on_emitted_streams(name):
    """orc_decode_contig is the bounded form without a bound plus full consumption; on the un-mutated streams of every contig the
    two agree with each other and give the contig back, with every stream read to its end"""
    r = _decmut.row(name)
    if name == "m1-lock":
        assert r.lock == _decmut.LOCK_POS and r.base[4][2] > 50
    for (streams, un, nmatch), contig in zip(r.base, r.contigs):
        back, un2 = _orc.decode_contig(r.clean_ref, r.params, dict(zip(_orc.STREAM_NAMES, streams)), r.lock, contig.size + 16)
        b = _orc.decode_contig_bounded(r.clean_ref, _decmut.REF_MAX, r.params, streams, r.lock, contig.size + 16)
        assert np.array_equal(back, contig) and np.array_equal(b["dest"], contig)
        assert b["unmatched"] == un2 == un and b["cur"] == [len(s) for s in streams]
    assert sum(b[2] for b in r.base) > 1000


def test_referee_stays_in_bounds_under_asan(tmp_path):
    exe, corpus = str(tmp_path / "referee"), str(tmp_path / "corpus.bin")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", _orc.ORACLE_DIR, "-o", exe,
                    os.path.join(HERE, "decode_oracle_main.c"), os.path.join(_orc.ORACLE_DIR, "decode_oracle.c")],
                   check=True, capture_output=True, text=True, timeout=300)
    n = _decmut.write_corpus(corpus)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: %d cases" % n and n == sum(len(_decmut.corpus(name)) for name in ROW_NAMES)
