"""Single fasta file mode under the lossy rule (`mbgc c -L -i`): the restatement tests/_singlefasta_lossy.py — mgmpInSplit_next's
elements, each read by kseq_read_lossy as a file of its own; under the sequential schedule the file as one stream — known
answers that need no reference, and, where oracle/_ref is built, held to what the reference's own `mbgc c -L -i` + `mbgc d` write
back for damaged files in both schedules: every element's records come back at that element's own longest line (the reference's
README: "the file is compressed in blocks and each block stores the length of the longest sequence line within that block").
No GPU."""
import os
import subprocess

import pytest

import _refh
import _singlefasta as sfa
import _singlefasta_lossy as sfl
from _fasta_lossy import lossy_parse


def test_split_records_known_answers():
    s = sfl.split_records
    d = b">a\nAC\n@b\nG>\n>c\nA@\n"                                  # marks at line starts: 0 '>', 6 '@', 12 '>'; inside lines: 10 '>', 16 '@'
    assert s(d, 0, 1, 0) == [10, 12, 18] and s(d, 0, 1, sfl.AT) == [6, 10, 12, 16, 18]
    assert s(d, 0, 1, sfl.LINE_START) == [12, 18] and s(d, 0, 1, sfl.LINE_START | sfl.AT) == [6, 12, 18]
    assert s(d, 0, 6, 3) == [6, 12, 18] and s(d, 0, 7, 3) == [12, 18]          # the threshold is inclusive
    assert s(d, 6, 1, 3) == [12, 18] and s(d, 6, (7, 1), 3) == [18]            # a start inside the buffer
    assert s(d, 0, 1, 3, is_file_end=False) == [6, 12] and s(d, 0, 13, 3, is_file_end=False) == []
    assert s(b">a\r\n>b\r>c\n", 0, 1, 3) == [4, 10]                           # CR LF '>' counts, CR '>' does not
    assert s(d, 0, 1, 3, max_elems=1) == [6] and s(b"", 0, 1, 3) == []
    for flags in range(4):                                                     # without line feeds or '@' the rules agree
        assert s(b">" * 10, 0, 3, flags & sfl.AT) == sfa.split_window(b">" * 10, True, 3, 3)


def test_restatement_known_answers():
    f = b"junk\nxx>h1 a > b\r\nACGT\r\nAC\r\n\r\n@h2\nGG\nGGGGG\n"
    p = sfl.sequential(f)
    assert p["records"] == [(b"h1 a > b", b"ACGTAC"), (b"h2", b"GGGGGGG")] and p["dna_line_len"] == 5
    assert sfl.sequential_text(f) == b">h1 a > b\nACGTA\nC\n>h2\nGGGGG\nGG\n"
    # cut as mgmpInSplit_next cuts: any '>' behind the threshold, also the one inside the header line
    e = sfa.elements(f, 8, 4)
    assert e == [f[:13], f[13:]] and [x["records"] for x in map(lossy_parse, e)] == [[(b"h1 a ", b"")], [(b" b", b"ACGTAC"), (b"h2", b"GGGGGGG")]]


def damaged_files():
    big, small = sfl.synth_single(8_600_000, 8, 5), sfl.synth_single(600_000, 6, 5)
    for f in (big, small):
        assert f.startswith(sfl.JUNK) and b"\r\n" in f and b"\n\n" in f and b"\n@" in f and b" a -> b" in f
    return big, small


def test_damaged_files_are_what_the_rule_is_for():
    big, small = damaged_files()
    ps = sfl.rounds(big)
    assert len(ps) >= 5 and all(p["status"] == 0 and p["records"] for p in ps)
    longest = sfl.sequential(big)["dna_line_len"]
    assert longest == 100 and sum(p["dna_line_len"] != longest for p in ps) >= 2          # "each block" has its own
    assert sfl.rounds_text(big) != sfl.sequential_text(big)
    assert len(sfa.elements(small)) < 5                                                    # the reference will fall back


@pytest.mark.skipif(not (_refh.available() and os.access(_refh.REF_MBGC, os.X_OK)), reason="oracle/_ref not built")
def test_restatement_equals_reference_cli(tmp_path):
    big, small = damaged_files()
    for name, data, text in (("big", big, sfl.rounds_text(big)), ("small", small, sfl.sequential_text(small)), ("big_t1", big, sfl.sequential_text(big))):
        (tmp_path / (name + ".fa")).write_bytes(data)
        args = ["-t1"] if name == "big_t1" else []
        r = subprocess.run([_refh.REF_MBGC, "c", "-L"] + args + ["-i", name + ".fa", name + ".mbgc"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert ("Switching to sequential matching mode" in r.stderr) == (name == "small"), r.stderr
        r = subprocess.run([_refh.REF_MBGC, "d", name + ".mbgc", name + "_out"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / (name + "_out") / (name + ".fa")).read_bytes() == text, name
