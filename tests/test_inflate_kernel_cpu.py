"""k_fa_inflate without a GPU: the decoder (mbgc_amd/csrc/fasta_inflate.h holds no HIP call) compiled as plain C++ with AddressSanitizer
and UBSan and run over the whole corpus of tests/_inflate_cases.py, the streams that must fail included (tests/fasta_inflate_emu.cpp).
Input and output are exactly as long as declared: a read or a write past either end ends the run. Says nothing about the compiled
device code or the wave's lockstep — that is tests/test_gpu_inflate.py's job."""
import os
import subprocess

import _inflate_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


def test_corpus_is_what_it_claims():
    names = [c[0] for c in cases.corpus()]
    assert len(set(names)) == len(names)
    for name, stream, cap, status, want in cases.corpus():
        if status == cases.OK:
            assert want == cases.ref_inflate(stream) and cap >= len(want)


def test_decoder_over_the_corpus_under_asan(tmp_path):
    exe, corpus = str(tmp_path / "emu"), str(tmp_path / "corpus.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(HERE, "fasta_inflate_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    cases.write_corpus(corpus)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: %d cases" % len(cases.corpus())
