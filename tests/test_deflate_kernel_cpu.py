"""k_fa_deflate and k_fa_deflate_pack without a GPU: the encoder (mbgc_amd/csrc/fasta_deflate.h holds no HIP call) compiled as plain C++
with AddressSanitizer and UBSan and run over the corpus of tests/_deflate_cases.py (tests/fasta_deflate_emu.cpp): every gzip file
inflates with zlib to its text, the trailers are right, the code-length function keeps the Kraft sum at exactly 1 — and the sizes the
program reports keep the class bars, which are computed here with Python's zlib. Says nothing about the compiled device code or the
wave's lockstep: that is tests/test_gpu_deflate.py's job."""
import os
import subprocess
import zlib

import pytest

import _deflate_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


def build_emu(exe, sanitize=True):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++"] + flags + ["-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_deflate_emu.cpp"), "-lz"],
                   check=True, capture_output=True, text=True, timeout=300)


def test_the_corpus_meets_its_own_bars_with_zlib():
    """the bars ask nothing zlib's own Huffman-only encoder, flushed every 32 KiB, does not give"""
    names = [n for n, _, _ in cases.singles()]
    assert len(set(names)) == len(names)
    for name, text, kind in cases.singles():
        if kind == cases.HUFFMAN:
            assert cases.huffman_only(text, cases.CHUNK) <= cases.limit(kind, text), name
        assert cases.limit(kind, text) <= cases.bound(len(text)) or kind == cases.HUFFMAN, name
    by = {n: t for n, t, _ in cases.singles()}
    assert cases.huffman_only(by["n_run_100000"]) > len(by["n_run_100000"]) // 10          # no bar without a matcher
    assert cases.huffman_only(by["one_value_70000"]) > 7000


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deflate_emu")
    exe, corpus, out = str(tmp / "emu"), str(tmp / "corpus.bin"), str(tmp / "gz.bin")
    build_emu(exe)
    cases.write_corpus(corpus)
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True, timeout=300)
    return r, out


def test_encoder_over_the_corpus_under_asan(emu):
    r, out = emu
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "ok: %d calls" % len(cases.calls())


def test_sizes_keep_the_class_bars(emu):
    r, out = emu
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [l.split() for l in r.stdout.splitlines() if not l.startswith("ok:")]
    sizes = {(name, int(job)): (int(n), int(size), int(chunks), int(stored)) for name, job, n, size, chunks, stored in rows}
    gz = cases.read_outputs(out)
    for name, buf, jobs, kinds in cases.calls():
        at = 0
        for k, ((off, n), kind) in enumerate(zip(jobs, kinds)):
            got_n, size, chunks, stored = sizes[(name, k)]
            text = buf[off: off + n]
            assert got_n == n and chunks == cases.chunks_of(n)
            assert zlib.decompress(gz[name][at: at + size], 31) == text, (name, k)
            at += size
            lim = cases.limit(kind, text)
            print("%s job %d (%s): %d bytes of text, %d of gzip, bar %d, Z_HUFFMAN_ONLY %d, %d of %d chunks stored"
                  % (name, k, kind, n, size, lim, cases.huffman_only(text), stored, chunks))
            assert size <= lim and size <= cases.bound(n), (name, k, size, lim)
            if kind == cases.RANDOM:
                assert stored == chunks
        assert at == len(gz[name])
    assert sizes[("empty", 0)][1] == 20
