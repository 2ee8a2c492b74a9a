"""mbgc_fasta_deflate_dev (k_fa_deflate, k_fa_deflate_pack: text in HBM becomes gzip files there) through the ctypes mirror, on torch
buffers, over the corpus of tests/_deflate_cases.py — the texts tests/test_deflate_kernel_cpu.py has already run through the encoder's
text on the CPU under AddressSanitizer. Every output is inflated by Python's zlib and by the project's own inflate_dev; sizes keep
the class bars (computed with zlib in _deflate_cases.py); nothing outside the gzip bytes is written; the bytes are those of the CPU
emulation of the same header."""
import functools
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import _deflate_cases as cases

pytestmark = pytest.mark.gpu
PATTERN = 0xC3
SLACK = 64


@functools.lru_cache(maxsize=None)
def device_run(name):
    """the call `name` of the corpus on the device -> (results, total, gzip buffer as numpy (with SLACK bytes behind), the text buffer read back)"""
    import torch
    from mbgc_amd import fasta
    _, buf, jobs, _ = [c for c in cases.calls() if c[0] == name][0]
    cap = sum(cases.bound(n) for _, n in jobs)
    text_dev = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to("cuda:0")
    gz_dev = torch.full((cap + SLACK,), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        results, total, ms = p.deflate_dev(text_dev.data_ptr(), len(buf), jobs, gz_dev.data_ptr(), cap)
    finally:
        p.close()
    return results, total, gz_dev.cpu().numpy(), text_dev.cpu().numpy().tobytes()


NAMES = [c[0] for c in cases.calls()]


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_guards_and_bars(name):
    _, buf, jobs, kinds = [c for c in cases.calls() if c[0] == name][0]
    results, total, gz, text_back = device_run(name)
    assert text_back == buf                                                       # the text and the guard bytes around every job
    assert (gz[total:] == PATTERN).all(), "a byte behind the gzip files was written"
    at = 0
    for (off, n), kind, (out_off, out_len, crc, chunks, stored) in zip(jobs, kinds, results):
        text = buf[off: off + n]
        assert out_off == at and chunks == cases.chunks_of(n) and stored <= chunks
        blob = gz[out_off: out_off + out_len].tobytes()
        z = zlib.decompressobj(31)
        assert z.decompress(blob) == text and z.eof and not z.unused_data, name
        assert blob[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff])
        assert struct.unpack("<II", blob[-8:]) == (zlib.crc32(text), n % 2 ** 32) and crc == zlib.crc32(text)
        lim = cases.limit(kind, text)
        print("%s (%s): %d bytes of text, %d of gzip, bar %d, %d of %d chunks stored" % (name, kind, n, out_len, lim, stored, chunks))
        assert out_len <= lim and out_len <= cases.bound(n), (name, out_len, lim)
        if kind == cases.RANDOM:
            assert stored == chunks
        at += out_len
    assert at == total
    if name == "empty":
        assert total == 20


def test_one_byte_short_is_refused_with_the_size_and_nothing_written():
    import torch
    from mbgc_amd import binding, fasta
    _, buf, jobs, _ = [c for c in cases.calls() if c[0] == "three_jobs"][0]
    _, total, _, _ = device_run("three_jobs")
    text_dev = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to("cuda:0")
    gz_dev = torch.full((total + SLACK,), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        with pytest.raises(fasta.GzipTooSmall) as e:
            p.deflate_dev(text_dev.data_ptr(), len(buf), jobs, gz_dev.data_ptr(), total - 1)
        assert e.value.needed == total
        assert (gz_dev.cpu().numpy() == PATTERN).all()
        # a job past the buffer's end: refused, nothing launched
        for bad in ([(0, len(buf) + 1)], [(len(buf) + 1, 0)], [(1, len(buf))], [(2 ** 63, 2 ** 63)], [jobs[0], (len(buf) - 3, 4)]):
            with pytest.raises(binding.SwsemError) as e:
                p.deflate_dev(text_dev.data_ptr(), len(buf), bad, gz_dev.data_ptr(), total)
            assert not isinstance(e.value, fasta.GzipTooSmall) and "outside the text" in str(e.value)
        assert (gz_dev.cpu().numpy() == PATTERN).all()
        results, again, ms = p.deflate_dev(text_dev.data_ptr(), len(buf), jobs, gz_dev.data_ptr(), total)      # exactly enough
        assert again == total and ms > 0
        assert (gz_dev.cpu().numpy()[total:] == PATTERN).all()
    finally:
        p.close()


def test_same_bytes_on_every_run_and_in_any_company():
    import torch
    from mbgc_amd import fasta
    _, buf, jobs, _ = [c for c in cases.calls() if c[0] == "three_jobs"][0]
    results, total, gz, _ = device_run("three_jobs")
    text_dev = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to("cuda:0")
    gz_dev = torch.full((total,), PATTERN, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = fasta.FastaParser()
    try:
        _, again, _ = p.deflate_dev(text_dev.data_ptr(), len(buf), jobs, gz_dev.data_ptr(), total)
    finally:
        p.close()
    assert again == total and gz_dev.cpu().numpy().tobytes() == gz[:total].tobytes()
    for single, (out_off, out_len, _, _, _) in zip(cases.THREE_JOBS, results):                                   # a job alone, at another alignment
        r1, t1, g1, _ = device_run(single)
        assert g1[:t1].tobytes() == gz[out_off: out_off + out_len].tobytes(), single


def test_the_projects_own_inflate_reads_every_output():
    """the "complete code sets" promise against an independent reader on the device: inflate_dev refuses incomplete sets"""
    import torch
    from mbgc_amd import fasta
    p = fasta.FastaParser()
    try:
        for name, buf, jobs, _ in cases.calls():
            results, total, gz, _ = device_run(name)
            gz_dev = torch.from_numpy(gz[:max(total, 1)].copy()).to("cuda:0")
            out_cap = sum(n for _, n in jobs)
            out_dev = torch.full((out_cap + 16,), PATTERN, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            inf_jobs, at = [], 0
            for (off, n), (out_off, out_len, _, _, _) in zip(jobs, results):
                inf_jobs.append((out_off, out_len, at, n))
                at += n
            res, _ = p.inflate_dev(gz_dev.data_ptr(), total, out_dev.data_ptr(), out_cap + 16, inf_jobs)
            out = out_dev.cpu().numpy()
            for (off, n), (in_off, in_len, o, cap), (st, members, out_len, in_used) in zip(jobs, inf_jobs, res):
                assert (st, members, out_len, in_used) == (fasta.INFLATE_OK, 1, n, in_len), name
                assert out[o: o + n].tobytes() == buf[off: off + n], name
    finally:
        p.close()


def test_bytes_are_those_of_the_cpu_emulation():
    if shutil.which("g++") is None:
        pytest.skip("no g++: the CPU emulation of fasta_deflate.h cannot be built")
    import test_deflate_kernel_cpu as cpu
    with tempfile.TemporaryDirectory() as tmp:
        exe, corpus, out = (os.path.join(tmp, f) for f in ("emu", "corpus.bin", "gz.bin"))
        cpu.build_emu(exe, sanitize=False)
        cases.write_corpus(corpus)
        r = subprocess.run([exe, corpus, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        want = cases.read_outputs(out)
    for name in NAMES:
        _, total, gz, _ = device_run(name)
        assert gz[:total].tobytes() == want[name], name
