"""k_fa_format without a GPU: the kernel's body and the host's table builders (mbgc_amd/csrc/fasta_format.h hold no HIP call)
compiled as plain C++ with AddressSanitizer and run lane step by lane step against a formatter written the obvious way
(tests/fasta_format_emu.cpp): random batches over the line, sequence and header lengths and the buffer alignments that
tests/test_gpu_fasta_format.py runs on the device. Says nothing about the compiled device code — that is the GPU test's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_kernel_body_equals_plain_formatter_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(HERE, "fasta_format_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: 1500 batches"
