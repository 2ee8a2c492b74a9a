"""k_fa_crc without a GPU: the lane steps and the host's table builder (mbgc_amd/csrc/fasta_crc.h holds no HIP call) compiled as
plain C++ with AddressSanitizer and run row by row, lane by lane, with both table lookups, over ranges of every size class (0 bytes
to several pieces; random, all 0x00, all 0xff, four letters; every alignment) against a bitwise CRC loop written the obvious way
(tests/fasta_crc_emu.cpp). Every range stands in an allocation that ends with it and whose bytes in front of it are poisoned: a read
outside a range ends the run. Says nothing about the compiled device code, the shuffles or the atomic — that is
tests/test_gpu_fasta_crc.py's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_plain_crc_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(HERE, "fasta_crc_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: 300 calls"
