"""k_fa_pack without a GPU: the lane step and the host's table builders (mbgc_amd/csrc/fasta_pack.h hold no HIP call) compiled as
plain C++ with AddressSanitizer and run lane step by lane step, tile by tile, over random piece tables against a byte loop written
the obvious way (tests/fasta_pack_emu.cpp). Both buffers are exactly as long as declared: a read or a write past either end ends the
run. Says nothing about the compiled device code — that is tests/test_gpu_fasta_pack.py's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_step_equals_plain_byte_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(HERE, "fasta_pack_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip() == "ok: 1500 calls"
