"""k_fa_find without a GPU: the lane steps, the search of a tile's record and the host's table builder (mbgc_amd/csrc/fasta_find.h holds
no HIP call) compiled as plain C++ with AddressSanitizer and UBSan and run tile by tile, lane by lane, over random texts, record
lists and pattern lists against a triple loop written the obvious way (tests/fasta_find_emu.cpp). The text, the pattern blob, the
table's arrays and the staging buffer are exactly as long as declared: a read outside the buffer ends the run, and a byte outside a
record that changed a result shows in the table of hits. Says nothing about the compiled device code, the barrier, the table's copy
in LDS or the atomic cursor — that is tests/test_gpu_fasta_find.py's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_the_triple_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_find_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("ok: 400 calls")
