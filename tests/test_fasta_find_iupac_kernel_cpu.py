"""k_fa_find_iupac without a GPU: the lane step and the host's table builder (mbgc_amd/csrc/fasta_find_iupac.h holds no HIP call)
compiled as plain C++ with AddressSanitizer and UBSan and run tile by tile, lane by lane, over random texts, record lists and pattern
lists against a triple loop written from the matching rule alone (tests/fasta_find_iupac_emu.cpp): texts over ACGTacgtUuNnRY-, and a
zero byte, records at every off % 16, at the buffer's end, shorter than the shortest pattern and of exactly its length, touching,
overlapping and repeated, patterns over the whole letter table at K = 0..3, the same one twice, windows that are not their segment's
first, a window of exactly 256 grams (accepted) and one of 1024 (refused by the builder). The text, the pattern blob, the table's arrays
and the staging buffer are exactly as long as declared: a read outside the buffer ends the run. Says nothing about the compiled device
code, the barrier, the bitmap's copy in LDS or the atomic cursor — that is tests/test_gpu_fasta_find_iupac.py's job."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_the_triple_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_find_iupac_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.startswith("ok: 400 calls")
