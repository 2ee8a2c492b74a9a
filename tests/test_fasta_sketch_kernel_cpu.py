"""k_fa_sketch without a GPU: the lane steps (mbgc_amd/csrc/fasta_sketch.h holds no HIP call) compiled as plain C++ with AddressSanitizer
and UBSan and run as a program of its own, tile by tile, lane by lane, the wave's shuffles emulated by arrays, over texts over
ACGTNacgtnRYU>\\0 and records that start at every offset mod 16, have 0, k - 1, k and k + 1 bytes and end on the buffer's last byte,
around a tile's edge and around a wave's edge, against a byte loop that builds every k-mer from scratch and its reverse complement by
reversing the string (tests/fasta_sketch_emu.cpp). k = 1, 2, 15, 16, 17, 31, 32: the 32-bit word boundary of the packed codes, the
reach into the second neighbour, and the 64-bit shift (UBSan ends the run on a shift by 64). The text is exactly seqBytes long: a read
outside the buffer ends the run. The program says how many k-mers it compared per k, and at least 10 000 are asked for here, with a
k-mer that is its own reverse complement at every even k, so that "ok" cannot mean "nothing to compare". Says nothing about the
compiled device code, the shuffles, the cursor, the sort or the pair kernel — that is tests/test_gpu_fasta_sketch.py's job."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_the_byte_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_sketch_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), r.stdout[-3000:] + r.stderr[-3000:]
    seen = {int(k): (int(n), int(p)) for k, n, p in re.findall(r"^k (\d+): (\d+) k-mers compared, (\d+) palindromic", r.stdout, flags=re.M)}
    assert sorted(seen) == [1, 2, 15, 16, 17, 31, 32], r.stdout
    for k, (compared, palindromic) in seen.items():
        assert compared >= 10_000, r.stdout
        assert k % 2 or palindromic >= 1, r.stdout
