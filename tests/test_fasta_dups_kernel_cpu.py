"""k_fa_dups and k_fa_dups_verify without a GPU: the lane steps and the arithmetic (mbgc_amd/csrc/fasta_dups.h holds no HIP call) compiled as
plain C++ with AddressSanitizer and UBSan and run as a program of its own, tile by tile, lane by lane, the wave's shuffles emulated by
arrays, against byte loops written the obvious way (tests/fasta_dups_emu.cpp): the two strand fingerprints of every record modulo every
prime, the comp table over all 256 bytes, and the verdict of the exactness step for every two records of equal length on both strands.
The text is exactly seqBytes long: a read outside the buffer ends the run. The program says how many pairs it found equal on the reverse
strand and how many it refuted, and a floor is asked for both here, so that "ok" cannot mean "nothing compared". Says nothing about the
compiled device code, the shuffles, the sums in LDS, the atomics or the rounds on the host — that is tests/test_gpu_fasta_dups.py's job."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_steps_equal_the_byte_loop_under_asan(tmp_path):
    exe = str(tmp_path / "emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-strict-aliasing",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fasta_dups_emu.cpp")], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.match(r"ok: 200 calls, (\d+) residues equal the byte loop's; pairs compared: (\d+) equal forward, (\d+) equal on the reverse strand, (\d+) refuted", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 8000 and int(m.group(3)) >= 100 and int(m.group(4)) >= 1000, r.stdout
